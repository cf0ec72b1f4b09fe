"""vq-wav2vec is the wav2vec expert on a checkpoint whose ``vq_type`` is ``gumbel`` or ``kmeans``
(s3prl/upstream/vq_wav2vec/expert.py re-exports wav2vec's)."""

from ..wav2vec.expert import UpstreamExpert  # noqa: F401
