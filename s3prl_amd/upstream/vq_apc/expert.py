"""VQ-APC (``s3prl/upstream/vq_apc/expert.py`` re-exports APC's expert): the same class, see ``upstream/apc/expert.py``."""

from ..apc.expert import UpstreamExpert  # noqa: F401
