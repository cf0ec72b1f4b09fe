"""AudioALBERT (``s3prl/upstream/audio_albert/expert.py`` re-exports Mockingjay's expert; ``share_layer`` comes with the checkpoint's
config): the same class, see ``upstream/mockingjay/expert.py``."""

from ..mockingjay.expert import UpstreamExpert  # noqa: F401
