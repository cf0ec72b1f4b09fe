"""TERA (``s3prl/upstream/tera/expert.py`` re-exports Mockingjay's expert): the same class, see ``upstream/mockingjay/expert.py``."""

from ..mockingjay.expert import UpstreamExpert  # noqa: F401
