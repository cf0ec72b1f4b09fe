"""hub entries of BYOL-A under the reference's names and signatures (s3prl/upstream/byol_a/hubconf.py:18-42):
``byol_a_2048`` / ``byol_a_1024`` / ``byol_a_512(refresh=False, **kwds)``; ``kwds`` carries ``window_secs`` / ``stride_secs``.  The
URLs resolve to the reference's cache files (``s3prl_amd.download``)."""

from pathlib import Path as _Path

from ...download import urls_to_filepaths as _urls_to_filepaths
from .expert import UpstreamExpert as _UpstreamExpert

DEFAULT_CONFIG_PATH = _Path(__file__).parent / "config.yaml"  # the reference's path; its front-end values are the ones built

_URL = "https://github.com/nttcslab/byol-a/raw/master/pretrained_weights/AudioNTT2020-BYOLA-64x96d{}.pth"


def byol_a_2048(refresh=False, **kwds):
    ckpt = _urls_to_filepaths(_URL.format(2048), refresh=refresh)
    return _UpstreamExpert(ckpt, DEFAULT_CONFIG_PATH, 2048, **kwds)


def byol_a_1024(refresh=False, **kwds):
    ckpt = _urls_to_filepaths(_URL.format(1024), refresh=refresh)
    return _UpstreamExpert(ckpt, DEFAULT_CONFIG_PATH, 1024, **kwds)


def byol_a_512(refresh=False, **kwds):
    ckpt = _urls_to_filepaths(_URL.format(512), refresh=refresh)
    return _UpstreamExpert(ckpt, DEFAULT_CONFIG_PATH, 512, **kwds)
