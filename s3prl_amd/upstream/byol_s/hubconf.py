"""hub entries of BYOL-S under the reference's names and signatures (s3prl/upstream/byol_s/hubconf.py:6-30):
``byol_s_default`` / ``byol_s_resnetish34(refresh=False, **kwds)``; ``kwds`` carries ``window_secs`` / ``hop_secs``.  The URLs
resolve to the reference's cache files (``s3prl_amd.download``).  ``byol_s_cvt`` is not registered: the CvT network is not built."""

from ...download import urls_to_filepaths as _urls_to_filepaths
from .expert import UpstreamExpert as _UpstreamExpert

_URL = "https://github.com/GasserElbanna/serab-byols/raw/main/checkpoints/"


def byol_s_default(refresh: bool = False, **kwds):
    kwds["model_name"] = "default"
    kwds["ckpt"] = _urls_to_filepaths(_URL + "default2048_BYOLAs64x96-2105311814-e100-bs256-lr0003-rs42.pth", refresh=refresh)
    return _UpstreamExpert(**kwds)


def byol_s_resnetish34(refresh: bool = False, **kwds):
    kwds["model_name"] = "resnetish34"
    kwds["ckpt"] = _urls_to_filepaths(_URL + "resnetish34_BYOLAs64x96-2105271915-e100-bs256-lr0003-rs42.pth", refresh=refresh)
    return _UpstreamExpert(**kwds)
