"""hub entries of SSAST under the reference's names and signatures (s3prl/upstream/ssast/hubconf.py:16-33):
``ssast_frame_base`` and ``ssast_patch_base(refresh=False, window_secs=1.0, **kwargs)`` — 1 s windows for speech commands, 6 s for
IEMOCAP, 10 s for SID.  A URL resolves to the reference's cache file (``s3prl_amd.download``)."""

from ...download import urls_to_filepaths as _urls_to_filepaths
from .expert import UpstreamExpert as _UpstreamExpert


def ssast_frame_base(refresh: bool = False, window_secs: float = 1.0, **kwargs):
    ckpt = _urls_to_filepaths("https://www.dropbox.com/s/nx6nl4d4bl71sm8/SSAST-Base-Frame-400.pth?dl=1", refresh=refresh)
    return _UpstreamExpert(ckpt, "base_f", window_secs)


def ssast_patch_base(refresh: bool = False, window_secs: float = 1.0, **kwargs):
    ckpt = _urls_to_filepaths("https://www.dropbox.com/s/ewrzpco95n9jdz6/SSAST-Base-Patch-400.pth?dl=1", refresh=refresh)
    return _UpstreamExpert(ckpt, "base_p", window_secs)
