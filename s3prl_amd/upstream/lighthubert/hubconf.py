"""hub entries of LightHuBERT under the reference's names and signatures (s3prl/upstream/lighthubert/hubconf.py:8-64):
``lighthubert_local(ckpt, ...)``, ``lighthubert_url(ckpt, refresh=False, ...)`` and the released ``lighthubert`` (= Small),
``lighthubert_small``, ``lighthubert_base``, ``lighthubert_stage1``.  URLs resolve to the reference's cache file
(``s3prl_amd.download``)."""

import os

from ...download import urls_to_filepaths as _urls_to_filepaths
from .. import _released
from .expert import UpstreamExpert as _UpstreamExpert

_RELEASED = "https://huggingface.co/mechanicalsea/lighthubert/resolve/main/"


def lighthubert_local(ckpt, *args, **kwargs):
    assert os.path.isfile(ckpt), ckpt
    return _UpstreamExpert(ckpt, *args, **kwargs)


def lighthubert_url(ckpt, refresh=False, *args, **kwargs):
    return lighthubert_local(_urls_to_filepaths(str(ckpt), refresh=refresh), *args, **kwargs)


def lighthubert(refresh=False, *args, **kargs):
    """The default model - Small (lighthubert/hubconf.py:28-33; the catch-all is spelled ``kargs`` there)"""
    return lighthubert_small(refresh=refresh, *args, **kargs)


lighthubert_small = _released.positional("lighthubert_small", lighthubert_url, _RELEASED + "lighthubert_small.pt")
lighthubert_base = _released.positional("lighthubert_base", lighthubert_url, _RELEASED + "lighthubert_base.pt")
lighthubert_stage1 = _released.positional("lighthubert_stage1", lighthubert_url, _RELEASED + "lighthubert_stage1.pt")
