"""hub entries of DeCoAR 2.0 under the reference's names and signatures (s3prl/upstream/decoar2/hubconf.py): ``decoar2_custom(ckpt,
refresh=False, *args, **kwargs)`` takes a path or a URL, ``decoar2_local`` / ``decoar2_url`` pass everything on to it, and
``decoar2(*args, refresh=False, **kwargs)`` names the released checkpoint.  A URL resolves to the reference's cache file
(``s3prl_amd.download``)."""

import os

from ...download import urls_to_filepaths as _urls_to_filepaths
from .expert import UpstreamExpert as _UpstreamExpert

_RELEASED = "https://huggingface.co/s3prl/converted_ckpts/resolve/main/checkpoint_decoar2.pt"


def _resolve(ckpt, refresh):
    path = _urls_to_filepaths(str(ckpt), refresh=refresh) if str(ckpt).startswith("http") else str(ckpt)
    assert os.path.isfile(path), path
    return path


def decoar2_custom(ckpt: str, refresh=False, *args, **kwargs):
    return _UpstreamExpert(_resolve(ckpt, refresh), *args, **kwargs)


def decoar2_local(*args, **kwargs):
    return decoar2_custom(*args, **kwargs)


def decoar2_url(*args, **kwargs):
    return decoar2_custom(*args, **kwargs)


def decoar2(*args, refresh=False, **kwargs):
    return decoar2_url(*args, **dict(kwargs, ckpt=_RELEASED, refresh=refresh))
