"""hub entries of APC under the reference's names and signatures (s3prl/upstream/apc/hubconf.py:17-61): ``apc_local(ckpt, *args,
**kwargs)``, ``apc_url(ckpt, refresh=False, *args, **kwargs)``, ``apc`` (= ``apc_360hr``), ``apc_360hr`` and ``apc_960hr``.  A URL
resolves to the reference's cache file (``s3prl_amd.download``)."""

import os

from ...download import urls_to_filepaths as _urls_to_filepaths
from .expert import UpstreamExpert as _UpstreamExpert


def apc_local(ckpt, *args, **kwargs):
    assert os.path.isfile(ckpt), ckpt
    return _UpstreamExpert(str(ckpt), *args, **kwargs)


def apc_url(ckpt, refresh=False, *args, **kwargs):
    return apc_local(_urls_to_filepaths(str(ckpt), refresh=refresh), *args, **kwargs)


def apc(refresh=False, *args, **kwargs):
    return apc_360hr(refresh=refresh, *args, **kwargs)


def apc_360hr(refresh=False, *args, **kwargs):
    kwargs["ckpt"] = "https://huggingface.co/leo19941227/apc_series/resolve/main/apc_360hr.ckpt"
    return apc_url(refresh=refresh, *args, **kwargs)


def apc_960hr(refresh=False, *args, **kwargs):
    kwargs["ckpt"] = "https://huggingface.co/leo19941227/apc_series/resolve/main/apc_960hr.ckpt"
    return apc_url(refresh=refresh, *args, **kwargs)
