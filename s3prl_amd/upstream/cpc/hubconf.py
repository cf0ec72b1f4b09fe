"""hub entries of modified CPC under the reference's names and signatures (s3prl/upstream/cpc/hubconf.py:16-41):
``cpc_local(ckpt, *args, **kwargs)``, ``cpc_url(ckpt, refresh=False, *args, **kwargs)`` and ``modified_cpc`` (the released
``60k_epoch4`` checkpoint).  A URL resolves to the reference's cache file (``s3prl_amd.download``)."""

import os

from ...download import urls_to_filepaths as _urls_to_filepaths
from .expert import UpstreamExpert as _UpstreamExpert


def cpc_local(ckpt, *args, **kwargs):
    assert os.path.isfile(ckpt), ckpt
    return _UpstreamExpert(str(ckpt), *args, **kwargs)


def cpc_url(ckpt, refresh=False, *args, **kwargs):
    return cpc_local(_urls_to_filepaths(str(ckpt), refresh=refresh), *args, **kwargs)


def modified_cpc(refresh=False, *args, **kwargs):
    kwargs["ckpt"] = modified_cpc.url
    return cpc_url(refresh=refresh, *args, **kwargs)


modified_cpc.url = "https://dl.fbaipublicfiles.com/librilight/CPC_checkpoints/60k_epoch4-d0f474de.pt"
