"""hub entries of NPC under the reference's names and signatures (s3prl/upstream/npc/hubconf.py:17-61): ``npc_local(ckpt, *args,
**kwargs)``, ``npc_url(ckpt, refresh=False, *args, **kwargs)``, ``npc`` (= ``npc_360hr``), ``npc_360hr`` and ``npc_960hr``.  A URL
resolves to the reference's cache file (``s3prl_amd.download``)."""

import os

from ...download import urls_to_filepaths as _urls_to_filepaths
from .expert import UpstreamExpert as _UpstreamExpert


def npc_local(ckpt, *args, **kwargs):
    assert os.path.isfile(ckpt), ckpt
    return _UpstreamExpert(str(ckpt), *args, **kwargs)


def npc_url(ckpt, refresh=False, *args, **kwargs):
    return npc_local(_urls_to_filepaths(str(ckpt), refresh=refresh), *args, **kwargs)


def npc(refresh=False, *args, **kwargs):
    return npc_360hr(refresh=refresh, *args, **kwargs)


def npc_360hr(refresh=False, *args, **kwargs):
    kwargs["ckpt"] = "https://huggingface.co/leo19941227/apc_series/resolve/main/npc_360hr.ckpt"
    return npc_url(refresh=refresh, *args, **kwargs)


def npc_960hr(refresh=False, *args, **kwargs):
    kwargs["ckpt"] = "https://huggingface.co/leo19941227/apc_series/resolve/main/npc_960hr.ckpt"
    return npc_url(refresh=refresh, *args, **kwargs)
