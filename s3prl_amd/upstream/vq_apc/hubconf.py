"""hub entries of VQ-APC under the reference's names and signatures (s3prl/upstream/vq_apc/hubconf.py:10-40): ``vq_apc_url`` is
APC's ``apc_url``; ``vq_apc`` (= ``vq_apc_360hr``), ``vq_apc_360hr`` and ``vq_apc_960hr``."""

from ..apc.hubconf import apc_url as vq_apc_url


def vq_apc(refresh=False, *args, **kwargs):
    return vq_apc_360hr(refresh=refresh, *args, **kwargs)


def vq_apc_360hr(refresh=False, *args, **kwargs):
    kwargs["ckpt"] = "https://huggingface.co/leo19941227/apc_series/resolve/main/vq_apc_360hr.ckpt"
    return vq_apc_url(refresh=refresh, *args, **kwargs)


def vq_apc_960hr(refresh=False, *args, **kwargs):
    kwargs["ckpt"] = "https://huggingface.co/leo19941227/apc_series/resolve/main/vq_apc_960hr.ckpt"
    return vq_apc_url(refresh=refresh, *args, **kwargs)
