"""hub entries of DeCoAR-layers under the reference's names and signatures (s3prl/upstream/decoar_layers/hubconf.py):
``decoar_layers_custom(ckpt, refresh=False, *args, **kwargs)`` takes a path or a URL, ``decoar_layers_local`` / ``decoar_layers_url``
pass everything on to it, and ``decoar_layers`` names the released checkpoint — the file of ``decoar``."""

from ..decoar.hubconf import _RELEASED, _resolve
from .expert import UpstreamExpert as _UpstreamExpert


def decoar_layers_custom(ckpt: str, refresh=False, *args, **kwargs):
    return _UpstreamExpert(_resolve(ckpt, refresh), *args, **kwargs)


def decoar_layers_local(*args, **kwargs):
    return decoar_layers_custom(*args, **kwargs)


def decoar_layers_url(*args, **kwargs):
    return decoar_layers_custom(*args, **kwargs)


def decoar_layers(*args, refresh=False, **kwargs):
    return decoar_layers_url(*args, **dict(kwargs, ckpt=_RELEASED, refresh=refresh))
