"""hub entries of TERA under the reference's names and signatures (s3prl/upstream/tera/hubconf.py): ``tera_local(ckpt, *args,
**kwargs)``, ``tera_url(ckpt, refresh=False, *args, **kwargs)`` and the released names (``tera`` = ``tera_960hr``)."""

import os

from ...download import urls_to_filepaths as _urls_to_filepaths
from .expert import UpstreamExpert as _UpstreamExpert


def tera_local(ckpt, *args, **kwargs):
    assert os.path.isfile(ckpt), ckpt
    return _UpstreamExpert(str(ckpt), *args, **kwargs)


def tera_url(ckpt, refresh=False, *args, **kwargs):
    return tera_local(_urls_to_filepaths(str(ckpt), refresh=refresh), *args, **kwargs)


def tera(refresh=False, *args, **kwargs):
    return tera_960hr(refresh, *args, **kwargs)


def tera_100hr(refresh=False, *args, **kwargs):
    return tera_logMelBase_T_F_M_AdamW_b32_200k_100hr(refresh, *args, **kwargs)


def tera_960hr(refresh=False, *args, **kwargs):
    return tera_logMelBase_T_F_M_AdamW_b32_1m_960hr_drop1(refresh, *args, **kwargs)


def tera_logMelBase_T_F_AdamW_b32_200k_100hr(refresh=False, *args, **kwargs):
    kwargs["ckpt"] = "https://www.dropbox.com/s/o36qt1zgtn3tsep/states-200000.ckpt?dl=1"
    return tera_url(refresh=refresh, *args, **kwargs)


def tera_logMelBase_T_F_M_AdamW_b32_200k_100hr(refresh=False, *args, **kwargs):
    kwargs["ckpt"] = "https://www.dropbox.com/s/l9ryl82k64m1lsk/states-200000.ckpt?dl=1"
    return tera_url(refresh=refresh, *args, **kwargs)


def tera_logMelBase_T_F_AdamW_b32_1m_960hr(refresh=False, *args, **kwargs):
    kwargs["ckpt"] = "https://www.dropbox.com/s/98olxex0m7oy9ta/states-1000000.ckpt?dl=1"
    return tera_url(refresh=refresh, *args, **kwargs)


def tera_logMelBase_T_F_AdamW_b32_1m_960hr_drop1(refresh=False, *args, **kwargs):
    kwargs["ckpt"] = "https://www.dropbox.com/s/2ekbt2gxlkbvfz0/states-1000000.ckpt?dl=1"
    return tera_url(refresh=refresh, *args, **kwargs)


def tera_logMelBase_T_F_AdamW_b32_1m_960hr_seq3k(refresh=False, *args, **kwargs):
    kwargs["ckpt"] = "https://www.dropbox.com/s/tfysinbalpm3gsj/states-1000000.ckpt?dl=1"
    return tera_url(refresh=refresh, *args, **kwargs)


def tera_logMelBase_T_F_M_AdamW_b32_1m_960hr_drop1(refresh=False, *args, **kwargs):
    kwargs["ckpt"] = ("https://huggingface.co/s3prl/tera/resolve/main/tera_logMelBase_T_F_M_AdamW_b32_1m_960hr_drop1/"
                      "states-1000000.ckpt")
    return tera_url(refresh=refresh, *args, **kwargs)


def tera_fbankBase_T_F_AdamW_b32_200k_100hr(refresh=False, *args, **kwargs):
    kwargs["ckpt"] = "https://www.dropbox.com/s/i32ob29m6afufot/states-200000.ckpt?dl=1"
    return tera_url(refresh=refresh, *args, **kwargs)
