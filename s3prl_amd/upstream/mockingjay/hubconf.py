"""hub entries of Mockingjay under the reference's names and signatures (s3prl/upstream/mockingjay/hubconf.py): ``mockingjay_local(ckpt,
options_config=None, *args, **kwargs)``, ``mockingjay_url(ckpt, refresh=False, *args, **kwargs)`` and the released names.  A URL
resolves to the reference's cache file (``s3prl_amd.download``)."""

import os

from ...download import urls_to_filepaths as _urls_to_filepaths
from .expert import UpstreamExpert as _UpstreamExpert


def mockingjay_local(ckpt, options_config=None, *args, **kwargs):
    assert os.path.isfile(ckpt), ckpt
    if options_config is not None:
        assert os.path.isfile(options_config), options_config
    return _UpstreamExpert(str(ckpt), options_config, *args, **kwargs)


def mockingjay_url(ckpt, refresh=False, *args, **kwargs):
    return mockingjay_local(_urls_to_filepaths(str(ckpt), refresh=refresh), *args, **kwargs)


def mockingjay(refresh=False, *args, **kwargs):
    return mockingjay_origin(refresh=refresh, *args, **kwargs)


def mockingjay_origin(refresh=False, *args, **kwargs):
    return mockingjay_logMelLinearLarge_T_AdamW_b32_500k_360hr_drop1(refresh=refresh, *args, **kwargs)


def mockingjay_100hr(refresh=False, *args, **kwargs):
    return mockingjay_logMelBase_T_AdamW_b32_200k_100hr(refresh=refresh, *args, **kwargs)


def mockingjay_960hr(refresh=False, *args, **kwargs):
    return mockingjay_logMelBase_T_AdamW_b32_1m_960hr_drop1(refresh=refresh, *args, **kwargs)


def mockingjay_logMelBase_T_AdamW_b32_200k_100hr(refresh=False, *args, **kwargs):
    kwargs["ckpt"] = "https://www.dropbox.com/s/luorglf8mdg67l2/states-200000.ckpt?dl=1"
    return mockingjay_url(refresh=refresh, *args, **kwargs)


def mockingjay_logMelLinearLarge_T_AdamW_b32_500k_360hr_drop1(refresh=False, *args, **kwargs):
    kwargs["ckpt"] = ("https://huggingface.co/s3prl/mockingjay/resolve/main/"
                      "mockingjay_logMelLinearLarge_T_AdamW_b32_500k_360hr_drop1/states-500000.ckpt")
    return mockingjay_url(refresh=refresh, *args, **kwargs)


def mockingjay_logMelBase_T_AdamW_b32_1m_960hr(refresh=False, *args, **kwargs):
    kwargs["ckpt"] = "https://www.dropbox.com/s/jzx0xggk663jev6/states-1000000.ckpt?dl=1"
    return mockingjay_url(refresh=refresh, *args, **kwargs)


def mockingjay_logMelBase_T_AdamW_b32_1m_960hr_drop1(refresh=False, *args, **kwargs):
    kwargs["ckpt"] = "https://www.dropbox.com/s/7f9z6dzc7oix6qv/states-1000000.ckpt?dl=1"
    return mockingjay_url(refresh=refresh, *args, **kwargs)


def mockingjay_logMelBase_T_AdamW_b32_1m_960hr_seq3k(refresh=False, *args, **kwargs):
    kwargs["ckpt"] = "https://www.dropbox.com/s/qnnvdrai2tfmjmh/states-1000000.ckpt?dl=1"
    return mockingjay_url(refresh=refresh, *args, **kwargs)
