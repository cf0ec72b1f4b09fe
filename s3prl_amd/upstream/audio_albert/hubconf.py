"""hub entries of AudioALBERT under the reference's names and signatures (s3prl/upstream/audio_albert/hubconf.py):
``audio_albert_local(ckpt, *args, **kwargs)``, ``audio_albert_url(ckpt, refresh=False, *args, **kwargs)`` and the released names."""

import os

from ...download import urls_to_filepaths as _urls_to_filepaths
from .expert import UpstreamExpert as _UpstreamExpert


def audio_albert_local(ckpt, *args, **kwargs):
    assert os.path.isfile(ckpt), ckpt
    return _UpstreamExpert(str(ckpt), *args, **kwargs)


def audio_albert_url(ckpt, refresh=False, *args, **kwargs):
    return audio_albert_local(_urls_to_filepaths(str(ckpt), refresh=refresh), *args, **kwargs)


def audio_albert(refresh=False, *args, **kwargs):
    return audio_albert_960hr(refresh=refresh, *args, **kwargs)


def audio_albert_960hr(refresh=False, *args, **kwargs):
    return audio_albert_logMelBase_T_share_AdamW_b32_1m_960hr_drop1(refresh=refresh, *args, **kwargs)


def audio_albert_logMelBase_T_share_AdamW_b32_1m_960hr_drop1(refresh=False, *args, **kwargs):
    kwargs["ckpt"] = ("https://huggingface.co/s3prl/audio_albert/resolve/main/"
                      "audio_albert_logMelBase_T_share_AdamW_b32_1m_960hr_drop1/states-1000000.ckpt")
    return audio_albert_url(refresh=refresh, *args, **kwargs)
