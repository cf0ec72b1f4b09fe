"""hub entries of wav2vec under the reference's names and signatures (s3prl/upstream/wav2vec/hubconf.py:18-64):
``wav2vec_custom(ckpt, *args, legacy=False, refresh=False, **kwargs)``, ``wav2vec_local`` / ``wav2vec_url``, ``wav2vec`` and
``wav2vec_large``.  ``http`` checkpoints resolve to the reference's cache file (``s3prl_amd.download``); ``legacy=True`` names the
ORIGINAL fairseq file, which is read here without the ``fairseq`` package (its layout is converted first)."""

import os

from ...ckpt import convert_fairseq_checkpoint as _convert_fairseq_checkpoint
from ...download import urls_to_filepaths as _urls_to_filepaths
from .. import _released
from .expert import UpstreamExpert as _UpstreamExpert


def wav2vec_custom(ckpt: str, *args, legacy: bool = False, refresh: bool = False, **kwargs):
    if str(ckpt).startswith("http"):
        ckpt = _urls_to_filepaths(str(ckpt), refresh=refresh)
    if legacy:
        ckpt = _convert_fairseq_checkpoint(str(ckpt), "wav2vec", refresh=refresh)
    assert os.path.isfile(ckpt), ckpt
    return _UpstreamExpert(str(ckpt), *args, **kwargs)


def wav2vec_local(*args, **kwargs):
    return wav2vec_custom(*args, **kwargs)


def wav2vec_url(*args, **kwargs):
    return wav2vec_custom(*args, **kwargs)


wav2vec = _released.alias("wav2vec", lambda: wav2vec_large, "The default model - Large model (wav2vec/hubconf.py:46-51)")
wav2vec_large = _released.with_legacy("wav2vec_large", wav2vec_custom,
                                      "https://huggingface.co/s3prl/converted_ckpts/resolve/main/wav2vec_large.pt",
                                      "https://dl.fbaipublicfiles.com/fairseq/wav2vec/wav2vec_large.pt")
