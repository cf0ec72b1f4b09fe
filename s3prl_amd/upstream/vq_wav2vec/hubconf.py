"""hub entries of vq-wav2vec under the reference's names and signatures (s3prl/upstream/vq_wav2vec/hubconf.py:18-72):
``vq_wav2vec_custom(ckpt, *args, legacy=False, refresh=False, **kwargs)``, ``vq_wav2vec`` (the gumbel model),
``vq_wav2vec_gumbel`` and ``vq_wav2vec_kmeans``.  (The reference file spells its local / url aliases ``wav2vec2_local`` /
``wav2vec2_url``; those names belong to the wav2vec 2.0 family here.)  ``vq_wav2vec_kmeans_roberta`` needs the RoBERTa upstream
and is not registered."""

import os

from ...ckpt import convert_fairseq_checkpoint as _convert_fairseq_checkpoint
from ...download import urls_to_filepaths as _urls_to_filepaths
from .. import _released
from .expert import UpstreamExpert as _UpstreamExpert

_CONVERTED = "https://huggingface.co/s3prl/converted_ckpts/resolve/main/"
_FAIRSEQ = "https://dl.fbaipublicfiles.com/fairseq/wav2vec/"


def vq_wav2vec_custom(ckpt: str, *args, legacy: bool = False, refresh: bool = False, **kwargs):
    if str(ckpt).startswith("http"):
        ckpt = _urls_to_filepaths(str(ckpt), refresh=refresh)
    if legacy:
        ckpt = _convert_fairseq_checkpoint(str(ckpt), "wav2vec", refresh=refresh)
    assert os.path.isfile(ckpt), ckpt
    return _UpstreamExpert(str(ckpt), *args, **kwargs)


vq_wav2vec = _released.alias("vq_wav2vec", lambda: vq_wav2vec_gumbel,
                             "The default model - Large model with context vector (vq_wav2vec/hubconf.py:39-44)")
vq_wav2vec_gumbel = _released.with_legacy("vq_wav2vec_gumbel", vq_wav2vec_custom, _CONVERTED + "vq-wav2vec.pt",
                                          _FAIRSEQ + "vq-wav2vec.pt")
vq_wav2vec_kmeans = _released.with_legacy("vq_wav2vec_kmeans", vq_wav2vec_custom, _CONVERTED + "vq-wav2vec_kmeans.pt",
                                          _FAIRSEQ + "vq-wav2vec_kmeans.pt")
