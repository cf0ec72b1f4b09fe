"""hub entries of MAE-AST under the reference's names and signatures (s3prl/upstream/mae_ast/hubconf.py:17-53):
``mae_ast_local(ckpt, *args, **kwargs)``, ``mae_ast_url(ckpt, refresh=False, *args, **kwargs)``, ``mae_ast_frame`` and
``mae_ast_patch(refresh=False, *args, **kwargs)``.  A URL resolves to the reference's cache file (``s3prl_amd.download``)."""

import os

from ...download import urls_to_filepaths as _urls_to_filepaths
from .expert import UpstreamExpert as _UpstreamExpert


def mae_ast_local(ckpt, *args, **kwargs):
    assert os.path.isfile(ckpt), ckpt
    return _UpstreamExpert(str(ckpt), *args, **kwargs)


def mae_ast_url(ckpt, refresh=False, *args, **kwargs):
    return mae_ast_local(_urls_to_filepaths(str(ckpt), refresh=refresh), *args, **kwargs)


def mae_ast_frame(refresh=False, *args, **kwargs):
    kwargs["ckpt"] = "https://www.cs.utexas.edu/~harwath/model_checkpoints/mae_ast/random_frame_75_12LayerEncoder.pt"
    return mae_ast_url(refresh=refresh, *args, **kwargs)


def mae_ast_patch(refresh=False, *args, **kwargs):
    kwargs["ckpt"] = "https://www.cs.utexas.edu/~harwath/model_checkpoints/mae_ast/chunk_patch_75_12LayerEncoder.pt"
    return mae_ast_url(refresh=refresh, *args, **kwargs)
