"""MI355X-native stand-in for ``s3prl/upstream/mae_ast/expert.py::UpstreamExpert`` (same constructor / forward /
get_downsample_rates contract; the forward runs in libs3enc's HIP kernels, csrc/mae_ast.hip, csrc/fbank.hip and csrc/patchembed.hip).

``UpstreamExpert(ckpt)``: ``ckpt`` is an MAE-AST checkpoint file — ``{"cfg": {"model", "task"}, "model": state_dict}`` — or the dict
itself.  ``forward(wavs)`` returns the ``encoder_layers`` layer outputs as ``(B, F_max // kt, V * D)`` tensors, ``V = 128 // kc``
tokens per time step (the embedding is not among them).  Rows at or behind an utterance's valid count are NOT zeros: they are the
reference's values — zero log-mel rows through the BatchNorm and the Linear, no position row, attention over the utterance's live
keys.  The reference's cut to ``len(range(0, max_len, kt * 160))`` rows never binds for utterances of at least 400 samples, and
shorter ones are refused."""

from ...ckpt import load_mae_ast_checkpoint
from ..base import HipUpstreamExpert

FBANK_SAMPLE_STRIDE = 160


class UpstreamExpert(HipUpstreamExpert):
    family = "mae_ast"

    def __init__(self, ckpt, model_config=None, dtype: str = None, **kwargs):
        import os

        import torch

        torch.nn.Module.__init__(self)
        if ckpt is None:
            raise ValueError("an MAE-AST checkpoint is required: a file with 'cfg' and 'model', or that dict")
        self.cfg, self._weights = load_mae_ast_checkpoint(ckpt)
        self.dtype = dtype or os.environ.get("S3PRL_AMD_DTYPE", "fp32")
        self._encoders = {}
        self.register_buffer("_device_probe", torch.zeros(1), persistent=False)
        self.eval()

    @property
    def hidden_sizes(self):
        return [self.cfg.ma_tokens_per_step * self.cfg.encoder_embed_dim] * self.num_layers

    def get_downsample_rates(self, key: str = None) -> int:
        return int(self.cfg.ma_kt * FBANK_SAMPLE_STRIDE)  # mae_ast/expert.py:57-58

    def _states_info(self, n: int):
        return tuple(f"state_{i}" for i in range(n))  # the reference's forward returns the list itself: no hooks
