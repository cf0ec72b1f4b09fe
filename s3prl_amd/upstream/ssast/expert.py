"""MI355X-native stand-in for ``s3prl/upstream/ssast/expert.py::UpstreamExpert`` (same constructor / forward /
get_downsample_rates contract; the forward runs in libs3enc's HIP kernels, csrc/ssast.hip, csrc/fbank.hip and csrc/patchstrided.hip).

``UpstreamExpert(ckpt, model_size, window_secs=1.0)``: ``ckpt`` is an SSAST pretraining file — a plain state dict with ``module.v.*``
keys and the two ``module.p_input_*`` scalars — or the dict itself; ``model_size`` is the reference's "<tiny|small|base>_<p|f>".
``forward(wavs)`` returns the ``depth`` block outputs as ``(B, T_out, f_dim * D)`` tensors: every utterance is cut into
``window_secs`` windows, each window is its own sequence behind a cls and a dist token, and row ``s * t_dim + ti`` holds the ``f_dim``
tokens of time step ``ti`` of window ``s``; the list is cut to ``len(range(0, max_len, 160 * tstride))`` rows.  Nothing is masked: the
rows behind an utterance's own length are the reference's values — zero samples through the whole model — and not zeros."""

from ...ckpt import load_ssast_checkpoint
from ..base import HipUpstreamExpert

FBANK_SAMPLE_STRIDE = 160


class UpstreamExpert(HipUpstreamExpert):
    family = "ssast"

    def __init__(self, ckpt: str, model_size: str, window_secs: float = 1.0, dtype: str = None, **kwargs):
        import os

        import torch

        torch.nn.Module.__init__(self)
        if ckpt is None:
            raise ValueError("an SSAST checkpoint is required: the pretraining file's state dict (module.v.*), or that dict")
        self.window_secs = window_secs
        self.stride_secs = window_secs
        self.cfg, self._weights = load_ssast_checkpoint(ckpt, model_size, window_secs)
        self.tstride = self.cfg.ss_tstride
        self.vertical_num_patches = self.cfg.ss_f_dim
        self.dtype = dtype or os.environ.get("S3PRL_AMD_DTYPE", "fp32")
        self._encoders = {}
        self.register_buffer("_device_probe", torch.zeros(1), persistent=False)
        self.eval()

    @property
    def hidden_sizes(self):
        return [self.cfg.ss_f_dim * self.cfg.encoder_embed_dim] * self.num_layers

    def get_downsample_rates(self, key: str = None) -> int:
        return int(FBANK_SAMPLE_STRIDE * self.tstride)  # ssast/expert.py:82-83

    def _states_info(self, n: int):
        return tuple(f"state_{i}" for i in range(n))  # the reference's forward returns the list itself: no hooks
