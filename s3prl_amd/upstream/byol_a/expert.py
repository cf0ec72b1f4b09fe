"""MI355X-native stand-in for ``s3prl/upstream/byol_a/expert.py::UpstreamExpert`` (same constructor / forward /
get_downsample_rates contract; the forward runs in libs3enc's HIP kernels, csrc/byol_a.hip, csrc/melspec.hip and csrc/conv2d.hip).

``UpstreamExpert(ckpt, model_config, feature_d, window_secs=1.0, stride_secs=1.0)``: ``ckpt`` is an ``AudioNTT2020`` weight file (a
plain state dict or one under ``"state_dict"``, keys cut at their ``fc.`` / ``features.`` component as the reference does) or the
dict itself.  ``model_config`` is the reference's ``config.yaml``, whose front-end values (16 kHz, n_fft = win_length = 1024, hop
160, 64 mels between 60 and 7800 Hz) are the only ones built: the argument is accepted and not read.  ``feature_d`` is checked
against ``fc.0.weight``.

``forward(wavs)`` returns one state of ``(B, S, feature_d)``, ``S = len(range(0, max_len, int(stride_secs * 16000)))``: every
utterance is zero-padded to ``starts[-1] + int(window_secs * 16000)`` and cut into segments, and row ``(b, s)`` is the network's
output for segment ``s`` of utterance ``b``.  Rows past an utterance's own length are NOT zeros: they are the network's response to
the padded segments, exactly as in the reference."""

from ...ckpt import load_byol_a_checkpoint
from ..base import HipUpstreamExpert

SAMPLE_RATE = 16000


class UpstreamExpert(HipUpstreamExpert):
    family = "byol_a"

    def __init__(self, ckpt, model_config=None, feature_d: int = None, window_secs: float = 1.0, stride_secs: float = 1.0,
                 dtype: str = None, **kwargs):
        import os

        import torch

        torch.nn.Module.__init__(self)
        if ckpt is None:
            raise ValueError("a BYOL-A checkpoint is required: an AudioNTT2020 weight file or its state dict")
        self.window_secs, self.stride_secs = window_secs, stride_secs
        self.cfg, self._weights = load_byol_a_checkpoint(ckpt, feature_d=feature_d, window_secs=window_secs, stride_secs=stride_secs)
        self.output_dim = self.cfg.encoder_embed_dim
        self.dtype = dtype or os.environ.get("S3PRL_AMD_DTYPE", "fp32")
        self._encoders = {}
        self.register_buffer("_device_probe", torch.zeros(1), persistent=False)
        self.eval()

    def get_downsample_rates(self, key: str = None) -> int:
        return int(self.stride_secs * SAMPLE_RATE)  # byol_a/expert.py:64-65

    def _states_info(self, n: int):
        return tuple(f"state_{i}" for i in range(n))  # the reference's forward returns the list itself: no hooks
