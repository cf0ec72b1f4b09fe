"""MI355X-native stand-in for ``s3prl/upstream/byol_s/expert.py::UpstreamExpert`` (same constructor / forward /
get_downsample_rates contract; the forward runs in libs3enc's HIP kernels, csrc/byol_s.hip, csrc/melspec.hip, csrc/stem.hip and
csrc/conv2d.hip).

``UpstreamExpert(ckpt, model_name, window_secs=1, hop_secs=0.05, model_config=None)``: ``ckpt`` is a BYOL-S weight file (a plain
state dict, as the reference's ``load_state_dict(torch.load(path))`` reads it) or the dict itself; ``model_name`` is "default"
(AudioNTT2020 at d = 2048) or "resnetish34"; "cvt" and "clstm" are refused by name.  ``model_config`` is accepted and not read, as in
the reference (its front-end values — 16 kHz, n_fft 1024, win_length 400, hop 160, 64 mels between 60 and 7800 Hz — are the ones
built).

``forward(wavs)`` returns one state of ``(B, S, 2048)``, ``S = max_len // step + 1``: the batch is zero-padded, cut into windows
centred every ``step = int(hop_secs * 1000 / 1000.0 * 16000)`` samples, and row ``(b, k)`` is the network's output for window ``k`` of
utterance ``b``.  Every window is normalised with the mean and std of ALL windows of the batch (both divided by the number of
windows, the reference's arithmetic), so a row depends on the whole batch, zero padding included, and rows past an utterance's own
length are the reference's values, not zeros.  The served semantics are eval mode: BatchNorm on its running statistics."""

from ...ckpt import load_byol_s_checkpoint
from ..base import HipUpstreamExpert

SAMPLE_RATE = 16000


class UpstreamExpert(HipUpstreamExpert):
    family = "byol_s"

    def __init__(self, ckpt: str = None, model_name: str = None, window_secs: float = 1, hop_secs: float = 0.05,
                 model_config: str = None, dtype: str = None, **kwargs):
        import os

        import torch

        torch.nn.Module.__init__(self)
        if ckpt is None:
            raise ValueError("a BYOL-S checkpoint is required: a weight file of the default or the resnetish34 network, or its state dict")
        self.frame_duration, self.hop_size = window_secs * 1000, hop_secs * 1000  # byol_s/expert.py:22-23
        self.model_config = model_config
        self.cfg, self._weights = load_byol_s_checkpoint(ckpt, model_name=model_name, window_secs=window_secs, hop_secs=hop_secs)
        self.output_dim = self.cfg.encoder_embed_dim
        self.dtype = dtype or os.environ.get("S3PRL_AMD_DTYPE", "fp32")
        self._encoders = {}
        self.register_buffer("_device_probe", torch.zeros(1), persistent=False)
        self.eval()

    def get_downsample_rates(self, key: str = None) -> int:
        return int(self.hop_size / 1000 * SAMPLE_RATE)  # byol_s/expert.py:27-28

    def _states_info(self, n: int):
        return tuple(f"state_{i}" for i in range(n))  # the reference's forward returns the list itself: no hooks
