"""MI355X-native stand-in for ``s3prl/upstream/vggish/expert.py::UpstreamExpert`` (same constructor / forward /
get_downsample_rates contract; the forward runs in libs3enc's HIP kernels, csrc/vggish.hip and csrc/conv2d.hip).

``UpstreamExpert(ckpt, pretrained=True, postprocess=True, progress=True, **kwargs)``: ``ckpt`` is the DICT the reference's hubconf
builds, ``{"vggish": state_dict, "pca": {"pca_eigen_vectors", "pca_means"}}`` (a path to a file holding that dict is accepted
too).  ``pretrained=False`` is the reference's randomly initialised model, which nobody can reproduce: refused.  ``progress`` only
concerns a download bar.

``forward(wavs)`` returns one state of ``(B, E_max, 128)``: per utterance its ``E = 1 + (F - 96) // 96`` examples of 96 un-padded
10 ms frames (``F = 1 + (n - 400) // 160``), then exact zero rows (``pad_sequence``).  With ``postprocess`` the values are the
PCA-transformed, clamped, 8-bit-quantised embeddings as whole numbers 0..255 in fp32.  An utterance shorter than 15600 samples holds
no example and is refused by index and length (the reference raises on it)."""

from ...ckpt import load_vggish_checkpoint
from ..base import HipUpstreamExpert


class UpstreamExpert(HipUpstreamExpert):
    family = "vggish"

    def __init__(self, ckpt=None, pretrained: bool = True, postprocess: bool = True, progress: bool = True, dtype: str = None,
                 **kwargs):
        import os

        import torch

        torch.nn.Module.__init__(self)
        if ckpt is None:
            raise ValueError("a VGGish checkpoint is required: the dict {'vggish': state_dict, 'pca': {...}} or a file holding it")
        if not pretrained:
            raise ValueError("pretrained=False (the reference's randomly initialised VGGish) is not built: there are no weights to run")
        self.cfg, self._weights = load_vggish_checkpoint(ckpt, postprocess=bool(postprocess))
        self.dtype = dtype or os.environ.get("S3PRL_AMD_DTYPE", "fp32")
        self._encoders = {}
        self.register_buffer("_device_probe", torch.zeros(1), persistent=False)
        self.eval()

    def get_downsample_rates(self, key: str = None) -> int:
        return 16000  # vggish/expert.py:21-22

    def _states_info(self, n: int):
        return tuple(f"state_{i}" for i in range(n))  # the reference's forward returns the list itself: no hooks
