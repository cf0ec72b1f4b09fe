"""MI355X-native stand-in for ``s3prl/upstream/lighthubert/expert.py::UpstreamExpert``.

The checkpoint is ``{"cfg": {"model": {...}}, "model": state_dict}``: a 768-wide HuBERT-base supernet.  ``cfg.model._name`` picks the
subnet — ``hubert_pruner``: the released 640-wide (``base.yaml``) or 384-wide (``small.yaml``) one, ``student_hubert``: the largest of
its search space — and ``s3prl_amd.ckpt.lighthubert_slice`` cuts every tensor to it at load, so only the subnet reaches the device.
Every waveform is normalised (``F.layer_norm(wav, wav.shape)``, whatever the config says).  The result is ``{"hidden_states": hs}``
only, as the reference returns it (no ``last_hidden_state``; ``UpstreamBase.__call__`` is not involved): 13 states, element 0 the
``post_extract_proj`` output with its padded frames exactly zero, then the outputs of the 12 layers.  Exact fp32 only."""

from ..base import HipUpstreamExpert


class UpstreamExpert(HipUpstreamExpert):
    family = "lighthubert"

    def __init__(self, ckpt: str = None, feature_selection: str = None, **kwds):
        if feature_selection is not None:  # the reference's expert has no such argument and returns one list
            raise ValueError(f"feature_selection={feature_selection!r} is not defined for LightHuBERT: its expert returns one "
                             "hidden_states list (the projection output and the 12 layer outputs)")
        import os

        dtype = kwds.get("dtype") or os.environ.get("S3PRL_AMD_DTYPE", "fp32")
        if dtype not in ("fp32", "f32", "float32"):
            raise ValueError(f"LightHuBERT is built for compute dtype fp32 only; {dtype} is not built")
        super().__init__(ckpt, **kwds)

    def get_downsample_rates(self, key: str = None) -> int:
        return 320

    def forward(self, wavs):
        return self._result(self.encode(wavs), wavs[0].device, full=False)
