"""MI355X-native stand-in for ``s3prl/upstream/decoar2/expert.py::UpstreamExpert`` (same constructor / forward /
get_downsample_rates contract; the forward runs in libs3enc's HIP kernels: csrc/fbank.hip's batch-wide pass, then HuBERT's encoder).

The checkpoint is ``{"model": state_dict}`` with no configuration: the reference's ``Decoar2()`` hard-codes its widths, here they are
read off the tensors (``s3prl_amd.ckpt.load_decoar2_checkpoint``).  The reference's expert is an ``UpstreamBase`` with one hook per
Transformer layer (its input) and one on the encoder (its output), cut to the shortest by ``postprocess`` — the padding of T to a
multiple of 2 never shows — so ``forward(wavs)`` returns the complete dict ``UpstreamBase.__call__`` builds: 13 states of
(B, ceil(F / 2), 768) for the released shape.  ``get_downsample_rates`` is the reference's 320: every second 10 ms fbank frame.
The layerdrop is 0 in the reference's expert (decoar2/expert.py:28) and a training-time option beyond it: ``set_layer_drop`` takes 0
or None and refuses the rest."""

from ..base import HipUpstreamExpert


class UpstreamExpert(HipUpstreamExpert):
    family = "decoar2"

    def __init__(self, ckpt: str = None, feature_selection: str = None, **kwds):
        if feature_selection is not None:  # the reference's expert has no such argument and returns one list
            raise ValueError(f"feature_selection={feature_selection!r} is not defined for DeCoAR 2.0: its expert returns one "
                             "hidden_states list (the 12 layer inputs and the encoder output)")
        super().__init__(ckpt, **kwds)

    @property
    def layer_drop(self) -> float:
        return 0.0

    def set_layer_drop(self, layerdrop: float = None):
        if layerdrop is None or (isinstance(layerdrop, float) and layerdrop == 0.0):
            return
        if not isinstance(layerdrop, float):
            raise ValueError("layerdrop can only be float or None")  # decoar2/expert.py:57-63
        raise ValueError(f"set_layer_drop({layerdrop}): layerdrop is a training-time option and this expert is inference-only; "
                         "only 0.0 or None (the expert's own 0.0) are taken")

    def get_downsample_rates(self, key: str = None) -> int:
        return 320  # decoar2/expert.py:65-66
