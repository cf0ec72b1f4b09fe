"""MI355X-native stand-in for ``s3prl/upstream/decoar_layers/expert.py::UpstreamExpert``: DeCoAR with one state per LSTM layer
(decoar_layers/decoar.py:67-97) — four (B, T, 2048) states from the SAME checkpoint file and tensor names as ``decoar`` (the
reference's expert only renames them to its per-layer modules, expert.py:35-47).  ``last_hidden_state`` is the last layer, i.e.
``decoar``'s single state."""

from ...config import decoar_config
from ..decoar.expert import UpstreamExpert as _Decoar


class UpstreamExpert(_Decoar):
    def __init__(self, ckpt: str = None, model_config: str = None, dtype: str = None, **kwargs):
        super().__init__(ckpt, model_config, dtype, **kwargs)
        self.cfg = self.per_layer(self.cfg)

    @staticmethod
    def per_layer(c):
        return decoar_config(c.decoar_hidden, c.decoar_layers, True, c.decoar_feat_dim, c.decoar_subsample, c.decoar_frame_length,
                             c.decoar_frame_shift)
