"""MI355X-native stand-in for ``s3prl/upstream/apc/expert.py::UpstreamExpert`` (APC and VQ-APC: same constructor / forward /
get_downsample_rates contract; the forward runs in libs3enc's HIP kernels, csrc/apc.hip, csrc/fbank.hip and csrc/rnn.hip).

``forward(wavs)`` returns what ``UpstreamBase.__call__`` builds from the reference's three hooks (apc/expert.py:29-42):
``hidden_states`` = (the input of ``rnn_layers[1]``, the input of ``rnn_layers[2]``, the last layer's output after its residual) —
three states even for a four-layer model —, ``last_hidden_state``, ``hidden_state_{i}`` and ``_hidden_states_info``.  The
reference's forward returns nothing itself, so there is no ``default`` key.  The GRU layers run on packed sequences: every row
behind an utterance's own frame count is exactly 0.  VQ-APC's quantizer and the post-net feed only the prediction that the
upstream discards, so the same expert serves both."""

from ..base import HipUpstreamExpert


class UpstreamExpert(HipUpstreamExpert):
    family = "apc"

    def get_downsample_rates(self, key: str = None) -> int:
        return 160  # apc/expert.py:44-45

    def _states_info(self, n: int):
        return ("self.model.rnn_layers[1]", "self.model.rnn_layers[2]", "self.model")
