"""MI355X-native stand-in for ``s3prl/upstream/cpc/expert.py::UpstreamExpert`` (modified CPC: same constructor / forward /
get_downsample_rates contract; the forward runs in libs3enc's HIP kernels, csrc/cpc.hip and csrc/rnn.hip).

``forward(wavs)`` returns what ``UpstreamBase.__call__`` builds from the reference's two hooks (cpc/expert.py:38-42):
``hidden_states`` = (the convolutional encoder's output as (B, T, C), the recurrent network's output (B, T, hiddenGar)),
``last_hidden_state``, ``hidden_state_{i}`` and ``_hidden_states_info``.  The reference's forward returns nothing itself, so there
is no ``default`` key.  The waveforms are zero-padded, never normalised, and there is no frame mask: the recurrence runs over the
padded time axis, so the frames behind an utterance's end are computed and returned like any others."""

from ..base import HipUpstreamExpert


class UpstreamExpert(HipUpstreamExpert):
    family = "cpc"

    def get_downsample_rates(self, key: str = None) -> int:
        return 160  # cpc/expert.py:44-45

    def _states_info(self, n: int):
        return ("self.model.gEncoder", "self.model.gAR")
