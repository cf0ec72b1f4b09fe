"""MI355X-native stand-in for ``s3prl/upstream/decoar/expert.py::UpstreamExpert`` (same constructor / forward /
get_downsample_rates contract; the forward runs in libs3enc's HIP kernels, csrc/decoar.hip, csrc/fbank.hip and csrc/rnnb.hip).

The reference's expert is a plain ``nn.Module`` (no ``UpstreamBase`` hooks), so ``forward(wavs)`` returns exactly its dict
(decoar/expert.py:70-74): ``hidden_states`` = a list with one (B, T, 2048) state — the forward and the backward LSTM stack's last
layers side by side — and ``last_hidden_state``.  The stacks run on packed sequences: every row behind an utterance's own frame
count is exactly 0.  ``get_downsample_rates`` is the reference's 160: a frame is one 10 ms fbank shift."""

from ..base import HipUpstreamExpert


class UpstreamExpert(HipUpstreamExpert):
    family = "decoar"

    def get_downsample_rates(self, key: str = None) -> int:
        return 160  # decoar/expert.py:42-43

    def forward(self, wavs):
        result = self._result(self.encode(wavs), wavs[0].device, full=False)
        result["last_hidden_state"] = result["hidden_states"][-1]
        return result
