"""MI355X-native stand-in for ``s3prl/upstream/wav2vec/expert.py::UpstreamExpert`` (wav2vec and vq-wav2vec: same constructor /
forward / get_downsample_rates contract; the forward runs in libs3enc's HIP kernels, csrc/wav2vec.hip).

``forward(wavs)`` returns the reference's keys (wav2vec/expert.py:39-62): ``z`` (the extractor output, (B, T, C)), ``c`` and
``default`` (the aggregator output), with a quantizer also ``codewords`` (B, T, vq_dim) and ``codeids`` (B, T, groups) int64,
plus what ``UpstreamBase.__call__`` adds from the hooks: ``hidden_states`` = z, the input of aggregator layers 1.., the aggregator
output; ``last_hidden_state``; ``hidden_state_{i}``.  The waveforms are zero-padded, never normalised, and there is no frame mask:
the GroupNorm statistics run over the padded time, so the states depend on the batch's longest utterance (``n_max``)."""

from ..base import HipUpstreamExpert


class UpstreamExpert(HipUpstreamExpert):
    family = "wav2vec"

    def get_downsample_rates(self, key: str = None) -> int:
        return self.cfg.downsample_rate  # 160 for every released model (wav2vec/expert.py:36-37)

    def _states_info(self, n: int):
        agg = "self.model.feature_aggregator"
        return ("self.model.feature_extractor",) + tuple(f"{agg}.conv_layers[{i + 1}]" for i in range(n - 2)) + (agg,)

    def forward(self, wavs):
        self._check_inference(wavs)
        enc = self._encoder_for(self._compute_device(wavs))
        aux = {} if self.cfg.vq_type != "none" else None
        hs = self._guard_backward(enc.forward(wavs, aux=aux))
        result = self._result(hs, wavs[0].device)
        result["z"] = result["hidden_states"][0]
        result["c"] = result["default"] = result["hidden_states"][-1]
        if aux is not None:
            result["codewords"] = aux["codewords"].to(wavs[0].device)
            result["codeids"] = aux["codeids"].to(wavs[0].device)
        return result
