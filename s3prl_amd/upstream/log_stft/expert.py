"""``UpstreamExpert`` of the ``stft_mag`` upstream on the MI355X.

Mirrors ``s3prl/upstream/log_stft/expert.py``: ``UpstreamExpert(model_config, **kwargs)`` with ``model_config`` a yaml file in
the reference's schema (``spectrogram: {n_fft, hop_length, win_length, window, center, log}``; ``stft_mag.yaml`` and
``log_stft_mag.yaml`` are 512 / 320 / 512, hann, centred, log off / on) or the parsed dict.  Per utterance
``|torch.stft(...)|`` (the magnitude, not the power), with ``log`` its ``log(clamp(., 1e-8))``, ``(B, T, n_fft / 2 + 1)`` with
``T = 1 + n // hop_length`` zero-padded; ``last_hidden_state`` is the LIST ``[feats]``, as the reference returns it.  The
arithmetic runs in ``libs3enc.so`` (``s3prl_amd/csrc/spectral_ops.hip``); there is no CPU fallback.
"""

from __future__ import annotations

from typing import List

import torch
import yaml

from ... import _lib
from ..baseline.expert import SAMPLE_RATE, spectral_forward


class UpstreamExpert(torch.nn.Module):
    def __init__(self, model_config=None, **kwargs):
        super().__init__()
        if isinstance(model_config, dict):
            self.config = model_config
        else:
            with open(model_config, "r") as f:
                self.config = yaml.load(f, Loader=yaml.FullLoader)
        if self.config.get("feat_type", "spectrogram") != "spectrogram":
            raise NotImplementedError(f"feat_type {self.config['feat_type']!r} is not implemented (spectrogram)")
        if int(self.config.get("sample_rate", SAMPLE_RATE)) != SAMPLE_RATE:
            raise NotImplementedError(f"sample_rate {self.config['sample_rate']} is not implemented (16000)")
        s = dict(self.config["spectrogram"])
        if s.get("window", "hann") != "hann":
            raise NotImplementedError(f"window {s['window']!r} is not implemented (hann)")
        if not s.get("center", True):
            raise NotImplementedError("center=False is not implemented")
        c = _lib.S3SpectralConfig()
        c.kind, c.sample_rate = _lib.SPECTRAL_KINDS["stft_mag"], SAMPLE_RATE
        c.n_fft, c.hop, c.win = int(s["n_fft"]), int(s["hop_length"]), int(s["win_length"])
        c.log = int(bool(s.get("log", False)))
        if c.n_fft % 4 or c.hop % 4 or not 0 < c.win <= c.n_fft:
            raise NotImplementedError(f"n_fft={c.n_fft}, hop_length={c.hop}, win_length={c.win}: n_fft and hop_length must be "
                                      "multiples of 4 and win_length at most n_fft")
        self._c = c
        self.output_dim = c.n_fft // 2 + 1
        self.downsample_rate = c.hop
        self._lib = _lib.load()
        self.register_buffer("_device_probe", torch.zeros(1), persistent=False)

    def get_downsample_rates(self, key: str = None) -> int:
        return self.downsample_rate

    def forward(self, wavs: List[torch.Tensor]):
        if len(wavs) == 0:
            raise ValueError("empty batch")
        feats = spectral_forward(self._lib, self._c, wavs, self.output_dim)
        return {"last_hidden_state": [feats], "hidden_states": [feats]}
