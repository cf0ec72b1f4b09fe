"""``UpstreamExpert`` of the baseline upstreams (``fbank`` is BASELINE configs[0]) on the MI355X.

Mirrors ``s3prl/upstream/baseline/expert.py:23-79``: ``UpstreamExpert(model_config, **kwargs)``, ``forward(wavs) ->
{"last_hidden_state", "hidden_states": [feats]}`` with ``feats`` the zero-padded ``(B, T_max, D)`` batch, ``get_downsample_rates``
= 160.  A configuration with a ``kaldi`` block is ``torchaudio.compliance.kaldi``'s ``fbank`` (``fbank.yaml``,
``fbank_no_cmvn.yaml``: framing + DC removal + pre-emphasis + povey window + DFT as one implicit GEMM on the raw PCM, mel / log,
deltas, CMVN; ``s3prl_amd/csrc/fbank.hip``), ``spectrogram`` or ``mfcc`` (``spectrogram.yaml``, ``mfcc.yaml``); one without is the
``OnlinePreprocessor``'s ``linear`` or ``mel`` (``linear.yaml``, ``mel.yaml``; ``s3prl_amd/csrc/spectral_ops.hip``).  Everything
runs in ``libs3enc.so``; there is no CPU fallback, and what is not built is refused by name.
"""

from __future__ import annotations

import ctypes as C
from typing import List

import torch
import yaml

from ... import _lib

SAMPLE_RATE = 16000

# torchaudio.compliance.kaldi's defaults: a configuration may state them, any other value is refused by name
_KALDI_DEFAULTS = dict(blackman_coeff=0.42, channel=-1, dither=0.0, energy_floor=1.0, min_duration=0.0, raw_energy=True,
                       remove_dc_offset=True, round_to_power_of_two=True, snip_edges=True, subtract_mean=False, window_type="povey",
                       use_energy=False, htk_compat=False, low_freq=20.0, high_freq=0.0, vtln_high=-500.0, vtln_low=100.0,
                       vtln_warp=1.0, sample_frequency=16000.0)


def _kaldi_spectral(config: dict) -> "_lib.S3SpectralConfig":
    kind = config["kaldi"].get("feat_type", "fbank")
    if kind not in ("spectrogram", "mfcc"):
        raise NotImplementedError(f"kaldi feat_type {kind!r} is not implemented (fbank, spectrogram, mfcc)")
    opts = dict(config["kaldi"].get(kind, {}))
    c = _lib.S3SpectralConfig()
    c.kind, c.sample_rate = _lib.SPECTRAL_KINDS[kind], SAMPLE_RATE
    c.frame_length_ms = float(opts.pop("frame_length", 25.0))
    c.frame_shift_ms = float(opts.pop("frame_shift", 10.0))
    c.preemphasis = float(opts.pop("preemphasis_coefficient", 0.97))
    if kind == "mfcc":
        c.num_ceps = int(opts.pop("num_ceps", 13))
        c.num_mel_bins = int(opts.pop("num_mel_bins", 23))
        c.cepstral_lifter = float(opts.pop("cepstral_lifter", 22.0))
    defaults = dict(_KALDI_DEFAULTS, energy_floor=0.0) if kind == "mfcc" else _KALDI_DEFAULTS
    for key, value in sorted(opts.items()):
        if key not in defaults or value != defaults[key]:
            raise NotImplementedError(f"kaldi.{kind} option {key}={value!r} is not implemented")
    delta = config.get("delta", {})
    c.delta_order, c.delta_win_length = int(delta.get("order", 2)), int(delta.get("win_length", 5))
    if unknown := sorted(set(delta) - {"order", "win_length"}):
        raise NotImplementedError(f"delta options {unknown} are not implemented")
    cmvn = config.get("cmvn", {})
    c.use_cmvn, c.cmvn_eps = int(bool(cmvn.get("use_cmvn", False))), float(cmvn.get("eps", 1e-10))
    return c


def _preprocessor_spectral(config: dict) -> "_lib.S3SpectralConfig":
    if "input" not in config:
        raise NotImplementedError("a baseline configuration needs a `kaldi` block or the preprocessor's `input` block")
    if "target" in config:
        raise NotImplementedError("a preprocessor `target` block is not implemented (the expert processes `input` only)")
    if int(config.get("sample_rate", SAMPLE_RATE)) != SAMPLE_RATE:
        raise NotImplementedError(f"sample_rate {config['sample_rate']} is not implemented (16000)")
    for key, want in (("win_ms", 25), ("hop_ms", 10), ("n_freq", 201)):
        if config.get(key, want) != want:
            raise NotImplementedError(f"{key}={config[key]!r} is not implemented ({want})")
    feat = dict(config["input"])
    kind = feat.get("feat_type")
    if kind not in ("linear", "mel"):
        raise NotImplementedError(f"preprocessor feat_type {kind!r} is not implemented (linear, mel)")
    if int(feat.get("delta", 0)) > 0:
        raise NotImplementedError(f"preprocessor delta={feat['delta']} is not implemented (0)")
    if not bool(feat.get("log", False)):
        raise NotImplementedError("preprocessor log=False is not implemented")
    if int(feat.get("channel", 0)) != 0:
        raise NotImplementedError(f"preprocessor channel={feat['channel']} is not implemented (0)")
    c = _lib.S3SpectralConfig()
    c.kind, c.sample_rate, c.log = _lib.SPECTRAL_KINDS[kind], SAMPLE_RATE, 1
    c.n_fft, c.hop, c.win = 400, 160, 400
    c.num_mel_bins = int(config.get("n_mels", 40))
    c.use_cmvn, c.cmvn_eps = int(bool(feat.get("cmvn", False))), 1e-10
    return c


def spectral_config(config: dict) -> "_lib.S3SpectralConfig":
    """The ``s3enc_spectral_config`` of a baseline configuration that is not the kaldi fbank; refuses what is not built."""
    return _kaldi_spectral(config) if "kaldi" in config else _preprocessor_spectral(config)


def spectral_output_dim(c) -> int:
    if c.kind == _lib.SPECTRAL_KINDS["spectrogram"]:
        size = int(c.sample_rate * c.frame_length_ms * 0.001)
        return ((1 << (size - 1).bit_length()) // 2 + 1) * (c.delta_order + 1)
    if c.kind == _lib.SPECTRAL_KINDS["mfcc"]:
        return c.num_ceps * (c.delta_order + 1)
    return {_lib.SPECTRAL_KINDS["linear"]: 201, _lib.SPECTRAL_KINDS["mel"]: c.num_mel_bins}.get(c.kind, c.n_fft // 2 + 1)


def spectral_forward(lib, c, wavs: List[torch.Tensor], output_dim: int) -> torch.Tensor:
    """``s3enc_spectral_num_frames`` + ``s3enc_spectral_forward`` on a list of device waveforms: the zero-padded (B, T, D) batch."""
    dev = wavs[0].device
    if dev.type != "cuda":
        raise RuntimeError("s3prl_amd runs the fbank upstream on an MI355X only (no CPU fallback); move the wavs to the GPU")
    held = [w.to(device=dev, dtype=torch.float32).contiguous() for w in wavs]
    lengths = [int(w.numel()) for w in held]
    kaldi = c.kind in (_lib.SPECTRAL_KINDS["spectrogram"], _lib.SPECTRAL_KINDS["mfcc"])
    if kaldi and min(lengths) < int(c.sample_rate * c.frame_length_ms * 0.001):
        raise ValueError("an utterance is shorter than one 25 ms analysis window")
    if c.kind == _lib.SPECTRAL_KINDS["stft_mag"] and min(lengths) <= c.n_fft // 2:
        raise ValueError(f"an utterance of {c.n_fft // 2} samples or fewer cannot be reflect-padded by n_fft / 2")
    if c.kind in (_lib.SPECTRAL_KINDS["linear"], _lib.SPECTRAL_KINDS["mel"]) and min(lengths) <= 200:
        raise ValueError("an utterance of 200 samples or fewer has no reflect-padded centred frame")
    B = len(held)
    ptrs = (C.c_void_p * B)(*[w.data_ptr() for w in held])
    lens = (C.c_int64 * B)(*lengths)
    frames = (C.c_int32 * B)()
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    with torch.cuda.device(dev):
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        _lib.check(lib.s3enc_spectral_num_frames(C.byref(c), ptrs, lens, B, frames, idx, stream), "s3enc_spectral_num_frames")
        T = max(frames)
        out = torch.empty((B, T, output_dim), dtype=torch.float32, device=dev)
        _lib.check(lib.s3enc_spectral_forward(C.byref(c), ptrs, lens, B, C.c_void_p(out.data_ptr()), T, idx, stream),
                   "s3enc_spectral_forward")
    return out


class UpstreamExpert(torch.nn.Module):
    def __init__(self, model_config, **kwargs):
        """``model_config``: path of a yaml file in the reference's baseline schema (``kaldi: {feat_type, fbank: {...}}``,
        ``delta: {order, win_length}``, ``cmvn: {use_cmvn}``) or the already-parsed dict."""
        super().__init__()
        if isinstance(model_config, dict):
            self.config = model_config
        else:
            with open(model_config, "r") as f:
                self.config = yaml.load(f, Loader=yaml.FullLoader)
        self._spectral = None
        if "kaldi" not in self.config or self.config["kaldi"].get("feat_type", "fbank") != "fbank":
            self._spectral = spectral_config(self.config)
            self.output_dim = spectral_output_dim(self._spectral)
            self.downsample_rate = 160 if "kaldi" not in self.config else round(self._spectral.frame_shift_ms * SAMPLE_RATE / 1000)
            self._lib = _lib.load()
            self.register_buffer("_device_probe", torch.zeros(1), persistent=False)
            return
        fb = dict(self.config["kaldi"].get("fbank", {}))
        if not fb.pop("use_log_fbank", True):
            raise NotImplementedError("use_log_fbank=False is not implemented")
        c = _lib.S3FbankConfig()
        c.sample_rate = SAMPLE_RATE
        c.num_mel_bins = int(fb.pop("num_mel_bins", 23))
        c.frame_length_ms = float(fb.pop("frame_length", 25.0))
        c.frame_shift_ms = float(fb.pop("frame_shift", 10.0))
        c.preemphasis = float(fb.pop("preemphasis_coefficient", 0.97))
        if fb:
            raise NotImplementedError(f"unsupported kaldi.fbank options: {sorted(fb)}")
        delta = self.config.get("delta", {})
        c.delta_order = int(delta.get("order", 2))
        c.delta_win_length = int(delta.get("win_length", 5))
        cmvn = self.config.get("cmvn", {})
        c.use_cmvn = int(bool(cmvn.get("use_cmvn", False)))
        c.cmvn_eps = float(cmvn.get("eps", 1e-10))
        self._c = c
        self.output_dim = c.num_mel_bins * (c.delta_order + 1)
        self.downsample_rate = round(c.frame_shift_ms * SAMPLE_RATE / 1000)
        self._lib = _lib.load()
        self.register_buffer("_device_probe", torch.zeros(1), persistent=False)

    def get_downsample_rates(self, key: str = None) -> int:
        return self.downsample_rate

    def num_frames(self, n: int) -> int:
        """Frames of an n-sample utterance of a kaldi configuration (the preprocessor's depend on the batch and the samples)."""
        t = C.c_int32()
        if self._spectral is not None:
            if "kaldi" not in self.config:
                raise ValueError("the frame count of a preprocessor configuration depends on the batch: run the forward")
            _lib.check(self._lib.s3enc_spectral_num_frames(C.byref(self._spectral), None, (C.c_int64 * 1)(int(n)), 1, C.byref(t), 0, None))
            return t.value
        _lib.check(self._lib.s3enc_fbank_num_frames(C.byref(self._c), int(n), C.byref(t)))
        return t.value

    def forward(self, wavs: List[torch.Tensor]):
        if len(wavs) == 0:
            raise ValueError("empty batch")
        if self._spectral is not None:
            out = spectral_forward(self._lib, self._spectral, wavs, self.output_dim)
            return {"last_hidden_state": out, "hidden_states": [out]}
        dev = wavs[0].device
        if dev.type != "cuda":
            raise RuntimeError("s3prl_amd runs the fbank upstream on an MI355X only (no CPU fallback); move the wavs to the GPU")
        held = [w.to(device=dev, dtype=torch.float32).contiguous() for w in wavs]
        lengths = [int(w.numel()) for w in held]
        frames = [self.num_frames(n) for n in lengths]
        if min(frames) < 1:
            raise ValueError("an utterance is shorter than one 25 ms analysis window")
        B, T = len(held), max(frames)
        out = torch.empty((B, T, self.output_dim), dtype=torch.float32, device=dev)
        ptrs = (C.c_void_p * B)(*[w.data_ptr() for w in held])
        lens = (C.c_int64 * B)(*lengths)
        idx = dev.index if dev.index is not None else torch.cuda.current_device()
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            rc = self._lib.s3enc_fbank_forward(C.byref(self._c), ptrs, lens, B, C.c_void_p(out.data_ptr()), T, idx,
                                               C.c_void_p(stream))
        _lib.check(rc, "s3enc_fbank_forward")
        return {"last_hidden_state": out, "hidden_states": [out]}
