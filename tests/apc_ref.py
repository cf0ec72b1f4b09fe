"""float64 numpy restatement of APC / VQ-APC (upstream/apc/apc.py:101-169, audio.py:53-115, expert.py:18-59), written from the
model's definition: the kaldi log-mel front end (hamming window, no deltas, CMVN over time) and GRU layers run on packed
sequences — an utterance's recurrence stops at its own frame count and the rows behind it are zeros.  The yardstick of the APC
tests on both sides: the reference-generated fixtures pin the model part on the CPU (the reference's own front end needs
torchaudio, so the fixtures are fed THIS front end's features, rounded to fp32); the GPU ops, the family and the fuzz cases are
compared with it.  The front end re-uses the helpers of ``oracle.fbank_oracle`` (mel banks, framing) and differs from that
oracle only in the window; with the povey window it equals it (tested to 1e-12)."""

import math

import numpy as np

from oracle import fbank_oracle as FO

import cpc_ref


def hamming_window(n: int) -> np.ndarray:
    """kaldi 'hamming': 0.54 - 0.46 cos(2 pi i / (N - 1)) (torch.hamming_window(periodic=False, alpha=0.54, beta=0.46))."""
    k = np.arange(n, dtype=np.float64)
    return 0.54 - 0.46 * np.cos(2.0 * math.pi * k / (n - 1))


def window(kind: str, n: int) -> np.ndarray:
    return {"hamming": hamming_window, "povey": FO.povey_window}[kind](n)


def kaldi_fbank(wav, num_mel_bins=80, frame_length=25.0, frame_shift=10.0, window_type="hamming", preemph=0.97, dtype=np.float64):
    """torchaudio.compliance.kaldi.fbank(num_mel_bins, frame_length, frame_shift, window_type) at 16 kHz, the other arguments at
    their defaults: (frames, num_mel_bins).  ``dtype`` = np.float32 evaluates every step but the FFT in fp32."""
    size, shift, padded = FO.frame_params(frame_length, frame_shift)
    wav = np.asarray(wav, dtype=dtype)
    m = FO.num_frames(len(wav), size, shift)
    if m == 0:
        return np.zeros((0, num_mel_bins), dtype=dtype)
    it = wav.itemsize
    frames = np.lib.stride_tricks.as_strided(np.ascontiguousarray(wav), shape=(m, size), strides=(shift * it, it)).copy()
    frames -= frames.mean(axis=1, keepdims=True)
    prev = np.concatenate([frames[:, :1], frames[:, :-1]], axis=1)
    frames = frames - dtype(preemph) * prev
    frames = frames * window(window_type, size).astype(dtype)
    spec = np.fft.rfft(frames.astype(np.float64), n=padded, axis=1)
    power = (spec.real ** 2 + spec.imag ** 2).astype(dtype)
    banks = FO.mel_banks(num_mel_bins, padded, FO.SAMPLE_RATE).astype(dtype)
    return np.log(np.maximum(power @ banks.T, dtype(FO.EPS32))).astype(dtype)


def cmvn(x, eps=1e-10):
    """apc/audio.py:43-47 over time: (x - mean) / (eps + std), std unbiased; one frame has no std (nan, like torch)."""
    std = x.std(axis=0, ddof=1, keepdims=True) if x.shape[0] > 1 else np.full((1, x.shape[1]), np.nan, dtype=x.dtype)
    return ((x - x.mean(axis=0, keepdims=True)) / (x.dtype.type(eps) + std)).astype(x.dtype)


def frontend(cfg, wav, dtype=np.float64):
    """FeatureExtractor.forward (apc/audio.py:81-94) on one waveform: (frames, feat_dim)."""
    y = kaldi_fbank(wav, cfg.apc_feat_dim, cfg.apc_frame_length, cfg.apc_frame_shift, cfg.apc_window, dtype=dtype)
    return cmvn(y) if cfg.apc_cmvn and y.shape[0] > 0 else y


def features(cfg, wavs, dtype=np.float64):
    """pad_sequence of the per-utterance features (apc/expert.py:48-52): (B, T, feat_dim) and the frame counts."""
    feats = [frontend(cfg, w, dtype) for w in wavs]
    lens = [f.shape[0] for f in feats]
    out = np.zeros((len(feats), max(lens), cfg.apc_feat_dim), dtype=dtype)
    for b, f in enumerate(feats):
        out[b, :f.shape[0]] = f
    return out, lens


def gru_layer_packed(x, lens, w_ih, w_hh, b_ih, b_hh):
    """nn.GRU(batch_first) on pack_padded_sequence(x, lens) -> pad_packed_sequence: every utterance runs its own length from a
    zero state, the rows behind it are zeros.  Returns (output, the gate pre-activations of the live rows)."""
    B, T, _ = x.shape
    H = w_hh.shape[1]
    out = np.zeros((B, T, H), dtype=x.dtype)
    gates = []
    for b, n in enumerate(lens):
        o, g = cpc_ref.rnn_layer(x[b:b + 1, :n], w_ih, w_hh, b_ih, b_hh, "GRU")
        out[b, :n] = o[0]
        gates.append(g.reshape(-1))
    return out, np.concatenate(gates)


def model(cfg, weights, feats, lens):
    """APC.forward (apc/apc.py:101-169) behind the front end, and what the expert's three hooks keep of it (expert.py:29-42):
    the inputs of rnn_layers[1] and rnn_layers[2] and the last layer's output after its residual."""
    x, outs, stds = np.asarray(feats, dtype=np.float64), [], []
    for l in range(cfg.apc_layers):
        g = lambda n: np.asarray(weights[f"rnn_layers.{l}.{n}_l0"], dtype=np.float64)  # noqa: E731
        y, gates = gru_layer_packed(x, lens, g("weight_ih"), g("weight_hh"), g("bias_ih"), g("bias_hh"))
        stds.append(float(gates.std()))
        if cfg.apc_residual and l > 0:
            y = y + x  # x is zero behind the lengths already
        outs.append(y)
        x = y
    return dict(hidden_states=[outs[0], outs[1], outs[-1]], gate_std=stds)


def forward(cfg, weights, wavs):
    feats, lens = features(cfg, wavs)
    out = model(cfg, weights, feats, lens)
    out["features"], out["lengths"] = feats, lens
    return out


# ---- the same model with every operation rounded to fp32: the CPU proxy of a GPU evaluation's error (make_golden_apc.py) --------
def forward_fp32(cfg, weights, wavs):
    f32 = np.float32
    feats, lens = features(cfg, wavs, dtype=f32)
    sig = lambda v: f32(1) / (f32(1) + np.exp(-v))  # noqa: E731
    x, outs = feats, []
    H = cfg.conv_dim
    for l in range(cfg.apc_layers):
        g = lambda n: np.asarray(weights[f"rnn_layers.{l}.{n}_l0"], dtype=f32)  # noqa: E731
        w_ih, w_hh, b_ih, b_hh = g("weight_ih"), g("weight_hh"), g("bias_ih"), g("bias_hh")
        y = np.zeros(x.shape[:2] + (H,), dtype=f32)
        for b, n in enumerate(lens):
            pre = x[b, :n] @ w_ih.T + b_ih
            h = np.zeros(H, dtype=f32)
            for t in range(n):
                a = w_hh @ h + b_hh
                r, z = sig(pre[t, :H] + a[:H]), sig(pre[t, H:2 * H] + a[H:2 * H])
                c = np.tanh(pre[t, 2 * H:] + r * a[2 * H:])
                h = ((f32(1) - z) * c + z * h).astype(f32)
                y[b, t] = h
        if cfg.apc_residual and l > 0:
            y = y + x
        outs.append(y)
        x = y
    return [outs[0], outs[1], outs[-1]]
