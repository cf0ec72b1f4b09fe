"""float64 numpy restatement of the Mockingjay / TERA / AudioALBERT family (upstream/mockingjay/{expert,builder,model}.py,
upstream/baseline/preprocessor.py), written from the definitions: the ``OnlinePreprocessor`` front end (decibel scale, centred
periodic-hann STFT of the zero-PADDED batch with reflect padding, HTK mel, log, CMVN over a batch-dependent frame count), the input
representation (Linear + sinusoid position row + TF-style LayerNorm with the checkpoint's eps), post-LN BERT layers (optionally one
layer's weights run several times) and the chunked forward for inputs over ``sequence_length`` frames.  The yardstick of the
Mockingjay tests on both sides: the reference-generated fixtures pin the model part on the CPU (torchaudio is absent, so the
fixtures are fed THIS front end's features, rounded to fp32); the GPU ops, the family and the fuzz cases are compared with it.  The
kaldi front end is ``oracle.fbank_oracle`` (povey window) through ``apc_ref``'s helpers."""

import math

import numpy as np

TARGET_EPS = 1e-10


# ---- front end --------------------------------------------------------------------------------------------------------------
def hann_periodic(n: int = 400) -> np.ndarray:
    return 0.5 - 0.5 * np.cos(2.0 * math.pi * np.arange(n, dtype=np.float64) / n)


def mel_banks(n_mels: int, n_freqs: int = 201, f_min: float = 0.0, f_max: float = 8000.0) -> np.ndarray:
    """MelScale's defaults in closed form (HTK mel scale, no norm): triangles in Hz whose corners are equally spaced in mel;
    (n_freqs, n_mels)."""
    freqs = np.linspace(0.0, 8000.0, n_freqs)
    hz2mel = lambda f: 2595.0 * np.log10(1.0 + f / 700.0)  # noqa: E731
    m = np.linspace(hz2mel(f_min), hz2mel(f_max), n_mels + 2)
    f = 700.0 * (10.0 ** (m / 2595.0) - 1.0)
    down = (freqs[:, None] - f[None, :-2]) / (f[1:-1] - f[:-2])[None]
    up = (f[None, 2:] - freqs[:, None]) / (f[2:] - f[1:-1])[None]
    return np.maximum(0.0, np.minimum(down, up))


def decibel_scale(wav, target_level=-25.0, dtype=np.float64):
    """builder.py:129-134: x * 10^(level / 20) / (rms + 1e-10), the rms over the utterance's own samples."""
    wav = np.asarray(wav, dtype=dtype)
    rms = np.sqrt(np.mean(wav * wav, dtype=dtype))
    return (wav * (dtype(10.0 ** (target_level / 20.0)) / (rms + dtype(TARGET_EPS)))).astype(dtype)


def stft_power(batch: np.ndarray) -> np.ndarray:
    """torch.stft(n_fft 400, hop 160, win 400, periodic hann, center, reflect, onesided, unnormalised) of the rows of a padded
    (B, max_len) batch, as |X|^2: (B, 1 + max_len // 160, 201)."""
    B, n = batch.shape
    if n <= 200:
        raise ValueError("reflect padding needs more than 200 samples")
    x = np.pad(np.asarray(batch, dtype=np.float64), ((0, 0), (200, 200)), mode="reflect")
    T = 1 + n // 160
    idx = 160 * np.arange(T)[:, None] + np.arange(400)[None]
    spec = np.fft.rfft(x[:, idx] * hann_periodic(), axis=-1)
    return spec.real ** 2 + spec.imag ** 2


def frame_counts(lengths, max_len=None):
    """preprocessor.py:204-205, with Python floats and Python's round: batch-dependent."""
    max_len = max(lengths) if max_len is None else max_len
    T = 1 + max_len // 160
    return [min(T, round(n / (max_len / T))) for n in lengths]


def cmvn_rows(x, eps=TARGET_EPS):
    std = x.std(axis=0, ddof=1, keepdims=True) if x.shape[0] > 1 else np.full((1, x.shape[1]), np.nan, dtype=x.dtype)
    return ((x - x.mean(axis=0, keepdims=True)) / (std + x.dtype.type(eps))).astype(x.dtype)


def logmel(wavs, n_mels=80, target_level=-25.0, cmvn=True, max_len=None, dtype=np.float64):
    """The ``audio.input`` path: (B, T, n_mels) and the frame counts (with CMVN: rows behind a count are zeros; without: every
    row is a feature of the padded signal and the count is T).  ``dtype`` = np.float32 rounds every step but the FFT to fp32."""
    lengths = [len(w) for w in wavs]
    max_len = max(lengths) if max_len is None else max_len
    batch = np.zeros((len(wavs), max_len), dtype=dtype)
    for b, w in enumerate(wavs):
        batch[b, :len(w)] = decibel_scale(w, target_level, dtype)
    power = stft_power(batch).astype(dtype)
    feats = np.log(power @ mel_banks(n_mels).astype(dtype) + dtype(TARGET_EPS)).astype(dtype)
    T = feats.shape[1]
    if not cmvn:
        return feats, [T] * len(wavs)
    counts = frame_counts(lengths, max_len)
    out = np.zeros_like(feats)
    for b, n in enumerate(counts):
        out[b, :n] = cmvn_rows(feats[b, :n])
    return out, counts


def kaldi_features(cfg, wavs, dtype=np.float64):
    """The ``audio.kaldi`` path (baseline/extracter.py): kaldi fbank (povey) -> deltas -> CMVN per utterance -> pad_sequence."""
    from oracle import fbank_oracle as FO

    import apc_ref

    feats = []
    for w in wavs:
        y = apc_ref.kaldi_fbank(w, cfg.mj_kaldi_mel_bins, cfg.mj_kaldi_frame_length, cfg.mj_kaldi_frame_shift, "povey",
                                cfg.mj_kaldi_preemphasis, dtype=dtype)
        parts = [y]
        for _ in range(cfg.mj_delta_order):
            parts.append(FO.compute_deltas(parts[-1], cfg.mj_delta_win).astype(dtype))
        y = np.concatenate(parts, axis=1)
        feats.append(cmvn_rows(y) if cfg.mj_cmvn else y)
    lens = [f.shape[0] for f in feats]
    out = np.zeros((len(feats), max(lens), feats[0].shape[1]), dtype=dtype)
    for b, f in enumerate(feats):
        out[b, :f.shape[0]] = f
    return out, lens


def features(cfg, wavs, max_len=None, dtype=np.float64):
    if cfg.mj_frontend == "kaldi":
        return kaldi_features(cfg, wavs, dtype)
    return logmel(wavs, cfg.mj_input_dim, cfg.mj_target_level, cfg.mj_cmvn, max_len, dtype)


# ---- model ------------------------------------------------------------------------------------------------------------------
def position_table(rows: int, D: int) -> np.ndarray:
    """builder.py:469-481: pos / 10000^(2 (j // 2) / D), sin on even j, cos on odd j; float64 rounded once to fp32."""
    j = np.arange(D)
    ang = np.arange(rows, dtype=np.float64)[:, None] / np.power(10000.0, 2.0 * (j // 2) / D)[None]
    ang[:, 0::2] = np.sin(ang[:, 0::2])
    ang[:, 1::2] = np.cos(ang[:, 1::2])
    return ang.astype(np.float32)


def layer_norm(x, g, b, eps):
    u = x.mean(-1, keepdims=True)
    s = ((x - u) ** 2).mean(-1, keepdims=True)
    return (x - u) / np.sqrt(s + x.dtype.type(eps)) * g + b


def chunk_sizes(T: int, sequence_length: int):
    """torch.chunk(x, ceil(T / sequence_length), dim=1): equal chunks of ceil(T / n) rows, a shorter last one."""
    if sequence_length <= 0 or T <= sequence_length:
        return [T]
    n = -(-T // sequence_length)
    size = -(-T // n)
    return [min(size, T - s) for s in range(0, T, size)]


def _erf(x):
    try:
        from scipy.special import erf

        return erf(x)
    except Exception:  # pragma: no cover
        return np.vectorize(math.erf)(x)


def _w(weights, name, dtype):
    return np.asarray(weights[name], dtype=dtype)


def model_chunk(cfg, weights, feats, counts, dtype=np.float64):
    """TransformerModel on one chunk (B, Tc, F) with ``counts`` live frames per utterance: the states (input representation, then
    every layer's output).  Keys at or behind a count get the additive -10000 of the reference; an utterance without a live key
    attends uniformly, as there."""
    D, H, eps = cfg.encoder_embed_dim, cfg.encoder_attention_heads, cfg.mj_layer_norm_eps
    B, Tc, _ = feats.shape
    w = lambda n: _w(weights, n, dtype)  # noqa: E731
    x = np.asarray(feats, dtype=dtype) @ w("input_representations.spec_transform.weight").T + w("input_representations.spec_transform.bias")
    x = x + position_table(Tc, D).astype(dtype)[None]
    x = layer_norm(x, w("input_representations.LayerNorm.weight"), w("input_representations.LayerNorm.bias"), eps)
    mask = np.zeros((B, 1, 1, Tc), dtype=dtype)
    for b, n in enumerate(counts):
        mask[b, ..., n:] = -10000.0
    states, stds = [x], []
    for l in range(cfg.encoder_layers):
        p = f"encoder.layer.{0 if cfg.mj_share_layer else l}."
        split = lambda y: y.reshape(B, Tc, H, 64).transpose(0, 2, 1, 3)  # noqa: E731
        q = split(x @ w(p + "attention.self.query.weight").T + w(p + "attention.self.query.bias"))
        k = split(x @ w(p + "attention.self.key.weight").T + w(p + "attention.self.key.bias"))
        v = split(x @ w(p + "attention.self.value.weight").T + w(p + "attention.self.value.bias"))
        s = q @ k.transpose(0, 1, 3, 2) / dtype(8.0) + mask
        for b, n in enumerate(counts):
            if n > 0:
                stds.append(float(s[b, :, :n, :n].std()))
        s = s - s.max(-1, keepdims=True)
        pr = np.exp(s)
        pr = pr / pr.sum(-1, keepdims=True)
        ctx = (pr @ v).transpose(0, 2, 1, 3).reshape(B, Tc, D)
        a = ctx @ w(p + "attention.output.dense.weight").T + w(p + "attention.output.dense.bias") + x
        a = layer_norm(a, w(p + "attention.output.LayerNorm.weight"), w(p + "attention.output.LayerNorm.bias"), eps)
        h = a @ w(p + "intermediate.dense.weight").T + w(p + "intermediate.dense.bias")
        h = (h * dtype(0.5) * (dtype(1.0) + _erf(h / dtype(math.sqrt(2.0))))).astype(dtype)
        y = h @ w(p + "output.dense.weight").T + w(p + "output.dense.bias") + a
        x = layer_norm(y, w(p + "output.LayerNorm.weight"), w(p + "output.LayerNorm.bias"), eps)
        states.append(x)
    return states, stds


def model(cfg, weights, feats, counts, dtype=np.float64):
    """builder.py:250-289: the whole sequence at once, or in torch.chunk pieces with the states concatenated along time."""
    T = feats.shape[1]
    outs, stds, s = None, [], 0
    for size in chunk_sizes(T, cfg.mj_sequence_length):
        st, sd = model_chunk(cfg, weights, feats[:, s:s + size], [min(max(n - s, 0), size) for n in counts], dtype)
        outs = st if outs is None else [np.concatenate([a, b], axis=1) for a, b in zip(outs, st)]
        stds += sd
        s += size
    return dict(hidden_states=outs, score_std=stds)


def forward(cfg, weights, wavs, max_len=None):
    feats, counts = features(cfg, wavs, max_len)
    out = model(cfg, weights, feats, counts)
    out["features"], out["lengths"] = feats, counts
    return out


def forward_fp32(cfg, weights, wavs):
    """The same model with every operation rounded to fp32: the CPU proxy of a GPU evaluation's error (make_golden_mockingjay.py)."""
    feats, counts = features(cfg, wavs, dtype=np.float32)
    return model(cfg, weights, feats, counts, dtype=np.float32)["hidden_states"]
