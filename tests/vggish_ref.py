"""float64 numpy restatement of VGGish (upstream/vggish/audio.py:30-84,256-294, vggish.py:18-133, expert.py:16-40) for any
configuration of family "vggish", written from the model's definition: the un-padded log-mel front end (periodic Hann window,
|rfft|, HTK mel matrix, log(. + offset)) cut into examples, the 3 x 3 conv + ReLU (+ 2 x 2 max-pool) stack, the flatten in
(frames, bands, channels) order, three Linear + ReLU layers, the PCA / clamp / round-half-to-even quantiser and ``pad_sequence``.
The yardstick of the VGGish tests on both sides: the reference-generated fixtures pin it on the CPU, the GPU family and the fuzz
cases are compared with it.  ``dtype=np.float32`` runs every operation in fp32: the CPU proxy of a GPU evaluation's error."""

import numpy as np


def mel_matrix(cfg, dtype=np.float64):
    """audio.py:174-253 at 16 kHz: (n_fft / 2 + 1, bands), edges linear in mel, DC row zero."""
    nb = cfg.vg_n_fft // 2 + 1
    mel = lambda f: 1127.0 * np.log(1.0 + np.asarray(f, np.float64) / 700.0)  # noqa: E731
    bins = mel(np.linspace(0.0, 8000.0, nb))
    edges = np.linspace(mel(cfg.vg_mel_min_hz), mel(cfg.vg_mel_max_hz), cfg.vg_num_mel_bins + 2)
    m = np.empty((nb, cfg.vg_num_mel_bins))
    for i in range(cfg.vg_num_mel_bins):
        lo, ce, hi = edges[i:i + 3]
        m[:, i] = np.maximum(0.0, np.minimum((bins - lo) / (ce - lo), (hi - bins) / (hi - ce)))
    m[0, :] = 0.0
    return m.astype(dtype)


def num_examples(cfg, n):
    _, window, shift = cfg.conv_layers[0]
    F = 1 + (n - window) // shift if n >= window else 0
    return 1 + (F - cfg.vg_example_frames) // cfg.vg_example_hop if F >= cfg.vg_example_frames else 0


def examples(cfg, wav, dtype=np.float64):
    """One utterance -> (E, frames, bands) log-mel examples; frames of an incomplete last example are not computed."""
    _, window, shift = cfg.conv_layers[0]
    E = num_examples(cfg, len(wav))
    assert E >= 1, (len(wav), "holds no example")
    F = E * cfg.vg_example_frames
    x = np.asarray(wav, dtype=dtype)
    idx = np.arange(F)[:, None] * shift + np.arange(window)[None, :]
    hann = (0.5 - 0.5 * np.cos(2 * np.pi / window * np.arange(window))).astype(dtype)
    frames = x[idx] * hann
    if dtype == np.float64:
        mag = np.abs(np.fft.rfft(frames, cfg.vg_n_fft))
    else:  # numpy's FFT computes in float64: the fp32 variant is the DFT as an fp32 matrix product, as the GPU path runs it
        k = np.arange(cfg.vg_n_fft // 2 + 1)[:, None] * np.arange(window)[None, :] % cfg.vg_n_fft
        ang = 2 * np.pi * k / cfg.vg_n_fft
        re, im = frames @ np.cos(ang).astype(dtype).T, frames @ (-np.sin(ang)).astype(dtype).T
        mag = np.sqrt(re * re + im * im)
    logmel = np.log(mag @ mel_matrix(cfg, dtype) + dtype(cfg.vg_log_offset))
    return logmel.reshape(E, cfg.vg_example_frames, cfg.vg_num_mel_bins).astype(dtype)


def conv3x3(x, w, b):
    """nn.Conv2d(C, N, 3, padding=1) on channel-last maps: x (E, H, W, C), w (N, C, 3, 3) -> (E, H, W, N)."""
    E, H, W, C = x.shape
    xp = np.zeros((E, H + 2, W + 2, C), dtype=x.dtype)
    xp[:, 1:H + 1, 1:W + 1] = x
    N = w.shape[0]
    wk = np.ascontiguousarray(w.transpose(2, 3, 1, 0)).reshape(3, 3 * C, N)  # [ky][kx * C + c][n]
    y = np.zeros((E * H * W, N), dtype=x.dtype) + b
    for ky in range(3):  # one contiguous (pixels, 3 C) patch matrix per kernel row: a BLAS product
        rows = np.concatenate([xp[:, ky:ky + H, kx:kx + W] for kx in range(3)], axis=3).reshape(E * H * W, 3 * C)
        y += rows @ wk[ky]
    return y.reshape(E, H, W, N)


def maxpool2(x):
    E, H, W, C = x.shape
    return x.reshape(E, H // 2, 2, W // 2, 2, C).max(axis=(2, 4))


def embed(cfg, weights, ex, dtype=np.float64):
    """VGG.forward (vggish.py:31-41) on (E, frames, bands) examples -> (E, D) embeddings."""
    g = lambda n: np.asarray(weights[n], dtype=dtype)  # noqa: E731
    x = np.asarray(ex, dtype=dtype)[..., None]
    for i, (_, pool) in enumerate(cfg.vg_layers):
        p = f"features.{cfg.vg_seq_index(i)}."
        x = np.maximum(conv3x3(x, g(p + "weight"), g(p + "bias")), 0)
        if pool:
            x = maxpool2(x)
    x = x.reshape(x.shape[0], -1)  # channel-last IS the reference's transposed flatten order (frames, bands, channels)
    for i in (0, 2, 4):
        x = np.maximum(x @ g(f"embeddings.{i}.weight").T + g(f"embeddings.{i}.bias"), 0)
    return x.astype(dtype)


def pre_round(cfg, weights, emb, dtype=np.float64):
    """Postprocessor.postprocess (vggish.py:77-117) up to the rounding: (clamp(P (y - m)) - min) * (255 / (max - min))."""
    P, m = np.asarray(weights["pca_eigen_vectors"], dtype=dtype), np.asarray(weights["pca_means"], dtype=dtype).reshape(-1)
    lo, hi = dtype(cfg.vg_quant_min), dtype(cfg.vg_quant_max)
    z = np.clip((emb - m) @ P.T, lo, hi)
    return (z - lo) * dtype(255.0 / (cfg.vg_quant_max - cfg.vg_quant_min))


def forward(cfg, weights, wavs, dtype=np.float64):
    """The expert's forward.  Returns a dict: ``state`` (B, E_max, D) — quantised (np.rint: half to even) with postprocess, else the
    embeddings — zero rows behind every utterance's own examples; ``pre`` (the float pre-rounding values, same layout, postprocess
    only); ``emb`` (the padded embeddings); ``counts`` (examples per utterance); ``examples`` (the per-utterance log-mel examples)."""
    exs = [examples(cfg, w, dtype) for w in wavs]
    counts = [e.shape[0] for e in exs]
    embs = embed(cfg, weights, np.concatenate(exs), dtype)
    D, E_max = embs.shape[1], max(counts)
    emb = np.zeros((len(wavs), E_max, D), dtype=dtype)
    pre = np.zeros_like(emb) if cfg.vg_postprocess else None
    o = 0
    for b, n in enumerate(counts):
        emb[b, :n] = embs[o:o + n]
        if cfg.vg_postprocess:
            pre[b, :n] = pre_round(cfg, weights, embs[o:o + n], dtype)
        o += n
    state = np.rint(pre) if cfg.vg_postprocess else emb
    for b, n in enumerate(counts):
        state[b, n:] = 0
    return dict(state=state, pre=pre, emb=emb, counts=counts, examples=exs)
