"""A float64 restatement of BYOL-S's forward (upstream/byol_s/expert.py:30-36, serab_byols/serab.py:106-170, serab_byols/utils.py:31-106,
byol_a/models/resnetish.py, byol_a/models/audio_ntt.py, torchaudio's MelSpectrogram with win_length = 400) that needs neither the
reference tree nor torchaudio: the yardstick of the GPU tests and of the fuzz sweep.  ``tests/test_byol_s_cpu.py`` pins it to every
fixture the reference itself produced."""

from __future__ import annotations

import numpy as np

import byol_a_ref

N_FFT, WIN, HOP, N_MELS = 1024, 400, 160, 64
EPS = float(np.finfo(np.float32).eps)


def window_plan(n_max: int, window: int, step: int):
    """frame_audio (utils.py:51-106): the starts of the windows inside the row padded with window // 2 zeros in front and window -
    window // 2 behind; S = len(starts) = n_max // step + 1"""
    padded = n_max + window
    starts, k = [], 0
    while True:
        starts.append(int(round(k * step)))
        k += 1
        if not int(round(k * step)) + window <= padded:
            break
    return starts


def frame(wavs, window: int, step: int, dtype=np.float64) -> np.ndarray:
    """(B, S, window): pad_sequence to n_max, the centring pad, the windows"""
    n_max = max(len(w) for w in wavs)
    starts = window_plan(n_max, window, step)
    rows = []
    for w in wavs:
        p = np.zeros(n_max + window, dtype)
        p[window // 2:window // 2 + len(w)] = np.asarray(w, dtype)
        rows.append(np.stack([p[s:s + window] for s in starts]))
    return np.stack(rows)


def hann400_in_1024(dtype=np.float64) -> np.ndarray:
    """torch.stft's window for win_length = 400 < n_fft: the periodic hann(400) with (1024 - 400) // 2 = 312 zeros on either side"""
    win = np.zeros(N_FFT, dtype)
    win[(N_FFT - WIN) // 2:(N_FFT - WIN) // 2 + WIN] = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(WIN) / WIN)
    return win


def logmel(seg: np.ndarray, dtype=np.float64) -> np.ndarray:
    """(frames, 64): log(MelSpectrogram(seg) + eps) of one window, un-normalised"""
    x = np.pad(np.asarray(seg, dtype), N_FFT // 2, mode="reflect")
    T = 1 + len(seg) // HOP
    idx = np.arange(T)[:, None] * HOP + np.arange(N_FFT)[None, :]
    X = np.fft.rfft(x[idx].astype(np.float64) * hann400_in_1024(), axis=1)
    mel = (X.real ** 2 + X.imag ** 2).astype(dtype) @ byol_a_ref.mel_bank(dtype)
    return np.log(mel + dtype(EPS)).astype(dtype)


def batch_stats(lm: np.ndarray):
    """compute_timestamp_stats (utils.py:31-48) on the (N, frames, 64) log-mels: (mean / N, std / N), the std unbiased over every
    element — both divided by the number of windows, the reference's own arithmetic"""
    N = lm.shape[0]
    x = np.asarray(lm, np.float64)
    return float(x.mean() / N), float(x.std(ddof=1) / N)


def _bn(weights, name):
    g, b = weights[f"{name}.weight"].astype(np.float64), weights[f"{name}.bias"].astype(np.float64)
    rm, rv = weights[f"{name}.running_mean"].astype(np.float64), weights[f"{name}.running_var"].astype(np.float64)
    scale = g / np.sqrt(rv + byol_a_ref.BN_EPS)
    return scale, b - rm * scale


def resnetish(weights, blocks, x: np.ndarray) -> np.ndarray:
    """ResNetish(BasicBlock, blocks).forward in eval mode on (N, frames, 64) normalised log-mels -> (N, 2048), float64"""
    import torch
    import torch.nn.functional as F

    t = lambda a: torch.from_numpy(np.asarray(a, np.float64))  # noqa: E731

    def conv_bn(x, conv, bn, stride, padding):
        scale, shift = _bn(weights, bn)
        x = F.conv2d(x, t(weights[conv + ".weight"]), None, stride=stride, padding=padding)
        return x * t(scale)[None, :, None, None] + t(shift)[None, :, None, None]

    x = t(x).transpose(1, 2).unsqueeze(1)  # (N, 1, mel, time)
    x = F.max_pool2d(torch.relu(conv_bn(x, "conv1", "bn1", 1, 3)), 3, 2, 1)
    for L, n_blocks in enumerate(blocks):
        for b in range(n_blocks):
            pre = f"layer{L + 1}.{b}"
            stride = 2 if (L > 0 and b == 0) else 1
            out = torch.relu(conv_bn(x, pre + ".conv1", pre + ".bn1", stride, 1))
            out = conv_bn(out, pre + ".conv2", pre + ".bn2", 1, 1)
            identity = conv_bn(x, pre + ".downsample.0", pre + ".downsample.1", stride, 0) if pre + ".downsample.0.weight" in weights else x
            x = torch.relu(out + identity)
    x = x.permute(0, 3, 2, 1)  # (N, time, mel, ch)
    n, T, D, C = x.shape
    x = x.reshape(n, T, C * D)  # mel-major, channel-minor: d * 512 + c
    return (x.mean(1) + x.amax(1)).numpy()


def network(cfg, weights, x: np.ndarray) -> np.ndarray:
    if cfg.bs_network == "default":  # AudioNTT2020: BYOL-A's network, then mean(1) + amax(1)
        return byol_a_ref.network(weights, x)
    return resnetish(weights, cfg.bs_blocks, x)


def forward(cfg, weights, wavs, dtype=np.float64, stats=None):
    """{"state": (B, S, 2048), "logmel": (B, S, frames, 64) un-normalised, "stats": (mean / N, std / N), "starts"}.  ``stats``: use
    these two statistics instead of the batch's own (the fuzz sweep scores the network on the GPU's statistics)."""
    _, window, step = cfg.conv_layers[0]
    frames = frame(wavs, window, step, dtype)
    B, S = frames.shape[:2]
    lm = np.stack([logmel(f, dtype) for f in frames.reshape(B * S, window)])
    own = batch_stats(lm)
    mean, std = own if stats is None else stats
    x = (lm - dtype(mean)) / dtype(std)
    state = network(cfg, weights, x).reshape(B, S, -1)
    return {"state": state, "logmel": lm.reshape(B, S, *lm.shape[1:]), "stats": own,
            "starts": window_plan(max(len(w) for w in wavs), window, step)}
