"""A float64 restatement of BYOL-A's forward (upstream/byol_a/expert.py:83-125, byol_a.py:91-137, torchaudio's MelSpectrogram
defaults) that needs neither the reference tree nor torchaudio: the yardstick of the GPU tests and of the fuzz sweep.
``tests/test_byol_a_cpu.py`` pins it to every fixture the reference itself produced."""

from __future__ import annotations

import numpy as np

SAMPLE_RATE = 16000
N_FFT, HOP, N_MELS, F_MIN, F_MAX = 1024, 160, 64, 60.0, 7800.0
MEAN, STD = -5.4919195, 5.0389895
EPS = float(np.finfo(np.float32).eps)
BN_EPS = 1e-5


def segment_plan(lengths, window: int, stride: int):
    """expert.py:83-86: (starts, padded length); S = len(starts)."""
    starts = list(range(0, max(lengths), stride))
    return starts, starts[-1] + window


def mel_bank(dtype=np.float64):
    """torchaudio.functional.melscale_fbanks(513, 60, 7800, 64, 16000, norm=None, mel_scale="htk"): (513, 64)."""
    freqs = np.linspace(0.0, SAMPLE_RATE // 2, N_FFT // 2 + 1)
    m_min, m_max = 2595.0 * np.log10(1.0 + F_MIN / 700.0), 2595.0 * np.log10(1.0 + F_MAX / 700.0)
    f_pts = 700.0 * (10.0 ** (np.linspace(m_min, m_max, N_MELS + 2) / 2595.0) - 1.0)
    f_diff = f_pts[1:] - f_pts[:-1]
    slopes = f_pts[None, :] - freqs[:, None]
    down, up = -slopes[:, :-2] / f_diff[:-1], slopes[:, 2:] / f_diff[1:]
    return np.maximum(0.0, np.minimum(down, up)).astype(dtype)


def power_spectrum(seg: np.ndarray, dtype=np.float64) -> np.ndarray:
    """(frames, 513): torch.stft(seg, 1024, 160, window=hann_window(1024), center=True, pad_mode="reflect").abs() ** 2"""
    x = np.pad(np.asarray(seg, dtype), N_FFT // 2, mode="reflect")
    T = 1 + len(seg) // HOP
    idx = np.arange(T)[:, None] * HOP + np.arange(N_FFT)[None, :]
    win = (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(N_FFT) / N_FFT)).astype(dtype)
    X = np.fft.rfft(x[idx].astype(np.float64) * win.astype(np.float64), axis=1)
    return (X.real ** 2 + X.imag ** 2).astype(dtype)


def logmel(seg: np.ndarray, dtype=np.float64) -> np.ndarray:
    """(frames, 64): the normalised log-mel of one segment"""
    mel = power_spectrum(seg, dtype) @ mel_bank(dtype)
    return ((np.log(mel + dtype(EPS)) - dtype(MEAN)) / dtype(STD)).astype(dtype)


def affine(weights, k: int):
    """the eval-mode BatchNorm2d behind conv ``features.k`` as (scale, shift) with the conv bias inside, float64"""
    g, b = weights[f"features.{k + 1}.weight"].astype(np.float64), weights[f"features.{k + 1}.bias"].astype(np.float64)
    rm, rv = weights[f"features.{k + 1}.running_mean"].astype(np.float64), weights[f"features.{k + 1}.running_var"].astype(np.float64)
    scale = g / np.sqrt(rv + BN_EPS)
    return scale, (weights[f"features.{k}.bias"].astype(np.float64) - rm) * scale + b


def network(weights, feats: np.ndarray) -> np.ndarray:
    """AudioNTT2020.forward on (nseg, frames, 64) log-mels -> (nseg, d), float64"""
    import torch
    import torch.nn.functional as F

    x = torch.from_numpy(np.asarray(feats, np.float64)).transpose(1, 2).unsqueeze(1)  # (nseg, 1, mel, time)
    for k in (0, 4, 8):
        scale, shift = affine(weights, k)
        x = F.conv2d(x, torch.from_numpy(weights[f"features.{k}.weight"].astype(np.float64)), None, padding=1)
        x = x * torch.from_numpy(scale)[None, :, None, None] + torch.from_numpy(shift)[None, :, None, None]
        x = F.max_pool2d(torch.relu(x), 2, 2)
    x = x.permute(0, 3, 2, 1)  # (nseg, time, mel, ch)
    n, T, D, C = x.shape
    x = x.reshape(n, T, D * C)  # mel-major, channel-minor: d * 64 + c
    x = torch.relu(x @ torch.from_numpy(weights["fc.0.weight"].astype(np.float64)).T + torch.from_numpy(weights["fc.0.bias"].astype(np.float64)))
    x = torch.relu(x @ torch.from_numpy(weights["fc.3.weight"].astype(np.float64)).T + torch.from_numpy(weights["fc.3.bias"].astype(np.float64)))
    return (x.max(dim=1).values + x.mean(dim=1)).numpy()


def forward(cfg, weights, wavs, dtype=np.float64):
    """{"state": (B, S, d), "logmel": (B, S, frames, 64), "starts", "padded_len"} for a list of numpy waveforms"""
    _, window, stride = cfg.conv_layers[0]
    lengths = [len(w) for w in wavs]
    starts, padded_len = segment_plan(lengths, window, stride)
    feats = []
    for w in wavs:
        p = np.concatenate([np.asarray(w, dtype), np.zeros(padded_len - len(w), dtype)])
        feats.append(np.stack([logmel(p[s:s + window], dtype) for s in starts]))
    feats = np.stack(feats)  # (B, S, frames, 64)
    B, S = feats.shape[:2]
    state = network(weights, feats.reshape(B * S, *feats.shape[2:])).reshape(B, S, -1)
    return {"state": state, "logmel": feats, "starts": starts, "padded_len": padded_len}
