#!/usr/bin/env python3
"""Generate the BYOL-S fixtures under ``tests/golden/byol_s/`` by RUNNING THE REFERENCE (PyTorch CPU) on seeded weights and waveforms.

Run in the build container only (it imports the reference tree through ``ref_shim``):

    python tests/golden/make_golden_byol_s.py                 # all cases + the hub-signature fixture
    python tests/golden/make_golden_byol_s.py byol_s_tiny_pad

NO torchaudio RUN STANDS BEHIND THESE FIXTURES.  torchaudio is not installed here; ``ref_shim`` stands in for the module (the
top-level ``import torchaudio`` of ``byol_a/common.py`` and ``byol_a/augmentations.py`` resolves to a placeholder), and ONLY the
``MelSpectrogram`` that ``serab.get_timestamp_embeddings`` builds is replaced, by a float32 restatement of torchaudio's transform at
the reference's own arguments: ``torch.stft(n_fft = 1024, hop 160, win_length = 400, periodic hann(400), center = True, pad_mode =
"reflect", onesided, not normalized)``, ``|.|^2``, and the float32 ``melscale_fbanks(513, 60, 7800, 64, 16000, norm = None, "htk")``
matrix computed with torchaudio's own expressions.  Everything else — ``pad_sequence``, ``frame_audio``, the ``log(. + eps)``,
``compute_timestamp_stats`` with its division by the number of windows, ``PrecomputedNorm``, the networks (loaded by the reference's
``load_model`` from a ``synth.py`` checkpoint file) and the reshapes — is the reference's own code, run in ``.eval()``.  The tiny ResNet
is the reference's own ``ResNetish(BasicBlock, [1, 1, 1, 1])`` put in place of ``expert.model``.

Same ``.npz`` meta format as the other generators (``conftest.load_golden`` reads them as ``"byol_s/<case>"``: ``n_states = 1``, seeds
instead of weights).  Every fixture is recorded whole: (B, S, 2048) is at most 3 x 6 x 2048 floats.  The meta records the reference's
two statistics, the number of windows N, and ``restatement_err`` / ``restatement_row_err``: the float64 restatement
``tests/byol_s_ref.py`` against the reference's fp32 output, whole and per (utterance, window) row.  ``bound`` is what the GPU is held
to: ``FP32_TOL`` = 1e-4 when the restatement is within a quarter of it; otherwise the reference's own fp32 rounding against float64
is larger than that, the measured figure is recorded as ``reference_fp32_vs_float64`` and the bound is four times it (the quarter rule
turned round).
"""

from __future__ import annotations

import inspect
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import byol_s_ref  # noqa: E402
from make_golden import _load  # noqa: E402
from s3prl_amd.synth import named_config, synth_wavs, synth_weights  # noqa: E402

FP32_TOL = 1e-4
MAX_RESTATEMENT_ERR = 0.25 * FP32_TOL
MAX_BYTES = 256 * 1024

# name -> (config, weight seed, wav seed, lengths, dc, scale)
CASES = {
    "byol_s_tiny_eq": ("tiny_byol_s_resnetish10", 1401, 1501, [2400, 2400], 0.0, 1.0),
    # step 800: one utterance shorter than a step, one exactly k * step, one k * step + 1
    "byol_s_tiny_pad": ("tiny_byol_s_resnetish10", 1401, 1502, [500, 2400, 2401], 0.0, 1.0),
    # window 4000, step 1600: 26 frames -> 13 -> 7 -> 4 -> 2, odd at two levels
    "byol_s_tiny_win025": ("tiny_byol_s_resnetish10_win025", 1402, 1503, [9000, 4800, 4801], 0.05, 0.5),
    # hop_secs 0.2 at a half-second window
    "byol_s_tiny_hop02": ("tiny_byol_s_resnetish10_hop02", 1403, 1504, [9000, 6400], 0.0, 1.0),
    "byol_s_tiny_default": ("tiny_byol_s_default", 1404, 1505, [6000, 3200, 1000], 0.0, 1.0),
    "byol_s_resnetish34_pseudo": ("byol_s_resnetish34", 1405, 1506, [2400, 1601, 500], 0.0, 1.0),
    "byol_s_default_pseudo": ("byol_s_default", 1406, 1507, [2400, 1601, 500], 0.0, 1.0),
}


def _import_reference():
    import ref_shim

    ref_shim.import_reference(roots=("torchaudio", "omegaconf", "einops"))
    import importlib

    importlib.import_module("torchaudio.transforms")  # a placeholder MODULE, so that serab.py's `from ... import MelSpectrogram` resolves


def rel(a, b):
    return float(np.linalg.norm(np.asarray(a, np.float64) - np.asarray(b, np.float64)) / np.linalg.norm(np.asarray(b, np.float64)))


class MelSpectrogramFp32:
    """``torchaudio.transforms.MelSpectrogram(sample_rate, n_fft, win_length, hop_length, n_mels, f_min, f_max)`` restated in float32
    torch for the arguments the reference passes: (..., n) -> (..., n_mels, 1 + n // hop)."""

    def __init__(self, sample_rate, n_fft, win_length, hop_length, n_mels, f_min, f_max):
        import math

        import torch

        assert (sample_rate, n_fft, win_length, hop_length, n_mels, f_min, f_max) == (16000, 1024, 400, 160, 64, 60, 7800)
        self.n_fft, self.win_length, self.hop = n_fft, win_length, hop_length
        self.window = torch.hann_window(win_length)
        all_freqs = torch.linspace(0, sample_rate // 2, n_fft // 2 + 1)
        m_min, m_max = 2595.0 * math.log10(1.0 + f_min / 700.0), 2595.0 * math.log10(1.0 + f_max / 700.0)
        f_pts = 700.0 * (10 ** (torch.linspace(m_min, m_max, n_mels + 2) / 2595.0) - 1.0)
        f_diff = f_pts[1:] - f_pts[:-1]
        slopes = f_pts.unsqueeze(0) - all_freqs.unsqueeze(1)
        self.fb = torch.max(torch.zeros(1), torch.min(-slopes[:, :-2] / f_diff[:-1], slopes[:, 2:] / f_diff[1:]))  # (513, 64)

    def to(self, device):
        return self

    def __call__(self, wav):
        import torch

        spec = torch.stft(wav, self.n_fft, self.hop, self.win_length, window=self.window, center=True, pad_mode="reflect",
                          normalized=False, onesided=True, return_complex=True).abs().pow(2.0)  # (..., 513, frames)
        return torch.matmul(spec.transpose(-1, -2), self.fb).transpose(-1, -2)


def reference_expert(cfg, weights, tmpdir, recorded):
    import torch

    _import_reference()
    from s3prl.upstream.byol_s.byol_a.models.audio_ntt import AudioNTT2020
    from s3prl.upstream.byol_s.byol_a.models.resnetish import BasicBlock, ResNetish, resnetish34
    from s3prl.upstream.byol_s.expert import UpstreamExpert
    from s3prl.upstream.byol_s.serab_byols import serab

    serab.MelSpectrogram = MelSpectrogramFp32
    stats_fn = serab.compute_timestamp_stats.__wrapped__ if hasattr(serab.compute_timestamp_stats, "__wrapped__") else serab.compute_timestamp_stats

    def recording_stats(melspec):
        stats = stats_fn(melspec)
        recorded["stats"], recorded["N"] = [float(s) for s in stats], int(len(melspec))
        return stats

    recording_stats.__wrapped__ = stats_fn
    serab.compute_timestamp_stats = recording_stats

    released = {(3, 4, 6, 3): ("resnetish34", resnetish34)}
    if cfg.bs_network == "default" or tuple(cfg.bs_blocks) in released:
        name, build = ("default", lambda: AudioNTT2020(n_mels=64, d=2048)) if cfg.bs_network == "default" else released[tuple(cfg.bs_blocks)]
        model = build()
        _load(model, weights)
        path = os.path.join(tmpdir, "byol_s.pth")
        torch.save(model.state_dict(), path)
        expert = UpstreamExpert(path, name, window_secs=cfg.bs_window_secs, hop_secs=cfg.bs_hop_secs)
    else:  # a ResNet the reference has no name for: its own classes, put in place of the model the constructor loaded
        stand_in = AudioNTT2020(n_mels=64, d=2048)
        path = os.path.join(tmpdir, "stand_in.pth")
        torch.save(stand_in.state_dict(), path)
        expert = UpstreamExpert(path, "default", window_secs=cfg.bs_window_secs, hop_secs=cfg.bs_hop_secs)
        model = ResNetish(BasicBlock, list(cfg.bs_blocks))
        _load(model, weights)
        expert.model = model
    expert = expert.eval()
    assert expert.get_downsample_rates("hidden_states") == cfg.conv_layers[0][2]
    return expert


def make_case(name: str):
    import torch

    cfg_name, wseed, xseed, lengths, dc, scale = CASES[name]
    cfg = named_config(cfg_name)
    weights = synth_weights(cfg, wseed)
    wavs = synth_wavs(lengths, xseed, dc=dc, scale=scale)
    recorded = {}
    with tempfile.TemporaryDirectory() as tmp:
        expert = reference_expert(cfg, weights, tmp, recorded)
        with torch.no_grad():
            out = expert([torch.from_numpy(w.copy()) for w in wavs])
    hs = out["hidden_states"]
    assert len(hs) == 1
    h = hs[0].numpy()
    _, window, step = cfg.conv_layers[0]
    S = cfg.num_frames(max(lengths))
    assert h.shape == (len(lengths), S, 2048) and h.dtype == np.float32, (h.shape, h.dtype)
    assert recorded["N"] == len(lengths) * S
    ref = byol_s_ref.forward(cfg, weights, wavs)
    mine = ref["state"]
    err = rel(mine, h)
    row_err = max(rel(mine[b, s], h[b, s]) for b in range(h.shape[0]) for s in range(S))
    stats_err = max(abs(a - b) / abs(b) for a, b in zip(ref["stats"], recorded["stats"]))
    assert stats_err < 1e-5, (ref["stats"], recorded["stats"])
    own = [cfg.num_frames(n) for n in lengths]
    pad_rows = [(b, s) for b in range(len(lengths)) for s in range(own[b], S)]
    assert all(np.abs(h[b, s]).max() > 0 for b, s in pad_rows)  # rows past an utterance's length are not zeros
    meta = dict(config=cfg_name, weight_seed=wseed, wav_seed=xseed, lengths=lengths, frames=own, windows=S, N=recorded["N"], dc=dc,
                scale=scale, shape=list(h.shape), n_states=1, window=window, step=step, stats=recorded["stats"],
                reference="s3prl 0.4.18 byol_s/expert.py (.eval()), torch CPU fp32; serab.py's MelSpectrogram replaced by a float32 "
                          "torch.stft + mel-bank restatement of torchaudio's transform at win_length = 400 (no torchaudio run)",
                zeros=float((h == 0).mean()), restatement_err=err, restatement_row_err=row_err, bound=FP32_TOL)
    worst = max(err, row_err)
    if worst > MAX_RESTATEMENT_ERR:
        # the reference's own fp32 rounding against float64 exceeds a quarter of FP32_TOL on this network: recorded, and the GPU is
        # held to four times the measured figure
        meta["reference_fp32_vs_float64"] = worst
        meta["bound"] = 4.0 * worst
    arrays = {"hs0": h, "norms": np.array([np.linalg.norm(h.astype(np.float64))]),
              "meta": np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)}
    os.makedirs(os.path.join(HERE, "byol_s"), exist_ok=True)
    path = os.path.join(HERE, "byol_s", f"{name}.npz")
    np.savez_compressed(path, **arrays)
    assert os.path.getsize(path) < MAX_BYTES, (path, os.path.getsize(path))
    print(f"{name}: shape {h.shape}, own windows {own}, stats {recorded['stats']}, zeros {meta['zeros']:.3f}, byol_s_ref float64 vs "
          f"reference {err:.2e} whole / {row_err:.2e} worst row, bound {meta['bound']:.2e} -> {os.path.getsize(path) / 1e3:.0f} kB")


def make_hub_fixture():
    """names and signatures of the reference's byol_s hubconf, in reference_hub_byol_a.json's layout"""
    _import_reference()
    import importlib

    mod = importlib.import_module("s3prl.upstream.byol_s.hubconf")
    sig = lambda f: [[k, v.kind.name, repr(v.default)] for k, v in inspect.signature(f).parameters.items()]  # noqa: E731
    res = {"byol_s": [[n, sig(f)] for n, f in vars(mod).items()
                      if inspect.isfunction(f) and not n.startswith("_") and f.__module__ == mod.__name__]}
    expert = importlib.import_module("s3prl.upstream.byol_s.expert").UpstreamExpert
    os.makedirs(os.path.join(HERE, "byol_s"), exist_ok=True)
    with open(os.path.join(HERE, "byol_s", "reference_hub_byol_s.json"), "w") as f:
        json.dump(dict(reference="s3prl 0.4.18: s3prl.upstream.byol_s.hubconf", hubconfs=res, expert_init=sig(expert.__init__)), f,
                  indent=1, sort_keys=True)


if __name__ == "__main__":
    names = sys.argv[1:] or list(CASES) + ["hub"]
    for n in names:
        make_hub_fixture() if n == "hub" else make_case(n)
