#!/usr/bin/env python3
"""Generate the BYOL-A fixtures under ``tests/golden/byol_a/`` by RUNNING THE REFERENCE (PyTorch CPU) on seeded weights and waveforms.

Run in the build container only (it imports the reference tree through ``ref_shim``):

    python tests/golden/make_golden_byol_a.py                 # all cases + the hub-signature fixture
    python tests/golden/make_golden_byol_a.py byol_a_tiny_pad

NO torchaudio RUN STANDS BEHIND THESE FIXTURES.  torchaudio is not installed here, and the reference's expert builds its front end
from ``torchaudio.transforms.MelSpectrogram``.  The generator builds the reference's ``UpstreamExpert`` on a ``synth.py`` checkpoint
and replaces ONLY ``expert.to_melspec`` with a float32 restatement of ``MelSpectrogram``'s defaults: ``torch.stft(n_fft = win_length
= 1024, hop 160, periodic hann, center = True, pad_mode = "reflect", onesided, not normalized)``, ``|.|^2``, and the float32
``melscale_fbanks(513, 60, 7800, 64, 16000, norm = None, "htk")`` matrix computed with torchaudio's own expressions.  Everything else
— the zero padding and segmenting, the ``log(. + eps)``, ``PrecomputedNorm``, ``AudioNTT2020`` (loaded through its own
``load_weight`` from a file), the reshapes and the trimming — is the reference's own code.

Same ``.npz`` meta format as the other generators (``conftest.load_golden`` reads them as ``"byol_a/<case>"``: ``n_states = 1``, seeds
instead of weights).  Every fixture is recorded whole: (B, S, d) is at most 3 x 3 x 2048 floats.  A case is written only when the
float64 restatement ``tests/byol_a_ref.py`` stays within a quarter of the GPU tests' ``FP32_TOL`` = 1e-4 of the reference's output,
whole and per (utterance, segment) row.

Measured when the committed fixtures were written (case: whole-tensor / worst-row relative difference of byol_a_ref, float64):
  see the ``restatement_err`` / ``restatement_row_err`` entries of every fixture's meta.
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

import byol_a_ref  # noqa: E402
from make_golden import _load  # noqa: E402
from s3prl_amd.synth import named_config, synth_wavs, synth_weights  # noqa: E402

FP32_TOL = 1e-4
MAX_RESTATEMENT_ERR = 0.25 * FP32_TOL
MAX_BYTES = 256 * 1024

# name -> (config, weight seed, wav seed, lengths, dc, scale)
CASES = {
    "byol_a_tiny_eq": ("tiny_byol_a", 1201, 1301, [32000, 32000], 0.0, 1.0),
    # one utterance shorter than a window, one exactly k * stride, one k * stride + 1 (a third segment of one sample + zeros)
    "byol_a_tiny_pad": ("tiny_byol_a", 1201, 1302, [9000, 32000, 32001], 0.0, 1.0),
    "byol_a_tiny_overlap": ("tiny_byol_a_overlap", 1202, 1303, [24000, 16001, 8000], 0.05, 0.5),
    # window 4000, stride 1600: 26 frames -> 13 -> 6 -> 3, odd at two levels
    "byol_a_tiny_win025": ("tiny_byol_a_win025", 1203, 1304, [9000, 4800, 4801], 0.0, 1.0),
    "byol_a_2048_pseudo": ("byol_a_2048", 1204, 1305, [40000, 32001, 9000], 0.0, 1.0),
}


def _import_reference():
    import ref_shim

    ref_shim.import_reference(roots=("torchaudio", "omegaconf"))
    import importlib

    importlib.import_module("torchaudio.transforms")  # a placeholder MODULE, so that the expert's MelSpectrogram(...) call resolves


def rel(a, b):
    return float(np.linalg.norm(np.asarray(a, np.float64) - np.asarray(b, np.float64)) / np.linalg.norm(np.asarray(b, np.float64)))


def melspectrogram_fp32():
    """``torchaudio.transforms.MelSpectrogram(16000, 1024, 1024, 160, n_mels=64, f_min=60, f_max=7800)`` restated in float32 torch:
    wav (n,) -> (64, 1 + n // 160)."""
    import math

    import torch

    window = torch.hann_window(1024)
    all_freqs = torch.linspace(0, 16000 // 2, 513)
    m_min, m_max = 2595.0 * math.log10(1.0 + 60.0 / 700.0), 2595.0 * math.log10(1.0 + 7800.0 / 700.0)
    f_pts = 700.0 * (10 ** (torch.linspace(m_min, m_max, 64 + 2) / 2595.0) - 1.0)
    f_diff = f_pts[1:] - f_pts[:-1]
    slopes = f_pts.unsqueeze(0) - all_freqs.unsqueeze(1)
    fb = torch.max(torch.zeros(1), torch.min(-slopes[:, :-2] / f_diff[:-1], slopes[:, 2:] / f_diff[1:]))  # (513, 64)

    def to_melspec(wav):
        spec = torch.stft(wav, 1024, 160, 1024, window=window, center=True, pad_mode="reflect", normalized=False, onesided=True,
                          return_complex=True).abs().pow(2.0)  # (513, frames)
        return torch.matmul(spec.transpose(-1, -2), fb).transpose(-1, -2)

    return to_melspec


def reference_expert(cfg, weights, tmpdir):
    import torch

    _import_reference()
    from s3prl.upstream.byol_a.byol_a import AudioNTT2020
    from s3prl.upstream.byol_a.expert import UpstreamExpert
    from s3prl.upstream.byol_a.hubconf import DEFAULT_CONFIG_PATH

    d = cfg.conv_layers[0][0]
    model = AudioNTT2020(d=d)
    _load(model, weights)
    path = os.path.join(tmpdir, "byol_a.pth")
    torch.save(model.state_dict(), path)
    expert = UpstreamExpert(path, DEFAULT_CONFIG_PATH, d, window_secs=cfg.ba_window_secs, stride_secs=cfg.ba_stride_secs).eval()
    expert.to_melspec = melspectrogram_fp32()
    assert expert.get_downsample_rates("hidden_states") == cfg.conv_layers[0][2]
    return expert


def make_case(name: str):
    import torch

    cfg_name, wseed, xseed, lengths, dc, scale = CASES[name]
    cfg = named_config(cfg_name)
    weights = synth_weights(cfg, wseed)
    wavs = synth_wavs(lengths, xseed, dc=dc, scale=scale)
    with tempfile.TemporaryDirectory() as tmp:
        expert = reference_expert(cfg, weights, tmp)
        with torch.no_grad():
            out = expert([torch.from_numpy(w.copy()) for w in wavs])
    hs = out["hidden_states"]
    assert len(hs) == 1
    h = hs[0].numpy()
    d, window, stride = cfg.conv_layers[0]
    S = cfg.num_frames(max(lengths))
    assert h.shape == (len(lengths), S, d) and h.dtype == np.float32, (h.shape, h.dtype)
    mine = byol_a_ref.forward(cfg, weights, wavs)["state"]
    err = rel(mine, h)
    row_err = max(rel(mine[b, s], h[b, s]) for b in range(h.shape[0]) for s in range(S))
    assert err <= MAX_RESTATEMENT_ERR and row_err <= MAX_RESTATEMENT_ERR, (name, err, row_err)
    own = [cfg.num_frames(n) for n in lengths]
    pad_rows = [(b, s) for b in range(len(lengths)) for s in range(own[b], S)]
    assert all(np.abs(h[b, s]).max() > 0 for b, s in pad_rows)  # rows past an utterance's length are not zeros
    meta = dict(config=cfg_name, weight_seed=wseed, wav_seed=xseed, lengths=lengths, frames=own, segments=S, dc=dc, scale=scale,
                shape=list(h.shape), n_states=1, window=window, stride=stride,
                reference="s3prl 0.4.18 byol_a/expert.py (.eval()), torch CPU fp32; to_melspec replaced by a float32 torch.stft + "
                          "mel-bank restatement of torchaudio's MelSpectrogram (no torchaudio run)",
                zeros=float((h == 0).mean()), restatement_err=err, restatement_row_err=row_err)
    arrays = {"hs0": h, "norms": np.array([np.linalg.norm(h.astype(np.float64))]),
              "meta": np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)}
    os.makedirs(os.path.join(HERE, "byol_a"), exist_ok=True)
    path = os.path.join(HERE, "byol_a", f"{name}.npz")
    np.savez_compressed(path, **arrays)
    assert os.path.getsize(path) < MAX_BYTES, (path, os.path.getsize(path))
    print(f"{name}: shape {h.shape}, own segments {own}, zeros {meta['zeros']:.3f}, byol_a_ref float64 vs reference {err:.2e} whole / "
          f"{row_err:.2e} worst row -> {os.path.getsize(path) / 1e3:.0f} kB")


def make_hub_fixture():
    """names and signatures of the reference's byol_a hubconf, in reference_hub_vggish.json's layout"""
    _import_reference()
    import importlib

    mod = importlib.import_module("s3prl.upstream.byol_a.hubconf")
    sig = lambda f: [[k, v.kind.name, repr(v.default)] for k, v in inspect.signature(f).parameters.items()]  # noqa: E731
    res = {"byol_a": [[n, sig(f)] for n, f in vars(mod).items()
                      if inspect.isfunction(f) and not n.startswith("_") and f.__module__ == mod.__name__]}
    expert = importlib.import_module("s3prl.upstream.byol_a.expert").UpstreamExpert
    os.makedirs(os.path.join(HERE, "byol_a"), exist_ok=True)
    with open(os.path.join(HERE, "byol_a", "reference_hub_byol_a.json"), "w") as f:
        json.dump(dict(reference="s3prl 0.4.18: s3prl.upstream.byol_a.hubconf", hubconfs=res, expert_init=sig(expert.__init__)), f,
                  indent=1, sort_keys=True)


if __name__ == "__main__":
    names = sys.argv[1:] or list(CASES) + ["hub"]
    for n in names:
        make_hub_fixture() if n == "hub" else make_case(n)
