"""BYOL-S's front end on the MI355X through the C ABI: s3enc_op_melspec400 — the hann(400)-in-1024 window table of melspec.hip's FFT
kernel, un-normalised — against float64 numpy (tests/byol_s_ref.py) at test_melspec_gpu.py's bound; s3enc_op_melspec1024 unchanged,
bit for bit, against a call recorded on the commit before the window table went in; and the whole-batch statistics of a forward —
the two debug-tap values against float64 statistics of the GPU's own log-mel tap, and identical in their bits from run to run."""

import ctypes as C
import os

import numpy as np
import pytest

import byol_s_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OP_TOL = 2e-5  # the project's op bound
LENGTHS = [520, 1120, 4000, 16000]
RECORDED = os.path.join(ROOT, "tests", "golden", "byol_s", "melspec1024_recorded.npz")


def _torch():
    import torch

    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def _op(segs, entry="s3enc_op_melspec400", power=False):
    from s3prl_amd import _lib

    torch = _torch()
    lib = _lib.load()
    nseg, L = segs.shape
    T = 1 + L // 160
    x = torch.from_numpy(np.ascontiguousarray(segs, dtype=np.float32)).cuda()
    out = torch.full((nseg, T, 64), float("nan"), device="cuda")
    pw = torch.full((nseg, T, 513), float("nan"), device="cuda") if power else None
    _lib.check(getattr(lib, entry)(C.c_void_p(x.data_ptr()), nseg, L, C.c_void_p(out.data_ptr()),
                                   C.c_void_p(pw.data_ptr()) if power else None, None), entry)
    torch.cuda.synchronize()
    return out.cpu().numpy(), (pw.cpu().numpy() if power else None)


def _rel(got, ref):
    return float(np.linalg.norm(got.astype(np.float64) - ref) / np.linalg.norm(ref))


def recorded_inputs():
    """the segments of the recorded s3enc_op_melspec1024 call: seeded, (3, 2560)"""
    return np.random.default_rng(4100).standard_normal((3, 2560)).astype(np.float32)


@pytest.mark.parametrize("L", LENGTHS)
def test_the_400_window_logmel_against_float64(L):
    rng = np.random.default_rng(200 + L)
    segs = rng.standard_normal((3, L)).astype(np.float32)
    lm64 = np.stack([R.logmel(s) for s in segs])
    lm, pw = _op(segs, power=True)
    assert lm.shape == lm64.shape == (3, 1 + L // 160, 64) and np.isfinite(lm).all()
    frames = np.linalg.norm(lm.astype(np.float64) - lm64, axis=-1) / np.linalg.norm(lm64, axis=-1)
    print(f"melspec400 logmel L={L}: whole {_rel(lm, lm64):.2e}, worst frame {frames.max():.2e}")
    assert _rel(lm, lm64) < OP_TOL and frames.max() < OP_TOL
    # the power spectrum per frame, against the same window in float64
    x = np.stack([np.pad(s.astype(np.float64), 512, mode="reflect") for s in segs])
    idx = np.arange(1 + L // 160)[:, None] * 160 + np.arange(1024)[None, :]
    X = np.fft.rfft(x[:, idx] * R.hann400_in_1024(), axis=-1)
    pw64 = X.real ** 2 + X.imag ** 2
    perr = np.linalg.norm(pw - pw64, axis=-1) / np.linalg.norm(pw64, axis=-1)
    assert perr.max() < OP_TOL, (L, perr.max())


def test_an_all_zero_window_is_one_constant():
    lm, _ = _op(np.zeros((2, 4000), np.float32))
    assert len(np.unique(lm.view(np.uint32))) == 1 and abs(float(lm[0, 0, 0]) / np.log(R.EPS) - 1.0) < 1e-6


def test_the_1024_entry_keeps_its_bits():
    """the recorded call: s3enc_op_melspec1024 on the seeded segments, as the commit before BYOL-S computed it"""
    z = np.load(RECORDED)
    segs = recorded_inputs()
    assert np.array_equal(z["segments_head"], segs[:, :8])
    lm, pw = _op(segs, entry="s3enc_op_melspec1024", power=True)
    assert np.array_equal(lm.view(np.uint32), z["logmel"].view(np.uint32)), "s3enc_op_melspec1024's log-mel changed its bits"
    assert np.array_equal(pw.view(np.uint32), z["power"].view(np.uint32)), "s3enc_op_melspec1024's power spectrum changed its bits"


def test_refusals_by_message():
    from s3prl_amd import _lib

    for L in (512, 400):
        with pytest.raises(_lib.S3EncError, match="s3enc_op_melspec400: a segment of at most 512 samples cannot be reflect-padded"):
            _op(np.zeros((1, L), np.float32))
    _op(np.zeros((1, 513), np.float32))  # the 8-frame rule is BYOL-A's network's, not this front end's


@pytest.mark.parametrize("name", ["byol_s/byol_s_tiny_win025", "byol_s/byol_s_tiny_pad"])
def test_the_statistics_of_a_forward(name, golden_loader):
    """the two debug-tap statistics against float64 statistics of the GPU's own log-mel tap to 1e-6 relative (the accumulation is
    float64, rounded once to fp32, then divided by N in fp32), and identical in their bits across three runs; the log-mel tap itself
    against the float64 restatement (windows that start in front of the utterance and end behind it included)"""
    from s3prl_amd.encoder import HipEncoder

    torch = _torch()
    meta, cfg, weights, wavs, _, _ = golden_loader(name)
    enc = HipEncoder(cfg, weights)
    try:
        runs = []
        for _ in range(3):
            enc.forward([torch.from_numpy(w).cuda() for w in wavs])
            torch.cuda.synchronize()
            runs.append((enc.debug_tap("stats").copy(), enc.debug_tap("logmel").copy()))
    finally:
        enc.close()
    stats, lm = runs[0]
    N = meta["N"]
    T = 1 + meta["window"] // 160
    assert stats.shape == (2,) and lm.shape == (N * T * 64,)
    x = lm.astype(np.float64)
    want = np.array([np.float32(x.mean()) / np.float32(N), np.float32(x.std(ddof=1)) / np.float32(N)], np.float64)
    err = np.abs(stats.astype(np.float64) - want) / np.abs(want)
    print(f"{name}: stats {stats}, float64 of the tap {want}, relative difference {err}, the reference's {meta['stats']}")
    assert err.max() < 1e-6
    assert np.abs(stats - np.array(meta["stats"])).max() / np.abs(meta["stats"]).min() < 1e-4
    for s, l in runs[1:]:
        assert np.array_equal(s.view(np.uint32), stats.view(np.uint32)) and np.array_equal(l.view(np.uint32), lm.view(np.uint32))
    ref = R.forward(cfg, weights, wavs)["logmel"].reshape(N, T, 64)
    rows = np.linalg.norm(lm.reshape(N, T, 64) - ref, axis=(1, 2)) / np.linalg.norm(ref, axis=(1, 2))
    assert rows.max() < OP_TOL, rows.max()
