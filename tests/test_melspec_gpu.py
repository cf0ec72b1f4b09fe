"""s3enc_op_melspec1024 on the MI355X through the C ABI: BYOL-A's front end (per-segment reflect padding, 1024-point periodic-hann
STFT, |X|^2, 64 HTK mel triangles, log, the fixed affine) against float64 numpy (tests/byol_a_ref.py) — the power spectrum per frame,
edge frames (which read reflected samples) scored apart from interior ones; impulses; the bits of a frame as a function of its own
samples only; the all-zero segment; the FFT form against the GEMM form (tuning key melspec_fft); the refusals."""

import ctypes as C

import numpy as np
import pytest

import byol_a_ref as R

pytestmark = pytest.mark.gpu

OP_TOL = 2e-5  # the project's op bound
LENGTHS = [1120, 2560, 4000, 16000]


def _torch():
    import torch

    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def _op(segs, power=False):
    """(nseg, L) float32 numpy -> (logmel (nseg, T, 64), power (nseg, T, 513) or None) as numpy"""
    from s3prl_amd import _lib

    torch = _torch()
    lib = _lib.load()
    nseg, L = segs.shape
    T = 1 + L // 160
    x = torch.from_numpy(np.ascontiguousarray(segs, dtype=np.float32)).cuda()
    out = torch.full((nseg, T, 64), float("nan"), device="cuda")
    pw = torch.full((nseg, T, 513), float("nan"), device="cuda") if power else None
    _lib.check(lib.s3enc_op_melspec1024(C.c_void_p(x.data_ptr()), nseg, L, C.c_void_p(out.data_ptr()),
                                        C.c_void_p(pw.data_ptr()) if power else None, None), "s3enc_op_melspec1024")
    torch.cuda.synchronize()
    return out.cpu().numpy(), (pw.cpu().numpy() if power else None)


def _frame_err(got, ref):
    """relative error of every frame (last axis) against float64"""
    d = np.linalg.norm(got.astype(np.float64) - ref, axis=-1)
    return d / np.linalg.norm(ref, axis=-1)


def _rel(got, ref):
    return float(np.linalg.norm(got.astype(np.float64) - ref) / np.linalg.norm(ref))


@pytest.fixture(scope="module")
def noise():
    """unit-variance noise segments per length and their float64 yardsticks, computed once"""
    out = {}
    for L in LENGTHS:
        rng = np.random.default_rng(100 + L)
        segs = rng.standard_normal((3, L)).astype(np.float32)
        out[L] = (segs, np.stack([R.power_spectrum(s) for s in segs]), np.stack([R.logmel(s) for s in segs]))
    return out


@pytest.mark.parametrize("L", LENGTHS)
def test_power_spectrum_per_frame(noise, L):
    segs, pw64, _ = noise[L]
    _, pw = _op(segs, power=True)
    assert pw.shape == pw64.shape == (3, 1 + L // 160, 513)
    err = _frame_err(pw, pw64)
    edge = np.concatenate([err[:, :4].ravel(), err[:, -4:].ravel()])
    inner = err[:, 4:-4].ravel() if err.shape[1] > 8 else np.zeros(1)
    print(f"melspec power L={L}: worst edge frame {edge.max():.2e}, worst interior frame {inner.max():.2e}, whole {_rel(pw, pw64):.2e}")
    assert edge.max() < OP_TOL and inner.max() < OP_TOL


@pytest.mark.parametrize("L", LENGTHS)
def test_logmel_against_float64(noise, L):
    segs, _, lm64 = noise[L]
    lm, _ = _op(segs)
    err = _rel(lm, lm64)
    print(f"melspec logmel L={L}: whole {err:.2e}, worst frame {_frame_err(lm, lm64).max():.2e}")
    assert np.isfinite(lm).all() and err < OP_TOL


def test_the_float32_stft_restatement_meets_the_bound_on_these_inputs(noise):
    """what the bound asks is within reach of float32: torch.stft in float32 + the float32 mel bank on the same inputs"""
    torch = _torch()
    fb = torch.from_numpy(R.mel_bank(np.float32))
    for L in LENGTHS:
        segs, _, lm64 = noise[L]
        spec = torch.stft(torch.from_numpy(segs), 1024, 160, 1024, window=torch.hann_window(1024), center=True, pad_mode="reflect",
                          return_complex=True).abs().pow(2.0).transpose(1, 2)
        lm = ((torch.matmul(spec, fb) + torch.finfo(torch.float).eps).log() - R.MEAN) / R.STD
        assert _rel(lm.numpy(), lm64) < OP_TOL, L


@pytest.mark.parametrize("offset", [700, 1023, 1024, 1500, 2047])
def test_an_impulse_gives_a_flat_spectrum(offset):
    L = 4000
    seg = np.zeros((1, L), np.float32)
    seg[0, offset] = 3.0
    _, pw = _op(seg, power=True)
    win = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(1024) / 1024)
    checked = 0
    for t in range(1 + L // 160):
        i = offset - (160 * t - 512)  # the impulse's place in frame t
        if 160 * t - 512 < 0 or 160 * t + 512 > L or not 0 <= i < 1024 or win[i] < 0.1:
            continue  # an edge frame also holds the impulse's reflection; a window value near zero leaves rounding noise only
        want = (3.0 * win[i]) ** 2
        assert np.abs(pw[0, t] / want - 1.0).max() < OP_TOL, (offset, t, np.abs(pw[0, t] / want - 1.0).max())
        checked += 1
    assert checked >= 3


def test_a_frames_bits_depend_on_its_samples_only(noise):
    segs, _, _ = noise[2560]
    L = 2560
    lm3, pw3 = _op(segs, power=True)
    for i in range(3):  # another nseg
        lm1, pw1 = _op(segs[i:i + 1], power=True)
        assert np.array_equal(lm1[0], lm3[i]) and np.array_equal(pw1[0], pw3[i]), i
    lmp, pwp = _op(segs[[2, 0, 1]], power=True)  # another place in the table
    assert np.array_equal(lmp[1], lm3[0]) and np.array_equal(pwp[0], pw3[2])
    # the same 1024 samples as frame t of one segment and frame t + 1 of another (interior frames: no reflected sample in either)
    shifted = np.zeros((1, L), np.float32)
    shifted[0, 160:] = segs[0, :-160]
    lms, pws = _op(shifted, power=True)
    inner = [t for t in range(1 + L // 160 - 1) if 160 * t - 512 >= 0 and 160 * (t + 1) + 512 <= L]
    assert len(inner) >= 4
    for t in inner:
        assert np.array_equal(pws[0, t + 1], pw3[0, t]) and np.array_equal(lms[0, t + 1], lm3[0, t]), t


def test_an_all_zero_segment_is_one_constant():
    segs = np.zeros((2, 2560), np.float32)
    segs[1] = np.random.default_rng(5).standard_normal(2560)
    lm, pw = _op(segs, power=True)
    assert not pw[0].any()
    assert len(np.unique(lm[0].view(np.uint32))) == 1, "the values of an all-zero segment differ in their bits"
    want = (np.log(R.EPS) - R.MEAN) / R.STD
    assert abs(float(lm[0, 0, 0]) / want - 1.0) < 1e-6


def test_the_fft_form_and_the_gemm_form_agree(noise):
    from s3prl_amd import _lib

    lib = _lib.load()
    for L in (1120, 4000):
        segs, pw64, lm64 = noise[L]
        lm_fft, pw_fft = _op(segs, power=True)
        _lib.check(lib.s3enc_set_tuning(b"melspec_fft", 0), "s3enc_set_tuning")
        try:
            lm_gemm, pw_gemm = _op(segs, power=True)
        finally:
            _lib.check(lib.s3enc_set_tuning(b"melspec_fft", 1), "s3enc_set_tuning")
        print(f"melspec forms L={L}: logmel fft vs gemm {_rel(lm_fft, lm_gemm.astype(np.float64)):.2e}, gemm vs float64 {_rel(lm_gemm, lm64):.2e}, "
              f"power fft vs gemm {_rel(pw_fft, pw_gemm.astype(np.float64)):.2e}")
        assert _rel(lm_fft, lm_gemm.astype(np.float64)) < OP_TOL and _rel(pw_fft, pw_gemm.astype(np.float64)) < OP_TOL
        assert _rel(lm_gemm, lm64) < OP_TOL and _frame_err(pw_gemm, pw64).max() < OP_TOL
    assert lib.s3enc_set_tuning(b"melspec_fft", 2) != 0 and b"0..1" in lib.s3enc_last_error()


def test_refusals_by_message():
    from s3prl_amd import _lib

    for L, match in ((512, "cannot be reflect-padded"), (400, "cannot be reflect-padded"), (513, "fewer than 8 frames"),
                     (1119, "fewer than 8 frames")):
        with pytest.raises(_lib.S3EncError, match=match):
            _op(np.zeros((1, L), np.float32))
