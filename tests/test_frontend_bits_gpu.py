"""The four spectral front ends on the MI355X, bit for bit against calls recorded on the commit before csrc/spectral.hip replaced
their private copies of the fold, the mel kernel, the CMVN and the reflect padding (tests/golden/make_recorded_frontends.py wrote
tests/golden/frontends/*.npz from the functions below): fbank through s3enc_fbank_forward_ex, the log-mel through
s3enc_logmel_forward, both forms of s3enc_op_melspec1024, s3enc_op_melspec400, and a tiny VGGish handle's log-mel tap and output.
Every fixture also holds the first 8 samples of each seeded input, so that a drift of the generator is told apart from one of a kernel."""

import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = os.path.join(ROOT, "tests", "golden", "frontends")


def _torch():
    import torch

    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def _dev(w, misaligned=False):
    """the waveform on the device; misaligned: at a pointer 4 bytes off a 16-byte line"""
    torch = _torch()
    if not misaligned:
        return torch.from_numpy(w).cuda()
    buf = torch.zeros(len(w) + 8, device="cuda")
    buf[1:1 + len(w)] = torch.from_numpy(w).cuda()
    out = buf[1:1 + len(w)]
    assert out.data_ptr() % 16 == 4
    return out


def _heads(wavs):
    return np.stack([w[:8] for w in wavs])


# ---- fbank: s3enc_fbank_forward_ex --------------------------------------------------------------------------------------------
FBANK_LENGTHS = [560, 879, 2000]  # two frames (the least the unbiased CMVN allows), three and a 159-sample remainder, eleven


def _fbank(nmel, window, order, cmvn, misaligned=None):
    from s3prl_amd import _lib
    from s3prl_amd.synth import synth_wavs

    torch = _torch()
    lib = _lib.load()
    c = _lib.S3FbankConfig()
    c.sample_rate, c.num_mel_bins, c.frame_length_ms, c.frame_shift_ms, c.preemphasis = 16000, nmel, 25.0, 10.0, 0.97
    c.delta_order, c.delta_win_length, c.use_cmvn, c.cmvn_eps = order, 5, int(cmvn), 1e-10
    wavs = synth_wavs(FBANK_LENGTHS, 4200 + nmel + window)
    dev = [_dev(w, misaligned == b) for b, w in enumerate(wavs)]
    B, T = len(wavs), max((n - 400) // 160 + 1 for n in FBANK_LENGTHS)
    out = torch.full((B, T, nmel * (order + 1)), float("nan"), device="cuda")
    ptrs = (C.c_void_p * B)(*[w.data_ptr() for w in dev])
    _lib.check(lib.s3enc_fbank_forward_ex(C.byref(c), window, ptrs, (C.c_int64 * B)(*FBANK_LENGTHS), B, C.c_void_p(out.data_ptr()), T,
                                          0, None), "s3enc_fbank_forward_ex")
    torch.cuda.synchronize()
    return {"heads": _heads(wavs), "out": out.cpu().numpy()}


# ---- log-mel: s3enc_logmel_frame_counts, s3enc_logmel_forward ---------------------------------------------------------------
LOGMEL_LENGTHS = [1000, 900, 300]  # 900 ends within 200 samples of max_len (zeros and reflection mixed); 300 is a frame count of 2


def _logmel(n_mels, cmvn, n_max=0):
    from s3prl_amd import _lib
    from s3prl_amd.synth import synth_wavs

    torch = _torch()
    lib = _lib.load()
    wavs = synth_wavs(LOGMEL_LENGTHS, 4300)
    dev = [_dev(w) for w in wavs]
    B, T = len(wavs), 1 + (n_max or max(LOGMEL_LENGTHS)) // 160
    lens = (C.c_int64 * B)(*LOGMEL_LENGTHS)
    counts = (C.c_int32 * B)()
    _lib.check(lib.s3enc_logmel_frame_counts(lens, B, n_max, counts), "s3enc_logmel_frame_counts")
    out = torch.full((B, T, n_mels), float("nan"), device="cuda")
    ptrs = (C.c_void_p * B)(*[w.data_ptr() for w in dev])
    _lib.check(lib.s3enc_logmel_forward(ptrs, lens, B, n_max, n_mels, -25.0, int(cmvn), counts, C.c_void_p(out.data_ptr()), 0, None),
               "s3enc_logmel_forward")
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    assert min(counts) == 2
    if cmvn:
        for b, n in enumerate(counts):
            assert not out[b, n:].view(np.uint32).any(), "rows behind the frame count must be exact zeros"
    return {"heads": _heads(wavs), "counts": np.array(list(counts), np.int32), "out": out}


# ---- melspec: s3enc_op_melspec1024 (both forms), s3enc_op_melspec400 ---------------------------------------------------------
def _melspec(entry, L, fft=1):
    from s3prl_amd import _lib

    torch = _torch()
    lib = _lib.load()
    segs = np.random.default_rng(4400 + L).standard_normal((3, L)).astype(np.float32)
    T = 1 + L // 160
    x = torch.from_numpy(segs).cuda()
    out = torch.full((3, T, 64), float("nan"), device="cuda")
    pw = torch.full((3, T, 513), float("nan"), device="cuda")
    _lib.check(lib.s3enc_set_tuning(b"melspec_fft", fft), "s3enc_set_tuning")
    try:
        _lib.check(getattr(lib, entry)(C.c_void_p(x.data_ptr()), 3, L, C.c_void_p(out.data_ptr()), C.c_void_p(pw.data_ptr()), None), entry)
        torch.cuda.synchronize()
    finally:
        _lib.check(lib.s3enc_set_tuning(b"melspec_fft", 1), "s3enc_set_tuning")
    return {"heads": _heads(segs), "logmel": out.cpu().numpy(), "power": pw.cpu().numpy()}


# ---- VGGish: the first tiny configuration, the five lengths of test_vggish_gpu.py's per-example test ---------------------------
def _vggish():
    from s3prl_amd.encoder import HipEncoder
    from s3prl_amd.synth import named_config, synth_wavs, synth_weights

    torch = _torch()
    cfg = named_config("tiny_vggish")
    lengths = [max(n, cfg.vg_min_samples) for n in [9000, 2800, 5599, 5600, 12000]]
    assert len({cfg.num_frames(n) for n in lengths}) >= 2
    wavs = synth_wavs(lengths, 77 + len(lengths))
    enc = HipEncoder(cfg, synth_weights(cfg, 31), dtype="fp32")
    try:
        out = enc.forward([_dev(w, b == 2) for b, w in enumerate(wavs)])
        torch.cuda.synchronize()
        return {"heads": _heads(wavs), "logmel": enc.debug_tap("logmel").copy(), "out": out.cpu().numpy()}
    finally:
        enc.close()


CASES = {
    "fbank80_povey_delta2_cmvn": lambda: _fbank(80, 0, 2, True, misaligned=1),
    "fbank80_hamming_cmvn": lambda: _fbank(80, 1, 0, True),  # APC's
    "fbank128_raw": lambda: _fbank(128, 0, 0, False),        # MAE-AST's
    "logmel80_cmvn": lambda: _logmel(80, True),
    "logmel80_raw": lambda: _logmel(80, False),
    "logmel16_cmvn": lambda: _logmel(16, True),
    "logmel16_raw": lambda: _logmel(16, False),
    "logmel80_cmvn_nmax1500": lambda: _logmel(80, True, n_max=1500),
    "melspec1024_gemm_1120": lambda: _melspec("s3enc_op_melspec1024", 1120, fft=0),
    "melspec1024_gemm_2560": lambda: _melspec("s3enc_op_melspec1024", 2560, fft=0),
    "melspec1024_fft_1120": lambda: _melspec("s3enc_op_melspec1024", 1120),
    "melspec400_520": lambda: _melspec("s3enc_op_melspec400", 520),
    "melspec400_2560": lambda: _melspec("s3enc_op_melspec400", 2560),
    "vggish_tiny": _vggish,
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_front_end_keeps_its_bits(name):
    z = np.load(os.path.join(FIXTURES, name + ".npz"))
    got = CASES[name]()
    assert sorted(list(got) + ["parent_commit"]) == sorted(z.files)
    assert np.array_equal(got["heads"], z["heads"]), "the seeded inputs are not the recorded ones: the generator drifted, not a kernel"
    for key in sorted(got):
        if key == "heads":
            continue
        g = np.ascontiguousarray(got[key])
        assert g.shape == z[key].shape and z[key].dtype == (np.uint32 if g.dtype == np.float32 else g.dtype), (name, key)
        same = np.array_equal(g.view(np.uint32) if g.dtype == np.float32 else g, z[key])
        assert same, f"{name}: {key} changed its bits against commit {str(z['parent_commit'])}"
