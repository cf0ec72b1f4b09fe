"""The batch-wide kaldi log-mel pass (csrc/fbank.hip: launch_fbank_batch) through its op entry s3enc_op_fbank_batch: one overlapping-row
GEMM over a padded batch, one power -> mel -> log launch, one CMVN launch with per-utterance counts.

The property held here is bit identity: every valid row of utterance b equals s3enc_fbank_forward_ex (hamming, CMVN, no deltas) of
that utterance ALONE, bit for bit, and every row behind it is exactly 0 — whatever stands behind the utterance's samples in the padded
batch (the slab is filled with NaN there), whatever the order of the utterances, the padded length, or the chunking of the spectrum
workspace.  Every check runs at B = 1 and B = 3.  Frame counts: 2 (the fewest the CMVN allows), an odd and an even count, and one
below, at and above the row-tile heights of the fp32 tile GEMM (gemmt.hip: 64 tm rows, tm = 1..4; M < 64 takes gemm.hip's kernel).

Against float64 the bound is the one tests/test_fbank_gpu.py holds the 80 CMVN'd log-mel columns to (5e-4 per element, its
``test_fbank_hub_entry_matches_oracle``), with that file's oracle module and waveform helper."""

import ctypes as C

import numpy as np
import pytest

import apc_ref
from test_fbank_gpu import F as FO, _wavs

pytestmark = pytest.mark.gpu

LOGMEL_ELEMENT_TOL = 5e-4  # tests/test_fbank_gpu.py: `np.abs(got[b, :T, :80] - ref[b, :T, :80]).max() < 5e-4`
FRAMES = (2, 23, 24, 63, 64, 65, 127, 128, 129, 192, 256, 257)


def _n(frames, extra=0):
    """samples of an utterance with `frames` analysis windows and `extra` < 160 samples behind the last one"""
    return 400 + 160 * (frames - 1) + extra


def _lengths(F, B):
    return [_n(F, 37)] if B == 1 else [_n(max(2, F // 2), 159), _n(F, 37), _n(max(2, F - 1), 1)]


@pytest.fixture(scope="module")
def gpu():
    import torch

    from s3prl_amd import _lib

    assert torch.cuda.is_available(), "these tests need the MI355X"
    lib = _lib.load()
    cfg = _lib.S3FbankConfig(16000, 80, 25.0, 10.0, 0.97, 0, 5, 1, 1e-10)
    dev, stream = torch.cuda.current_device(), lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
    alone_cache = {}

    def wav(n, seed):
        return _wavs([n], seed=seed)[0]

    def alone(n, seed):
        """s3enc_fbank_forward_ex on the utterance alone: (F, 80)"""
        if (n, seed) not in alone_cache:
            w = wav(n, seed).cuda()
            T = FO.num_frames(n)
            out = torch.full((1, T, 80), np.nan, dtype=torch.float32, device="cuda")
            rc = lib.s3enc_fbank_forward_ex(C.byref(cfg), 1, (C.c_void_p * 1)(w.data_ptr()), (C.c_int64 * 1)(n), 1, C.c_void_p(out.data_ptr()),
                                            T, dev, stream())
            _lib.check(rc, "s3enc_fbank_forward_ex")
            torch.cuda.synchronize()
            alone_cache[(n, seed)] = out[0].cpu().numpy()
        return alone_cache[(n, seed)]

    def batch(lengths, seeds, n_max=0, cap=0, config=cfg, stride=None, check=True):
        """the op on a (B, stride) slab whose samples behind every utterance are NaN: (B, Fmax, 80), or the return code"""
        B, longest = len(lengths), max(max(lengths), n_max)
        stride = (longest + 3) // 4 * 4 if stride is None else stride
        slab = torch.full((B, stride), np.nan, dtype=torch.float32)
        for b, (n, s) in enumerate(zip(lengths, seeds)):
            slab[b, :n] = wav(n, s)
        slab = slab.cuda()
        Fmax = FO.num_frames(longest)
        out = torch.full((B, max(Fmax, 1), 80), np.nan, dtype=torch.float32, device="cuda")
        rc = lib.s3enc_op_fbank_batch(C.byref(config), 1, C.c_void_p(slab.data_ptr()), stride, (C.c_int64 * B)(*lengths), B, n_max,
                                      C.c_void_p(out.data_ptr()), cap, dev, stream())
        if not check:
            return rc, lib.s3enc_last_error().decode()
        _lib.check(rc, "s3enc_op_fbank_batch")
        torch.cuda.synchronize()
        return out.cpu().numpy()

    return alone, batch, _lib


def _assert_rows(got, lengths, seeds, alone):
    for b, (n, s) in enumerate(zip(lengths, seeds)):
        ref = alone(n, s)
        Fb = ref.shape[0]
        assert Fb == FO.num_frames(n) and np.isfinite(ref).all()
        assert np.array_equal(got[b, :Fb].view(np.int32), ref.view(np.int32)), \
            f"utterance {b} ({Fb} frames): {np.count_nonzero(got[b, :Fb] != ref)} values differ from launch_fbank alone, max {np.abs(got[b, :Fb] - ref).max():.2e}"
        assert np.array_equal(got[b, Fb:].view(np.int32), np.zeros_like(got[b, Fb:]).view(np.int32)), f"utterance {b}: rows behind its {Fb} frames must be +0"


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("F", FRAMES)
def test_every_valid_row_equals_the_utterance_alone_and_the_rest_is_zero(F, B, gpu):
    alone, batch, _ = gpu
    lengths, seeds = _lengths(F, B), list(range(11, 11 + B))
    got = batch(lengths, seeds)
    assert got.shape == (B, F, 80)
    _assert_rows(got, lengths, seeds, alone)


@pytest.mark.parametrize("B", [1, 3])
def test_order_and_padded_length_do_not_matter(B, gpu):
    alone, batch, _ = gpu
    lengths, seeds = _lengths(65, B), list(range(21, 21 + B))
    base = batch(lengths, seeds)
    perm = [0] if B == 1 else [2, 0, 1]
    got = batch([lengths[i] for i in perm], [seeds[i] for i in perm])
    for j, i in enumerate(perm):
        assert np.array_equal(got[j].view(np.int32), base[i].view(np.int32)), f"utterance {i} moved to slot {j}"
    n_max = max(lengths) + 160 * 70 + 3  # 70 more frames: another row tile of the GEMM
    wide = batch(lengths, seeds, n_max=n_max)
    assert wide.shape[1] == FO.num_frames(n_max) == 135
    _assert_rows(wide, lengths, seeds, alone)
    assert np.array_equal(wide[:, :65].view(np.int32), base.view(np.int32))
    if B == 1:  # a row pitch wider than the padded length
        assert np.array_equal(batch(lengths, seeds, stride=max(lengths) + 64 + (-max(lengths)) % 4).view(np.int32), base.view(np.int32))


@pytest.mark.parametrize("B", [1, 3])
def test_chunks_of_whole_utterances_give_the_same_bits(B, gpu):
    """a spectrum cap below the batch: chunks of 1 and of 2 utterances, and a cap below ONE utterance (a chunk of its own)"""
    alone, batch, _ = gpu
    lengths, seeds = _lengths(129, B), list(range(31, 31 + B))
    base = batch(lengths, seeds)
    per_utt = 129 * 2 * 257 * 4
    for cap in (per_utt, 2 * per_utt + 5, 1000):
        assert np.array_equal(batch(lengths, seeds, cap=cap).view(np.int32), base.view(np.int32)), cap
    _assert_rows(base, lengths, seeds, alone)


@pytest.mark.parametrize("B", [1, 3])
def test_against_the_float64_front_end(B, gpu):
    _, batch, _ = gpu
    lengths, seeds = _lengths(128, B), list(range(41, 41 + B))
    got = batch(lengths, seeds)
    worst = 0.0
    for b, (n, s) in enumerate(zip(lengths, seeds)):
        ref = apc_ref.cmvn(apc_ref.kaldi_fbank(_wavs([n], seed=s)[0].numpy().astype(np.float64), 80, 25.0, 10.0, "hamming"))
        worst = max(worst, np.abs(got[b, :ref.shape[0]] - ref).max())
    print(f"B = {B}: max |batched - float64| {worst:.2e} (< {LOGMEL_ELEMENT_TOL:.0e})")
    assert worst < LOGMEL_ELEMENT_TOL


def test_refusals(gpu):
    _, batch, _lib = gpu
    deltas = _lib.S3FbankConfig(16000, 80, 25.0, 10.0, 0.97, 2, 5, 1, 1e-10)
    no_cmvn = _lib.S3FbankConfig(16000, 80, 25.0, 10.0, 0.97, 0, 5, 0, 1e-10)
    for kw, what in ((dict(config=deltas), "delta_order must be 0"), (dict(config=no_cmvn), "use_cmvn must be 1"),
                     (dict(n_max=1000), "n_max is smaller than the longest utterance"), (dict(stride=4002), "row_stride a multiple of 4"),
                     (dict(cap=-1), "spec_cap_bytes must not be negative")):
        rc, msg = batch([4000, 2000], [1, 2], check=False, **kw)
        assert rc != 0 and what in msg, (kw, msg)
    rc, msg = batch([4000, 399], [1, 2], check=False)
    assert rc != 0 and "shorter than one analysis window" in msg
