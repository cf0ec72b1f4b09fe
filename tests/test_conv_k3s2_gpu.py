"""s3enc_op_conv_k3s2 on the MI355X, every call through the C ABI: convf22.hip — Conv1d(C, C, 3, stride 2) in the two-output form —
driven directly at the smallest widths at which each of its mechanisms exists (C = 32: two K steps per phase; 64; 96: one ragged
n-tile; 160: two n-tiles, the second ragged; 512 once), against float64 row by row, and bit for bit against itself where its
design says so: a row's bits depend on its three frames and the weights only, so they are the same at every length M (the clamp
to frame 2M is invisible), behind any even number of junk rows, at any place in any batch and on any grid; frame 2M + 1 is never
read; nothing but rows [0, M) is written; rows at or above row_limit are +0.0.  The implicit GEMM that conv_f22 = 0 falls back to
(and conv5-6's k = 2) gets the same per-row sweep through s3enc_op_gemm, and a handle's conv2 tap is this op applied to its
conv1 tap.

The per-row rule is test_conv2d_res_gpu.py's: a row's relative error over its C values (the row norm floored at 1e-3) stays below
max(OP_TOL, 8 x the error of torch's own fp32 conv1d + GELU on the same rows), and no element is off by more than
50 OP_TOL (1 + |ref|).  tests/test_conv_k3s2_ref_cpu.py shows what the rule catches."""

import ctypes as C

import numpy as np
import pytest

import conv_k3s2_ref as R

pytestmark = pytest.mark.gpu

OP_TOL = R.OP_TOL
GUARD = 64     # NaN floats in front of and behind `out`: nothing outside the rows may be written
SENTINEL = 2   # NaN rows behind every utterance's M rows (o_bs = (M + 2) C)
EDGES = [1, 2, 3, 63, 64, 65, 127, 128, 129, 130, 255, 256, 257]


def _torch():
    import torch

    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _dev(a, dtype=np.float32):
    return None if a is None else _torch().from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def _call(x, x_bs, w, bias, limit, B, M, Cc, act, out, o_bs):
    from s3prl_amd import _lib

    wh = np.ascontiguousarray(w, dtype=np.float32)
    _lib.check(_lib.load().s3enc_op_conv_k3s2(_ptr(x), x_bs, C.c_void_p(wh.ctypes.data), _ptr(bias), _ptr(limit), B, M, Cc, act, _ptr(out),
                                              o_bs, None), "s3enc_op_conv_k3s2")
    _torch().cuda.synchronize()


def _run(x, w, bias, M, act=1, limit=None, B=None, x_bs=None):
    """The op on x (device, (B, L, C) or flat with x_bs given) into NaN: o_bs = (M + SENTINEL) C between GUARD floats.  Asserts
    that the guards and the sentinel rows are still NaN and returns rows [0, M) of every utterance, (B, M, C)."""
    torch = _torch()
    Cc = w.shape[0]
    B = x.shape[0] if B is None else B
    x_bs = x.shape[1] * Cc if x_bs is None else x_bs
    rows = M + SENTINEL
    buf = torch.full((GUARD + B * rows * Cc + GUARD,), float("nan"), device="cuda")
    body = buf[GUARD:GUARD + B * rows * Cc].view(B, rows, Cc)
    _call(x, x_bs, w, bias, limit, B, M, Cc, act, body, rows * Cc)
    assert torch.isnan(buf[:GUARD]).all() and torch.isnan(buf[-GUARD:]).all(), ("a guard float of out was written", M, B)
    assert torch.isnan(body[:, M:]).all(), ("a row behind the M rows of an utterance was written", M, B)
    return body[:, :M].clone()


def _theirs(x, w, bias, M, act, k=3):
    """torch.nn.functional.conv1d + GELU in CPU fp32 on the same operands, (B, M, C)"""
    torch = _torch()
    y = torch.nn.functional.conv1d(torch.from_numpy(x[:, :2 * (M - 1) + k]).transpose(1, 2), torch.from_numpy(w),
                                   None if bias is None else torch.from_numpy(bias), stride=2).transpose(1, 2)
    return torch.nn.functional.gelu(y) if act else y


def _check(got, x, w, bias, M, act, what, k=3):
    """the op rule per row; prints the worst row of ours and of torch's"""
    ref = R.conv_ref(x, w, bias, M, act, k=k)
    assert tuple(got.shape) == ref.shape, (got.shape, ref.shape)
    ours = R.row_scores(got.cpu(), ref)
    them = R.row_scores(_theirs(x, w, bias, M, act, k=k).contiguous(), ref)
    print(f"conv_k3s2 {what}: worst row ours {ours[1]:.2e} (row {divmod(ours[2], M)}) torch {them[1]:.2e}, whole {ours[0]:.2e}, "
          f"elements off {ours[3]}")
    assert ours[1] < max(OP_TOL, 8 * them[1]), (what, ours, them)
    assert ours[3] == 0, (what, ours)


@pytest.mark.parametrize("Cc", [32, 96, 160, 64])
def test_every_length_per_row_and_bit_for_bit(Cc):
    """One pass at M = 260 scored against float64; then every M' below it (C = 160 and 64: the edge list) on the same buffer must
    give the long run's rows [0, M') bit for bit — every residue mod 128 and both sides of the tile edges at 128 and 256 — with
    the two rows behind each utterance and the guards still NaN (_run)."""
    torch = _torch()
    M = 260
    x, w, bias = R.draw(np.random.default_rng(Cc), 3, R.frames_for(M), Cc)
    xd, bd = _dev(x), _dev(bias)
    full = _run(xd, w, bd, M)
    _check(full, x, w, bias, M, 1, ("C", Cc, "M", M))
    bad = [m for m in (range(1, M) if Cc in (32, 96) else EDGES) if not torch.equal(_run(xd, w, bd, m), full[:, :m])]
    assert not bad, ("rows [0, M') differ from the long run's at M' =", bad)


@pytest.mark.parametrize("Cc", [32, 160])
def test_frame_2m_plus_1_is_never_read(Cc):
    """x_bs = (2M + 2) C: frame 2M + 1 of every utterance — the first frame of the next one is right behind it — and a guard
    behind the last utterance become NaN; the output stays finite and keeps its bits.  M odd and even, either side of 128."""
    torch = _torch()
    for M in (1, 2, 127, 128, 129, 130):
        L = R.frames_for(M)
        x, w, bias = R.draw(np.random.default_rng(7 * Cc + M), 3, L, Cc)
        buf = torch.full((3 * L * Cc + GUARD,), float("nan"), device="cuda")
        xd = buf[:3 * L * Cc].view(3, L, Cc)
        xd[:] = _dev(x)
        clean = _run(xd, w, _dev(bias), M)
        xd[:, 2 * M + 1] = float("nan")
        got = _run(xd, w, _dev(bias), M)
        assert torch.isfinite(got).all(), ("a frame behind 2M was read", M)
        assert torch.equal(got, clean), M
        _check(got, x, w, bias, M, 1, ("C", Cc, "M", M, "NaN behind frame 2M"))


@pytest.mark.parametrize("Cc", [96, 160])
def test_a_rows_bits_do_not_depend_on_where_it_sits(Cc):
    """An utterance behind 4s junk frames (loud ones) gives its rows 2s further down with the same bits; alone, in a permuted
    batch and in another B it gives the same bits."""
    torch = _torch()
    M, nb = 130, 5
    rng = np.random.default_rng(Cc + 1)
    x, w, bias = R.draw(rng, nb, R.frames_for(M), Cc)
    bd = _dev(bias)
    full = _run(_dev(x), w, bd, M)
    assert torch.isfinite(full).all()
    for s in (1, 2, 33):
        junk = (100.0 * rng.standard_normal((nb, 4 * s, Cc))).astype(np.float32)
        moved = _run(_dev(np.concatenate([junk, x], axis=1)), w, bd, M + 2 * s)
        assert torch.equal(moved[:, 2 * s:], full), ("behind junk frames", 4 * s)
    for ub in range(nb):
        assert torch.equal(_run(_dev(x[ub:ub + 1]), w, bd, M)[0], full[ub]), ("alone", ub)
    perm = [3, 0, 4, 2, 1]
    permuted = _run(_dev(x[perm]), w, bd, M)
    for j, i in enumerate(perm):
        assert torch.equal(permuted[j], full[i]), ("permuted", j, i)
    wide = _run(_dev(np.concatenate([x] * 7)[:-1]), w, bd, M)
    assert torch.equal(wide[:nb], full) and torch.equal(wide[-4:], full[:4]), "another B"


@pytest.mark.parametrize("Cc, M, nmax", [(32, 3, 24), (160, 130, 5)])
def test_every_small_grid_maps_each_tile_once(Cc, M, nmax):
    """Grids of 1..24 workgroups (C = 32, M = 3: one tile per utterance) on both sides of the 8-XCD remainder rule, and of 4..20
    (C = 160, M = 130: four tiles per utterance): every utterance equals its stand-alone run bit for bit, so the tile remap is a
    bijection at each size (a tile mapped twice leaves another one NaN)."""
    torch = _torch()
    x, w, bias = R.draw(np.random.default_rng(3 * Cc), nmax, R.frames_for(M), Cc)
    xd, bd = _dev(x), _dev(bias)
    alone = torch.stack([_run(xd[b:b + 1], w, bd, M)[0] for b in range(nmax)])
    assert torch.isfinite(alone).all()
    _check(alone, x, w, bias, M, 1, ("C", Cc, "M", M, "alone"))
    bad = [B for B in range(1, nmax + 1) if not torch.equal(_run(xd[:B], w, bd, M), alone[:B])]
    assert not bad, ("an utterance differs from its stand-alone run at B =", bad)


@pytest.mark.parametrize("Cc", [32, 160])
def test_row_limit_zeroes_the_rows_at_and_above_it(Cc):
    torch = _torch()
    M = 130
    limits = [M, 1, M - 1, 0, 64, 65]
    x, w, bias = R.draw(np.random.default_rng(11 * Cc), len(limits), R.frames_for(M), Cc)
    xd, bd = _dev(x), _dev(bias)
    free = _run(xd, w, bd, M)
    got = _run(xd, w, bd, M, limit=_dev(limits, np.int32))
    for b, lim in enumerate(limits):
        assert torch.equal(got[b, :lim], free[b, :lim]), ("rows below the limit", b, lim)
        assert (got[b, lim:].view(torch.int32) == 0).all(), ("rows at or above the limit are not +0.0", b, lim)
    assert torch.equal(_run(xd, w, bd, M, limit=_dev([M] * len(limits), np.int32)), free)


@pytest.mark.parametrize("Cc", [32, 160])
def test_both_activations_and_a_null_bias(Cc):
    torch = _torch()
    M = 129
    x, w, bias = R.draw(np.random.default_rng(13 * Cc), 3, R.frames_for(M), Cc)
    xd = _dev(x)
    for act in (0, 1):
        _check(_run(xd, w, _dev(bias), M, act=act), x, w, bias, M, act, ("C", Cc, "act", act))
        none = _run(xd, w, None, M, act=act)
        _check(none, x, w, None, M, act, ("C", Cc, "act", act, "no bias"))
        assert torch.equal(none, _run(xd, w, _dev(np.zeros(Cc)), M, act=act)), ("a null bias is not a zero bias", act)


def test_the_released_width_once():
    M, Cc = 257, 512
    x, w, bias = R.draw(np.random.default_rng(512), 3, R.frames_for(M), Cc)
    _check(_run(_dev(x), w, _dev(bias), M), x, w, bias, M, 1, ("C", Cc, "M", M))


def _gemm(xd, w, bias, M, act):
    """the same convolution as the implicit GEMM: rows of lda = 2C floats, K = k C, the tap-major weight, through s3enc_op_gemm"""
    from s3prl_amd import _lib

    torch = _torch()
    B, L, Cc = xd.shape
    k = w.shape[2]
    wt = _dev(np.ascontiguousarray(w.transpose(0, 2, 1)).reshape(Cc, k * Cc))  # [n][j * C + c]
    out = torch.full((B, M, Cc), float("nan"), device="cuda")
    _lib.check(_lib.load().s3enc_op_gemm(_lib.F32, _ptr(xd), 2 * Cc, L * Cc, _ptr(wt), _ptr(bias), M, Cc, k * Cc, B, act, None, None,
                                         _ptr(out), None, Cc, M * Cc, None), "s3enc_op_gemm")
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("Cc", [32, 96, 160])
def test_the_implicit_gemm_per_row_at_the_edge_lengths(Cc):
    """What conv_f22 = 0 runs: scored per row under the same rule at the edge list of M, with a NaN frame right behind the last
    frame it may read (2M for k = 3; 2M - 1 for conv5-6's k = 2, at M of 1 and either side of 128)."""
    torch = _torch()
    for k, lengths in ((3, EDGES), (2, [1, 127, 128, 129])):
        for M in lengths:
            last = 2 * (M - 1) + k - 1
            x, w, bias = R.draw(np.random.default_rng(17 * Cc + 2 * M + k), 3, last + 2, Cc)
            w = np.ascontiguousarray(w[:, :, :k])
            x[:, last + 1] = np.nan
            got = _gemm(_dev(x), w, _dev(bias), M, 1)
            assert torch.isfinite(got).all(), ("a frame behind the last one was read", k, M)
            _check(got, x, w, bias, M, 1, ("gemm C", Cc, "k", k, "M", M), k=k)


@pytest.mark.parametrize("l1", [129, 192])
def test_the_engine_runs_this_op(l1):
    """test_conv_f22_gpu.py's GroupNorm extractor: the handle's conv2 tap is this op (GELU, the checkpoint's conv_layers.2 weight)
    applied to its conv1 tap, bit for bit — the same kernel on weights packed by the same code."""
    from s3prl_amd.encoder import HipEncoder
    from s3prl_amd.synth import named_config, synth_wavs, synth_weights

    torch = _torch()
    cfg = named_config("tiny_hubert")
    cfg.conv_layers = [(128, 10, 5)] + [(128, 3, 2)] * 3
    cfg.encoder_layers = 1
    weights = synth_weights(cfg, 3)
    n = 5 * (2 * l1) + 10  # a waveform whose conv1 output has l1 frames
    enc = HipEncoder(cfg, weights, dtype="fp32")
    try:
        enc.forward([torch.from_numpy(wv).cuda() for wv in synth_wavs([n, n], l1)])
        torch.cuda.synchronize()
        conv1 = enc.debug_tap("conv1").reshape(2, l1, 128)
        l2 = (l1 - 3) // 2 + 1
        conv2 = enc.debug_tap("conv2").reshape(2, l2, 128)
    finally:
        enc.close()
    bias = weights.get("feature_extractor.conv_layers.2.0.bias")
    got = _run(_dev(conv1), weights["feature_extractor.conv_layers.2.0.weight"], _dev(bias), l2)
    assert np.isfinite(conv2).all() and np.array_equal(got.cpu().numpy(), conv2)


def test_refusals_by_message():
    from s3prl_amd import _lib

    torch = _torch()
    lib = _lib.load()
    M, Cc = 5, 32
    x, w, bias = R.draw(np.random.default_rng(1), 2, R.frames_for(M), Cc)
    xd, bd = _dev(x), _dev(bias)
    out = torch.zeros((2 * M * Cc + 8,), device="cuda")
    L = x.shape[1]

    def refused(match, x=xd, x_bs=L * Cc, w=w, bias=bd, M=M, Cc=Cc, act=1, out=out, o_bs=M * Cc, null_w=False):
        wh = np.ascontiguousarray(w, dtype=np.float32)
        with pytest.raises(_lib.S3EncError, match=match):
            _lib.check(lib.s3enc_op_conv_k3s2(_ptr(x), x_bs, None if null_w else C.c_void_p(wh.ctypes.data), _ptr(bias), None, 2, M, Cc,
                                              act, _ptr(out), o_bs, None), "s3enc_op_conv_k3s2")

    refused("null argument", x=None)
    refused("null argument", null_w=True)
    refused("null argument", out=None)
    refused("C must be a multiple of 32", Cc=48, w=np.zeros((48, 48, 3)), x_bs=L * 48, o_bs=M * 48)
    refused("C must be a multiple of 32", Cc=16, w=np.zeros((16, 16, 3)))
    refused("frame 2M must exist", x_bs=2 * M * Cc)
    refused("o_bs is smaller than M C", o_bs=(M - 1) * Cc)
    refused("16-byte aligned", x=xd.view(-1)[1:])
    refused("16-byte aligned", out=out[2:])
    refused("16-byte aligned", bias=_dev(np.zeros(Cc + 1))[1:])
    refused("multiples of 4 floats", x_bs=L * Cc + 2)
    refused("multiples of 4 floats", o_bs=M * Cc + 1)
    refused("act must be 0 .* or 1", act=2)
    refused("bad shape", M=0)
    _lib.check(lib.s3enc_set_tuning(b"conv_f22", 0), "s3enc_set_tuning")
    try:
        refused("conv_f22 is 0")
    finally:
        _lib.check(lib.s3enc_set_tuning(b"conv_f22", 1), "s3enc_set_tuning")
    assert (out == 0).all(), "a refused call wrote"
    _run(xd, w, bd, M)  # and the same operands are accepted
