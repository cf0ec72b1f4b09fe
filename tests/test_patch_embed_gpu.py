"""s3enc_op_patch_embed alone (csrc/patchembed.hip) against float64: every token row to FP32_TOL at the smallest shapes that cross
each edge — every (kt, kc) class, one / two / 63 / 65 / 129 time steps (one tile, a ragged second tile, several tiles), N below,
beside and above one n-tile, one and three utterances, a batch large enough for the 128-row tile — with the frames behind the last
whole patch set to NaN (they must never be read); the position rows below kv[b] and their absence at and above it; a row's bits
across B, place in the batch, Tt and tile height; the fused kernel against the two-step form and, for (2, 128), against
s3enc_op_gemm on the contiguous view; the refusals.

Inputs: unit-variance images, weights 1 / sqrt(K), bias and position rows of deviation 0.5 — a token row's N values stay at the scale
of their products, so its relative error measures fp32 rounding (the rule of the conv2d op tests)."""

import ctypes as C

import numpy as np
import pytest

from oracle import encoder_oracle as O

pytestmark = pytest.mark.gpu

FP32_TOL = 1e-4  # the project's fixture bound

# (kt, kc, Tt, N, B)
SHAPES = [
    (16, 16, 1, 64, 1), (16, 16, 2, 132, 3), (16, 16, 63, 768, 1), (16, 16, 65, 64, 3), (16, 16, 129, 132, 1),
    (2, 128, 1, 132, 3), (2, 128, 63, 64, 1), (2, 128, 65, 768, 3), (2, 128, 129, 64, 1),
    (1, 16, 2, 64, 3), (1, 16, 65, 132, 1), (1, 16, 129, 768, 1),
    (3, 32, 1, 768, 1), (3, 32, 63, 132, 3), (3, 32, 129, 64, 1),
    (4, 64, 2, 768, 3), (4, 64, 65, 64, 1), (4, 64, 129, 132, 3),
    (16, 16, 129, 768, 5),  # 5 x 9 x 6 = 270 tiles of 128 rows: the 128-row tile
]


def _torch():
    import torch

    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def _lib():
    from s3prl_amd import _lib

    return _lib


def _case(kt, kc, Tt, N, B, seed=0):
    """image with NaN behind the last whole patch (Fpad % kt != 0 where kt > 1), weights, bias, position rows"""
    rng = np.random.default_rng([kt, kc, Tt, N, B, seed])
    V, K = 128 // kc, kt * kc
    Fpad = Tt * kt + (kt - 1 if kt > 1 else 3)
    img = rng.standard_normal((B, Fpad, 128)).astype(np.float32)
    img[:, Tt * kt:] = np.nan
    w = (rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
    bias = (0.5 * rng.standard_normal(N)).astype(np.float32)
    pos = (0.5 * rng.standard_normal((Tt * V, N))).astype(np.float32)
    return img, w, bias, pos


def _kv(B, Ttok, rot=0):
    return [[0, 1, Ttok, Ttok // 2, max(Ttok - 1, 0)][(b + rot) % 5] for b in range(B)]


def _ref(img, w, bias, pos, kv, Tt, kt, kc):
    B = img.shape[0]
    V = 128 // kc
    x = img[:, :Tt * kt].astype(np.float64).reshape(B, Tt, kt, V, kc).transpose(0, 1, 3, 2, 4).reshape(B, Tt * V, kt * kc)
    out = x @ w.astype(np.float64).T + (0 if bias is None else bias.astype(np.float64))
    for b in range(B):
        if pos is not None:
            out[b, :kv[b]] += pos[:kv[b]].astype(np.float64)
    return out


def _run(img, w, bias, pos, kv, Tt, kt, kc, fused=1):
    torch = _torch()
    L = _lib()
    lib = L.load()
    B, Fpad, _ = img.shape
    N, V = w.shape[0], 128 // kc
    d_img = torch.from_numpy(img).cuda()
    d_bias = None if bias is None else torch.from_numpy(bias).cuda()
    d_pos = None if pos is None else torch.from_numpy(pos).cuda()
    d_kv = None if kv is None else torch.tensor(kv, dtype=torch.int32).cuda()
    out = torch.full((B, Tt * V, N), float("nan"), dtype=torch.float32, device="cuda")
    wh = np.ascontiguousarray(w, dtype=np.float32)
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    L.check(lib.s3enc_set_tuning(b"patch_embed_fused", int(fused)), "s3enc_set_tuning")
    try:
        rc = lib.s3enc_op_patch_embed(p(d_img), Fpad * 128, wh.ctypes.data_as(C.c_void_p), p(d_bias), p(d_pos), p(d_kv), B, Tt, kt, kc, N,
                                      p(out), None)
    finally:
        L.check(lib.s3enc_set_tuning(b"patch_embed_fused", 1), "s3enc_set_tuning")
    L.check(rc, "s3enc_op_patch_embed")
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _row_errs(g, h):
    return [O.rel_err(g[b, t], h[b, t]) for b in range(h.shape[0]) for t in range(h.shape[1])]


@pytest.mark.parametrize("kt, kc, Tt, N, B", SHAPES)
def test_every_token_row_against_float64(kt, kc, Tt, N, B):
    img, w, bias, pos = _case(kt, kc, Tt, N, B)
    kv = _kv(B, Tt * (128 // kc))
    got = _run(img, w, bias, pos, kv, Tt, kt, kc)
    want = _ref(img, w, bias, pos, kv, Tt, kt, kc)
    assert got.shape == want.shape and np.isfinite(got).all()  # the NaN frames behind the last whole patch were never read
    rows = _row_errs(got, want)
    print(f"({kt}, {kc}) Tt {Tt} N {N} B {B}: worst token row {max(rows):.2e}")
    assert max(rows) < FP32_TOL


def test_the_shape_set_covers_every_edge():
    assert {(kt, kc) for kt, kc, *_ in SHAPES} == {(16, 16), (2, 128), (1, 16), (3, 32), (4, 64)}
    assert {s[2] for s in SHAPES} == {1, 2, 63, 65, 129} and {s[3] for s in SHAPES} == {64, 132, 768} and {1, 3} <= {s[4] for s in SHAPES}


@pytest.mark.parametrize("kt, kc, Tt, N", [(16, 16, 9, 132), (2, 128, 70, 64)])
def test_position_rows_below_kv_and_absent_above(kt, kc, Tt, N):
    """kv = 0, 1 and Ttok: out - (the same call without positions) is the position row below kv[b] and exactly zero at and above"""
    Ttok = Tt * (128 // kc)
    img, w, bias, pos = _case(kt, kc, Tt, N, 3, seed=1)
    kv = [0, 1, Ttok]
    got = _run(img, w, bias, pos, kv, Tt, kt, kc)
    bare = _run(img, w, bias, None, None, Tt, kt, kc)
    for b in range(3):
        assert np.array_equal(got[b, kv[b]:], bare[b, kv[b]:]), b
        d = got[b, :kv[b]].astype(np.float64) - bare[b, :kv[b]]
        assert np.abs(d - pos[:kv[b]]).max(initial=0.0) < 1e-6 * 8, b  # one fp32 rounding of a sum of magnitude < 8
    assert max(_row_errs(got, _ref(img, w, bias, pos, kv, Tt, kt, kc))) < FP32_TOL


def test_a_rows_bits_do_not_depend_on_batch_place_tt_or_tile_height():
    kt, kc, Tt, N = 16, 16, 129, 768
    V = 8
    img, w, bias, pos = _case(kt, kc, Tt, N, 5, seed=2)
    kv5 = [Tt * V] * 5
    full = _run(img, w, bias, pos, kv5, Tt, kt, kc)                       # 270 tiles of 128 rows
    for b in (0, 3):                                                       # alone: 64-row tiles
        alone = _run(img[b:b + 1], w, bias, pos, [Tt * V], Tt, kt, kc)
        assert np.array_equal(alone[0], full[b]), b
    perm = [4, 2, 0, 1, 3]
    permuted = _run(img[perm], w, bias, pos, kv5, Tt, kt, kc)
    assert all(np.array_equal(permuted[j], full[i]) for j, i in enumerate(perm))
    short = _run(img[1:2, :40 * kt + 5], w, bias, pos[:40 * V], [40 * V], 40, kt, kc)  # fewer time steps: the same leading rows
    assert np.array_equal(short[0], full[1, :40 * V])


@pytest.mark.parametrize("kt, kc, Tt, N, B", [(16, 16, 65, 132, 3), (2, 128, 63, 64, 1), (3, 32, 9, 768, 3), (1, 16, 2, 64, 3), (4, 64, 129, 132, 1)])
def test_fused_against_the_two_step_form(kt, kc, Tt, N, B):
    img, w, bias, pos = _case(kt, kc, Tt, N, B, seed=3)
    kv = _kv(B, Tt * (128 // kc), rot=2)
    fused = _run(img, w, bias, pos, kv, Tt, kt, kc, fused=1)
    two = _run(img, w, bias, pos, kv, Tt, kt, kc, fused=0)
    want = _ref(img, w, bias, pos, kv, Tt, kt, kc)
    assert np.isfinite(two).all()
    assert max(_row_errs(fused, two)) < FP32_TOL and max(_row_errs(two, want)) < FP32_TOL and max(_row_errs(fused, want)) < FP32_TOL


@pytest.mark.parametrize("Tt, N, B", [(65, 132, 3), (129, 768, 1)])
def test_frame_geometry_against_the_tile_gemm_on_the_contiguous_view(Tt, N, B):
    """(2, 128): a token is 256 contiguous floats, so s3enc_op_gemm expresses it with lda = 256"""
    torch = _torch()
    L = _lib()
    lib = L.load()
    kt, kc = 2, 128
    img, w, bias, _ = _case(kt, kc, Tt, N, B, seed=4)
    got = _run(img, w, bias, None, None, Tt, kt, kc)
    Fpad = img.shape[1]
    d_img, d_w, d_b = torch.from_numpy(img).cuda(), torch.from_numpy(w).cuda(), torch.from_numpy(bias).cuda()
    out = torch.empty((B, Tt, N), dtype=torch.float32, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    L.check(lib.s3enc_op_gemm(0, p(d_img), 256, Fpad * 128, p(d_w), p(d_b), Tt, N, 256, B, 0, None, None, p(out), None, N, Tt * N, None),
            "s3enc_op_gemm")
    torch.cuda.synchronize()
    assert max(_row_errs(got, out.cpu().numpy())) < FP32_TOL


def test_refusals_by_message():
    torch = _torch()
    L = _lib()
    img, w, bias, pos = _case(16, 16, 2, 64, 1)
    for kw, msg in ((dict(kc=48), "kc must be 16, 32, 64 or 128"), (dict(kc=8), "kc must be 16, 32, 64 or 128"), (dict(kt=0), "kt must be 1..32"),
                    (dict(kt=33), "kt must be 1..32")):
        a = dict(kt=16, kc=16)
        a.update(kw)
        with pytest.raises(L.S3EncError, match=msg):
            _run(np.zeros((1, 1200, 128), np.float32), np.zeros((64, a["kt"] * a["kc"]), np.float32), None, None, None, 2, a["kt"], a["kc"])
    with pytest.raises(L.S3EncError, match="N must be a multiple of 4"):
        _run(img, np.zeros((66, 256), np.float32), None, None, None, 2, 16, 16)
    with pytest.raises(L.S3EncError, match="img batch stride is smaller than Tt \\* kt image rows"):
        _run(img[:, :20], w, bias, None, None, 2, 16, 16)
    with pytest.raises(L.S3EncError, match="pos and kv come together"):
        _run(img, w, bias, pos, None, 2, 16, 16)
    lib = L.load()
    d = torch.zeros(2 * 47 * 128 + 4, device="cuda")
    rc = lib.s3enc_op_patch_embed(C.c_void_p(d.data_ptr() + 4), 47 * 128, w.ctypes.data_as(C.c_void_p), None, None, None, 1, 2, 16, 16, 64,
                                  C.c_void_p(d.data_ptr()), None)
    with pytest.raises(L.S3EncError, match="16-byte aligned"):
        L.check(rc, "s3enc_op_patch_embed")
