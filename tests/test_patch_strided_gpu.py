"""s3enc_op_patch_embed_strided alone (csrc/patchstrided.hip) against float64: every token row to FP32_TOL — the per-row bound of
s3enc_op_patch_embed's tests, K = 256 being the same K class — at the smallest shapes that cross each edge: the patch geometry
(16 x 16, stride 10 x 10) at t_dim 1, 5, 6 and 11 (12, 60, 72 and 132 tokens: each side of the 64- and the 128-row tile), the frame
geometry (128 x 2, stride 128 x 1) at t_dim 1, 63, 64, 65 and 129, one, two and three windows, N below and above one n-tile.  The image
rows behind a window's ``rows`` are NaN (they must never be read).  Both forms (the implicit GEMM and gather + tile GEMM + position
add) to the same bound; a window's rows bit for bit alone and as the last of three and at both tile heights; the two prefix rows;
the refusals.

Inputs: unit-variance images, weights 1 / sqrt(K), bias and position rows of deviation 0.5 — a token row's N values stay at the scale
of their products, so its relative error measures fp32 rounding (the rule of the patch-embedding op tests)."""

import ctypes as C

import numpy as np
import pytest

from oracle import encoder_oracle as O

pytestmark = pytest.mark.gpu

FP32_TOL = 1e-4  # the project's fixture bound, the per-row bound of tests/test_patch_embed_gpu.py

PATCH, FRAME = (16, 16, 10, 10), (128, 2, 128, 1)  # fshape, tshape, fstride, tstride
# (geometry, t_dim, extra image rows inside `rows` behind the last patch, windows, N)
SHAPES = [
    (PATCH, 1, 0, 1, 64), (PATCH, 5, 9, 3, 192), (PATCH, 6, 3, 2, 64), (PATCH, 11, 4, 1, 192), (PATCH, 11, 0, 3, 64),
    (FRAME, 1, 0, 3, 192), (FRAME, 63, 0, 1, 64), (FRAME, 64, 0, 2, 192), (FRAME, 65, 0, 1, 64), (FRAME, 129, 0, 3, 64),
    (FRAME, 129, 0, 1, 192),
]


def _torch():
    import torch

    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def _lib():
    from s3prl_amd import _lib

    return _lib


def _dims(geo, rows):
    fs, ts, fst, tst = geo
    return (128 - fs) // fst + 1, (rows - ts) // tst + 1


def _case(geo, t_dim, extra, nwin, N, seed=0):
    """images of `rows` rows with two NaN rows behind them, weights in [n][t][f] order, bias, time-major position rows, prefix rows"""
    fs, ts, fst, tst = geo
    rng = np.random.default_rng([fs, ts, t_dim, extra, nwin, N, seed])
    rows = ts + tst * (t_dim - 1) + extra
    assert _dims(geo, rows)[1] == t_dim
    f_dim = _dims(geo, rows)[0]
    img = rng.standard_normal((nwin, rows + 2, 128)).astype(np.float32)
    img[:, rows:] = np.nan
    K = fs * ts
    w = (rng.standard_normal((N, ts, fs)) / np.sqrt(K)).astype(np.float32)
    bias = (0.5 * rng.standard_normal(N)).astype(np.float32)
    pos = (0.5 * rng.standard_normal((t_dim * f_dim, N))).astype(np.float32)
    prefix = rng.standard_normal((2, N)).astype(np.float32)
    return img, rows, w, bias, pos, prefix


def _ref(geo, img, rows, w, bias, pos):
    """(nwin, f_dim * t_dim, N) float64, time-major: token ti * f_dim + fi"""
    fs, ts, fst, tst = geo
    f_dim, t_dim = _dims(geo, rows)
    x = img.astype(np.float64)
    pat = np.stack([np.stack([x[:, ti * tst:ti * tst + ts, fi * fst:fi * fst + fs] for fi in range(f_dim)], 1) for ti in range(t_dim)], 1)
    out = np.einsum("wtfab,nab->wtfn", pat, w.astype(np.float64)) + bias.astype(np.float64)
    out = out.reshape(img.shape[0], t_dim * f_dim, -1)
    return out + (0 if pos is None else pos.astype(np.float64))


def _run(geo, img, rows, w, bias, pos, prefix, fused=1, tile_rows=0):
    torch = _torch()
    L = _lib()
    lib = L.load()
    fs, ts, fst, tst = geo
    f_dim, t_dim = _dims(geo, rows)
    nwin, N = img.shape[0], w.shape[0]
    d_img = torch.from_numpy(img).cuda()
    dev = lambda a: None if a is None else torch.from_numpy(a).cuda()
    d_bias, d_pos, d_pre = dev(bias), dev(pos), dev(prefix)
    out = torch.full((nwin, 2 + f_dim * t_dim, N), float("nan"), dtype=torch.float32, device="cuda")
    wh = np.ascontiguousarray(w.reshape(N, -1), dtype=np.float32)
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    L.check(lib.s3enc_set_tuning(b"patch_strided_fused", int(fused)), "s3enc_set_tuning")
    try:
        rc = lib.s3enc_op_patch_embed_strided(p(d_img), img.shape[1] * 128, wh.ctypes.data_as(C.c_void_p), p(d_bias), p(d_pos), p(d_pre),
                                              nwin, rows, fs, ts, fst, tst, N, tile_rows, p(out), None)
    finally:
        L.check(lib.s3enc_set_tuning(b"patch_strided_fused", 1), "s3enc_set_tuning")
    L.check(rc, "s3enc_op_patch_embed_strided")
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _row_errs(g, h):
    return [O.rel_err(g[b, t], h[b, t]) for b in range(h.shape[0]) for t in range(h.shape[1])]


@pytest.mark.parametrize("fused", [1, 0])
@pytest.mark.parametrize("geo, t_dim, extra, nwin, N", SHAPES)
def test_every_token_row_against_float64(geo, t_dim, extra, nwin, N, fused):
    img, rows, w, bias, pos, prefix = _case(geo, t_dim, extra, nwin, N)
    got = _run(geo, img, rows, w, bias, pos, prefix, fused=fused)
    want = _ref(geo, img, rows, w, bias, pos)
    assert got.shape == (nwin, 2 + want.shape[1], N) and np.isfinite(got).all()  # the NaN rows behind `rows` were never read
    assert all(np.array_equal(got[i, :2], prefix) for i in range(nwin))
    errs = _row_errs(got[:, 2:], want)
    print(f"{geo} t_dim {t_dim} windows {nwin} N {N} fused {fused}: worst token row {max(errs):.2e}")
    assert max(errs) < FP32_TOL


def test_the_shape_set_covers_every_edge():
    assert {s[1] for s in SHAPES if s[0] == PATCH} == {1, 5, 6, 11} and {s[1] for s in SHAPES if s[0] == FRAME} == {1, 63, 64, 65, 129}
    assert {12 * s[1] for s in SHAPES if s[0] == PATCH} == {12, 60, 72, 132}
    for geo in (PATCH, FRAME):
        assert {s[3] for s in SHAPES if s[0] == geo} == {1, 2, 3} and {s[4] for s in SHAPES if s[0] == geo} == {64, 192}


@pytest.mark.parametrize("geo, t_dim, N", [(PATCH, 11, 192), (PATCH, 5, 64), (FRAME, 129, 64), (FRAME, 64, 192)])
def test_fused_against_the_two_step_form(geo, t_dim, N):
    img, rows, w, bias, pos, prefix = _case(geo, t_dim, 2 if geo == PATCH else 0, 3, N, seed=3)
    fused = _run(geo, img, rows, w, bias, pos, prefix, fused=1)
    two = _run(geo, img, rows, w, bias, pos, prefix, fused=0)
    assert np.isfinite(two).all() and np.array_equal(fused[:, :2], two[:, :2])
    assert max(_row_errs(fused[:, 2:], two[:, 2:])) < FP32_TOL


@pytest.mark.parametrize("geo, t_dim", [(PATCH, 11), (PATCH, 5), (FRAME, 129), (FRAME, 65)])
def test_a_windows_bits_do_not_depend_on_its_place_the_window_count_or_the_tile_height(geo, t_dim):
    img, rows, w, bias, pos, prefix = _case(geo, t_dim, 0, 3, 192, seed=2)
    three = _run(geo, img, rows, w, bias, pos, prefix)
    alone = _run(geo, img[2:3], rows, w, bias, pos, prefix)
    assert np.array_equal(alone[0], three[2])  # alone and as the last of three
    first = _run(geo, img[[2, 0, 1]], rows, w, bias, pos, prefix)
    assert np.array_equal(first[0], three[2]) and np.array_equal(first[1], three[0])
    t64 = _run(geo, img, rows, w, bias, pos, prefix, tile_rows=64)
    t128 = _run(geo, img, rows, w, bias, pos, prefix, tile_rows=128)
    assert np.array_equal(t64, three) and np.array_equal(t128, three)


def test_without_position_and_prefix_rows():
    """pos = null adds nothing; prefix = null leaves rows 0 and 1 of every sequence as they were"""
    img, rows, w, bias, pos, prefix = _case(PATCH, 6, 0, 2, 64, seed=4)
    bare = _run(PATCH, img, rows, w, bias, None, None)
    assert np.isnan(bare[:, :2]).all()
    assert max(_row_errs(bare[:, 2:], _ref(PATCH, img, rows, w, bias, None))) < FP32_TOL
    full = _run(PATCH, img, rows, w, bias, pos, None)
    d = full[:, 2:].astype(np.float64) - bare[:, 2:]
    assert np.abs(d - pos).max() < 1e-6 * 8  # one fp32 rounding of a sum of magnitude < 8


def test_refusals_by_message():
    torch = _torch()
    L = _lib()
    img, rows, w, bias, pos, prefix = _case(PATCH, 2, 0, 1, 64)
    z = lambda n, ts, fs: np.zeros((n, ts, fs), np.float32)
    for geo, wz, msg in (((48, 16, 10, 10), z(64, 16, 48), "fshape must be 16, 32, 64 or 128"), ((8, 16, 10, 10), z(64, 16, 8), "fshape must be 16, 32, 64 or 128"),
                         ((16, 0, 10, 10), z(64, 1, 16), "tshape must be 1..32"), ((16, 33, 10, 10), z(64, 33, 16), "tshape must be 1..32"),
                         ((16, 16, 9, 10), z(64, 16, 16), "fstride must be even"), ((16, 16, 10, 0), z(64, 16, 16), "tstride must be 1..1024")):
        with pytest.raises(L.S3EncError, match=msg):
            lib = L.load()
            d = torch.zeros((1, 64, 128), device="cuda")
            o = torch.zeros((1, 4096, 64), device="cuda")
            L.check(lib.s3enc_op_patch_embed_strided(C.c_void_p(d.data_ptr()), 64 * 128, wz.ctypes.data_as(C.c_void_p), None, None, None, 1, 40,
                                                     *geo, 64, 0, C.c_void_p(o.data_ptr()), None), "s3enc_op_patch_embed_strided")
    with pytest.raises(L.S3EncError, match="N must be a multiple of 4"):
        _run(PATCH, img, rows, np.zeros((66, 16, 16), np.float32), None, None, None)
    with pytest.raises(L.S3EncError, match="fewer rows than one patch"):
        _run(PATCH, img, 15, w, bias, None, None)
    with pytest.raises(L.S3EncError, match="img window stride is smaller than the window's image rows"):
        _run(PATCH, img[:, :20], rows, w, bias, None, None)
    with pytest.raises(L.S3EncError, match="tile_rows must be 0, 64 or 128"):
        _run(PATCH, img, rows, w, bias, None, None, tile_rows=32)
    lib = L.load()
    d = torch.zeros(2 * 40 * 128 + 4, device="cuda")
    rc = lib.s3enc_op_patch_embed_strided(C.c_void_p(d.data_ptr() + 4), 40 * 128, w.ctypes.data_as(C.c_void_p), None, None, None, 1, 26, 16, 16,
                                          10, 10, 64, 0, C.c_void_p(d.data_ptr()), None)
    with pytest.raises(L.S3EncError, match="16-byte aligned"):
        L.check(rc, "s3enc_op_patch_embed_strided")
