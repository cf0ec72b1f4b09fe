"""s3enc_op_stem7x7_pool on the MI355X through the C ABI: BYOL-S's ResNet stem — Conv2d(1, 64, 7, padding 3) + per-channel affine + ReLU
+ MaxPool2d(3, 2, 1) on (H, 64) single-channel images — against float64 pixel by pixel at H of 1, 2, 7 and 26 (one pool row, an even
and two odd / even heights with both edge cases of the pool), the fused kernel equal to the split form bit for bit, a NaN input pixel
reaching exactly the pooled pixels whose windows hold it, and the destination's border untouched.

The per-pixel rule is test_conv2d_gpu.py's, with torch's own fp32 conv2d + max_pool2d as the yardstick's yardstick."""

import ctypes as C

import numpy as np
import pytest

import posconv_ref as PR

pytestmark = pytest.mark.gpu

OP_TOL = 2e-5  # the project's op bound
HEIGHTS = [1, 2, 7, 26]


def _torch():
    import torch

    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _dev(a):
    return _torch().from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def _inputs(nb, H, seed):
    """unit-variance images (example 1 is loud), weights 1 / 7, a folded BatchNorm whose shifts put a good part of the values across
    the ReLU's edge"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((nb, H, 64)).astype(np.float32)
    if nb > 1:
        x[1] *= 30.0
    w = (rng.standard_normal((64, 1, 7, 7)) / 7.0).astype(np.float32)
    scale = (1.0 + 0.2 * rng.standard_normal(64)) / np.sqrt(rng.uniform(0.5, 2.0, 64) + 1e-5)
    shift = 0.3 * rng.standard_normal(64)
    return x, w, scale, shift


def _op(x, w, scale, shift, fused, guard=0):
    """-> the pooled (B, Hp, 32, 64) interior, and the whole bordered destination (its border pre-filled with -7)"""
    from s3prl_amd import _lib

    torch = _torch()
    lib = _lib.load()
    nb, H = x.shape[:2]
    Hp = (H - 1) // 2 + 1
    xb = torch.zeros((nb, H + 8, 72), device="cuda")
    xb[:, 4:H + 4, 4:68] = torch.from_numpy(x).cuda()
    dst = torch.full((nb, Hp + 2, 34, 64), -7.0, device="cuda")
    dst[:, 1:Hp + 1, 1:33] = float("nan")
    fmap = None if fused else torch.zeros((nb, H + 2, 66, 64), device="cuda")
    wh = np.ascontiguousarray(w, dtype=np.float32)
    sc, sh = _dev(scale), _dev(shift)
    _lib.check(lib.s3enc_op_stem7x7_pool(_ptr(xb), C.c_void_p(wh.ctypes.data), _ptr(sc), _ptr(sh), nb, H, fused, _ptr(dst),
                                         _ptr(fmap), None), "s3enc_op_stem7x7_pool")
    torch.cuda.synchronize()
    return dst[:, 1:Hp + 1, 1:33].contiguous(), dst, fmap


def _torch_ref(x, w, scale, shift, dtype):
    torch = _torch()
    F = torch.nn.functional
    y = F.conv2d(torch.from_numpy(x).cuda().to(dtype)[:, None], torch.from_numpy(w).cuda().to(dtype), None, padding=3)
    y = y * torch.from_numpy(scale).cuda().to(dtype)[None, :, None, None] + torch.from_numpy(shift).cuda().to(dtype)[None, :, None, None]
    return F.max_pool2d(torch.relu(y), 3, 2, 1).permute(0, 2, 3, 1).contiguous()


@pytest.mark.parametrize("H", HEIGHTS)
def test_the_stem_per_pixel_and_fused_equals_split(H):
    torch = _torch()
    nb = 3
    x, w, scale, shift = _inputs(nb, H, 100 + H)
    ref = _torch_ref(x, w, scale, shift, torch.float64)
    theirs = _torch_ref(x, w, scale.astype(np.float32), shift.astype(np.float32), torch.float32)
    Hp = (H - 1) // 2 + 1
    assert tuple(ref.shape) == (nb, Hp, 32, 64)
    got = {}
    for fused in (1, 0):
        got[fused], dst, _ = _op(x, w, scale, shift, fused)
        inner = torch.zeros((Hp + 2, 34), dtype=torch.bool, device="cuda")
        inner[1:Hp + 1, 1:33] = True
        assert (dst[:, ~inner] == -7.0).all(), "a border pixel of dst was written"
        ours = PR.frame_scores(got[fused].reshape(nb, Hp * 32, 64), ref.reshape(nb, Hp * 32, 64), OP_TOL).cpu().numpy()
        them = PR.frame_scores(theirs.reshape(nb, Hp * 32, 64), ref.reshape(nb, Hp * 32, 64), OP_TOL).cpu().numpy()
        print(f"stem H {H} fused {fused}: worst pixel ours {ours[1]:.2e} theirs {them[1]:.2e}, whole {ours[0]:.2e}, elements off {int(ours[3])}")
        assert ours[1] < max(OP_TOL, 8 * them[1]) and ours[3] == 0, (H, fused, ours, them)
        assert (got[fused] >= 0).all() and not torch.signbit(got[fused]).any()  # behind the ReLU, and never a negative zero
    assert torch.equal(got[1], got[0]), "the fused and the split form differ"


def test_the_split_forms_map_is_the_unpooled_activation():
    torch = _torch()
    x, w, scale, shift = _inputs(2, 7, 5)
    pooled, _, fmap = _op(x, w, scale, shift, 0)
    F = torch.nn.functional
    want = F.max_pool2d(fmap[:, 1:8, 1:65].permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1)
    assert torch.equal(pooled, want)
    border = torch.ones((9, 66), dtype=torch.bool, device="cuda")
    border[1:8, 1:65] = False
    assert (fmap[:, border] == 0).all(), "the map's border was written"


def test_a_nan_reaches_every_window_that_holds_it():
    """a NaN at input pixel (y, x) reaches the un-pooled pixels within 3 of it, hence the pooled pixels whose 3 x 3 / stride-2 window
    (rows 2 yo - 1 .. 2 yo + 1) meets rows y - 3 .. y + 3 — and no other"""
    torch = _torch()
    H = 26
    for (y, xx) in [(0, 0), (12, 31), (25, 63), (7, 40)]:
        x, w, scale, shift = _inputs(1, H, 11 + y)
        x[0, y, xx] = np.nan
        want = np.zeros(((H - 1) // 2 + 1, 32), bool)
        for yo in range(want.shape[0]):
            for xo in range(32):
                rows = [r for r in range(2 * yo - 1, 2 * yo + 2) if 0 <= r < H]
                cols = [c for c in range(2 * xo - 1, 2 * xo + 2) if 0 <= c < 64]
                want[yo, xo] = any(abs(r - y) <= 3 for r in rows) and any(abs(c - xx) <= 3 for c in cols)
        for fused in (1, 0):
            got, _, _ = _op(x, w, scale, shift, fused)
            nan_px = torch.isnan(got).all(dim=3)[0].cpu().numpy()
            any_px = torch.isnan(got).any(dim=3)[0].cpu().numpy()
            assert (nan_px == want).all() and (any_px == want).all(), (y, xx, fused)


def test_refusals_by_message():
    from s3prl_amd import _lib

    torch = _torch()
    lib = _lib.load()
    x, w, scale, shift = _inputs(1, 4, 1)
    xb = torch.zeros((1, 12, 72), device="cuda")
    dst = torch.zeros((1, 4, 34, 64), device="cuda")
    wh = np.ascontiguousarray(w)
    sc, sh = _dev(scale), _dev(shift)
    assert lib.s3enc_op_stem7x7_pool(_ptr(xb), C.c_void_p(wh.ctypes.data), _ptr(sc), _ptr(sh), 1, 4, 0, _ptr(dst), None, None) != 0
    assert lib.s3enc_last_error().decode() == "s3enc_op_stem7x7_pool: the split form needs its map"
    assert lib.s3enc_op_stem7x7_pool(_ptr(xb), C.c_void_p(wh.ctypes.data), _ptr(sc), _ptr(sh), 1, 4, 2, _ptr(dst), None, None) != 0
    assert lib.s3enc_last_error().decode() == "s3enc_op_stem7x7_pool: fused must be 0 or 1"
    assert lib.s3enc_op_stem7x7_pool(_ptr(xb), C.c_void_p(wh.ctypes.data), _ptr(sc), _ptr(sh), 1, 0, 1, _ptr(dst), None, None) != 0
    assert lib.s3enc_last_error().decode() == "s3enc_op_stem7x7_pool: bad shape"
