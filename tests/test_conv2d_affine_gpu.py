"""s3enc_op_conv2d3x3_affine on the MI355X, every call through the C ABI: the 3 x 3 / padding-1 convolution with the per-channel
affine (an eval-mode BatchNorm) -> ReLU -> 2 x 2 max-pool in nn.MaxPool2d's floor mode, against float64 pixel by pixel on even and
odd maps, with Cin of 1 / 16 / 64 and Cout below / at / across both n-tile widths (64 and 128), batches whose tiles span examples and
end ragged; and bit for bit where it must be: the pooled output is the max over the un-pooled output's windows, an example's bits
depend neither on B, nor on its position, nor on the n-tile width key, a null scale is the old entry, and nothing outside the
destination's interior is written.

The per-pixel rule is test_conv2d_gpu.py's: a pixel's relative error over its Cout values stays below max(OP_TOL, 8 x the error of
torch's own fp32 conv2d at that group of pixels), and no element is off by more than 50 OP_TOL (1 + |ref|)."""

import ctypes as C

import numpy as np
import pytest

import posconv_ref as PR

pytestmark = pytest.mark.gpu

OP_TOL = 2e-5  # the project's op bound
GUARD = 64

MAPS = [(2, 2), (3, 2), (3, 3), (5, 4), (7, 6), (13, 9), (25, 16)]
# (Cin, Cout, B): Cin of 1 / 16 / 64, Cout of 4 / 64 / 68 / 128 / 192 — the 64-wide tile, a ragged n-tile of either width, both widths
WIDTHS = [(1, 4, 3), (16, 64, 5), (64, 68, 3), (16, 128, 2), (64, 192, 3), (1, 64, 2), (64, 4, 5)]


def _torch():
    import torch

    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _inputs(nb, H, W, Cin, N, seed, loud=30.0):
    """unit-variance channel-last images (example 1 is loud), weights 1 / sqrt(9 Cin), a conv bias, and BatchNorm statistics with
    running variances well away from zero"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((nb, H, W, Cin)).astype(np.float32)
    if nb > 1:
        x[1] *= loud
    w = (rng.standard_normal((N, Cin, 3, 3)) / np.sqrt(9 * Cin)).astype(np.float32)
    b = (0.1 * rng.standard_normal(N)).astype(np.float32)
    bn = dict(gamma=1.0 + 0.2 * rng.standard_normal(N), beta=0.2 * rng.standard_normal(N), mean=0.3 * rng.standard_normal(N),
              var=rng.uniform(0.5, 2.0, N))
    if N < 16:
        # A pixel is scored by its relative error over its Cout values.  With four channels the ReLU leaves, in about one pixel of a
        # thousand, nothing but one value a hundred times below the accumulated products: such a pixel has no scale of its own to
        # measure fp32 rounding against (torch's fp32 conv2d scores 2e-5 there as well).  The few-channel cases therefore get inputs
        # that keep a pixel's values at the scale of its products — no loud example, bias and shift three deviations up — instead of
        # a wider bound; the ReLU's edge is exercised at every other width.
        if nb > 1:
            x[1] /= loud
        b += 3.0
        bn["beta"] += 3.0
    return x, w, b, bn


def _fold(b, bn):
    """(scale, shift) in float64, the conv bias inside the shift"""
    scale = bn["gamma"] / np.sqrt(bn["var"] + 1e-5)
    return scale, (b.astype(np.float64) - bn["mean"]) * scale + bn["beta"]


def _bordered(x, fill=0.0):
    torch = _torch()
    nb, H, W, Cc = x.shape
    xb = torch.full((nb, H + 2, W + 2, Cc), fill, device="cuda")
    xb[:, 1:H + 1, 1:W + 1] = torch.from_numpy(x).cuda()
    return xb


def _dev(a):
    return None if a is None else _torch().from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def _op(xb, w, bias, scale, shift, act, pool, floor, dst, dst_pad, ldo):
    from s3prl_amd import _lib

    lib = _lib.load()
    nb, H, W = xb.shape[0], xb.shape[1] - 2, xb.shape[2] - 2
    N, Cin = w.shape[:2]
    wh = np.ascontiguousarray(w, dtype=np.float32)
    _lib.check(lib.s3enc_op_conv2d3x3_affine(_ptr(xb), C.c_void_p(wh.ctypes.data), _ptr(bias), _ptr(scale), _ptr(shift), nb, H, W, Cin,
                                             N, act, pool, floor, _ptr(dst), dst_pad, ldo, None), "s3enc_op_conv2d3x3_affine")
    _torch().cuda.synchronize()


def _plain(xb, w, bias=None, scale=None, shift=None, act=1, pool=0, floor=0):
    """the op into a NaN-filled plain (B, Ho, Wo, N) tensor"""
    torch = _torch()
    H, W = xb.shape[1] - 2, xb.shape[2] - 2
    out = torch.full((xb.shape[0], H >> pool, W >> pool, w.shape[0]), float("nan"), device="cuda")
    _op(xb, w, bias, scale, shift, act, pool, floor, out, 0, w.shape[0])
    return out


def _torch_ref(x, w, scale, shift, act, pool, dtype):
    """conv2d -> affine -> ReLU -> max_pool2d (floor mode) in `dtype` on the GPU, channel-last"""
    torch = _torch()
    F = torch.nn.functional
    y = F.conv2d(torch.from_numpy(x).cuda().to(dtype).permute(0, 3, 1, 2), torch.from_numpy(w).cuda().to(dtype), None, padding=1)
    y = y * torch.from_numpy(scale).cuda().to(dtype)[None, :, None, None] + torch.from_numpy(shift).cuda().to(dtype)[None, :, None, None]
    if act:
        y = torch.relu(y)
    if pool:
        y = F.max_pool2d(y, 2, 2)
    return y.permute(0, 2, 3, 1).contiguous()


def _check(got, x, w, scale, shift, act, pool, what=()):
    torch = _torch()
    ref = _torch_ref(x, w, scale, shift, act, pool, torch.float64)
    theirs = _torch_ref(x, w, scale.astype(np.float32), shift.astype(np.float32), act, pool, torch.float32)
    nb, Ho, Wo, N = ref.shape
    assert got.shape == ref.shape, (got.shape, ref.shape)
    ours = PR.frame_scores(got.reshape(nb, Ho * Wo, N), ref.reshape(nb, Ho * Wo, N), OP_TOL).cpu().numpy()
    them = PR.frame_scores(theirs.reshape(nb, Ho * Wo, N), ref.reshape(nb, Ho * Wo, N), OP_TOL).cpu().numpy()
    print(f"conv2d3x3_affine {what}: worst pixel ours {ours[1]:.2e} theirs {them[1]:.2e}, whole {ours[0]:.2e}, elements off {int(ours[3])}")
    assert ours[1] < max(OP_TOL, 8 * them[1]), (what, ours, them)
    assert ours[3] == 0, (what, ours)


def _run(x, w, b, bn, affine, pool, floor):
    """the op with or without the affine, and the (scale, shift) its float64 yardstick uses"""
    if affine:
        scale, shift = _fold(b, bn)
        return _plain(_bordered(x), w, None, _dev(scale), _dev(shift), 1, pool, floor), scale, shift
    return _plain(_bordered(x), w, _dev(b), None, None, 1, pool, floor), np.ones(len(b)), b.astype(np.float64)


@pytest.mark.parametrize("H, W", MAPS)
def test_every_map_and_width_per_pixel(H, W):
    even = not ((H | W) & 1)
    for Cin, N, nb in WIDTHS:
        for affine in (0, 1):
            for pool, floor in [(0, 0), (1, 1)] + ([(1, 0)] if even else []):
                x, w, b, bn = _inputs(nb, H, W, Cin, N, 1000 * H + 10 * W + Cin + N + nb)
                got, scale, shift = _run(x, w, b, bn, affine, pool, floor)
                assert got.shape[1:3] == ((H // 2, W // 2) if pool else (H, W))
                _check(got, x, w, scale, shift, 1, pool, what=(H, W, Cin, N, nb, affine, pool, floor))


def test_the_released_map_once():
    """101 x 64 -> 50 x 32 (layer 0, Cin = 1) and, at 64 channels, the MFMA kernel on the same odd map: several 256-row tiles"""
    for Cin, nb in ((1, 3), (64, 3)):
        x, w, b, bn = _inputs(nb, 101, 64, Cin, 64, 4242 + Cin)
        got, scale, shift = _run(x, w, b, bn, 1, 1, 1)
        assert tuple(got.shape) == (nb, 50, 32, 64)
        _check(got, x, w, scale, shift, 1, 1, what=("released", Cin))


@pytest.mark.parametrize("H, W, Cin, N", [(3, 2, 16, 4), (5, 4, 64, 64), (7, 6, 64, 68), (13, 9, 16, 192), (25, 16, 1, 64), (3, 3, 1, 4)])
def test_pooled_equals_the_max_over_the_unpooled_windows(H, W, Cin, N):
    torch = _torch()
    x, w, b, bn = _inputs(3, H, W, Cin, N, 77 + H)
    scale, shift = (_dev(v) for v in _fold(b, bn))
    xb = _bordered(x)
    for act in (0, 1):
        full = _plain(xb, w, None, scale, shift, act, 0, 0)
        pooled = _plain(xb, w, None, scale, shift, act, 1, 1)
        want = torch.nn.functional.max_pool2d(full.permute(0, 3, 1, 2), 2, 2).permute(0, 2, 3, 1)
        assert torch.equal(pooled, want), (act, H, W, Cin, N)


@pytest.mark.parametrize("H, W, Cin, N", [(13, 9, 64, 64), (7, 6, 16, 4), (25, 16, 1, 64), (5, 4, 64, 68)])
def test_an_examples_bits_depend_on_nothing_but_the_example(H, W, Cin, N):
    """Another B, another batch position (examples start inside a tile and straddle two), enough examples for the tall tiles, and
    the 128-wide n-tile instead of the 64-wide one (tuning key conv2d_n64)."""
    from s3prl_amd import _lib

    torch = _torch()
    lib = _lib.load()
    x, w, b, bn = _inputs(5, H, W, Cin, N, 1234 + H)
    scale, shift = (_dev(v) for v in _fold(b, bn))
    run = lambda xs: _plain(_bordered(xs), w, None, scale, shift, 1, 1, 1)  # noqa: E731
    full = run(x)
    assert torch.isfinite(full).all()
    assert torch.equal(run(x), full)
    for ub in range(5):
        assert torch.equal(run(x[ub:ub + 1])[0], full[ub]), ("alone", ub)
    perm = [3, 0, 4, 2, 1]
    permuted = run(x[perm])
    for j, i in enumerate(perm):
        assert torch.equal(permuted[j], full[i]), ("permuted", j, i)
    reps = -(-(256 * 300) // (5 * 4 * (H // 2) * (W // 2)))  # enough rows for the 256-row tiles on a chip of up to 300 CUs
    many = np.concatenate([x] * reps)[:5 * reps - 1]
    wide = run(many)
    assert torch.equal(wide[:5], full) and torch.equal(wide[-4:], full[:4])
    _lib.check(lib.s3enc_set_tuning(b"conv2d_n64", 0), "s3enc_set_tuning")
    try:
        assert torch.equal(run(x), full), "the 128-wide n-tile gives other bits"
        assert torch.equal(run(many)[:5], full)
    finally:
        _lib.check(lib.s3enc_set_tuning(b"conv2d_n64", 1), "s3enc_set_tuning")
    assert lib.s3enc_set_tuning(b"conv2d_n64", 2) != 0 and b"0..1" in lib.s3enc_last_error()


@pytest.mark.parametrize("H, W, Cin, N", [(7, 5, 64, 64), (13, 9, 16, 68), (9, 7, 1, 64)])
def test_border_gap_and_guard_are_untouched(H, W, Cin, N):
    torch = _torch()
    nb, dp, ldo = 3, 2, N + 8
    x, w, b, bn = _inputs(nb, H, W, Cin, N, 55 + H)
    scale, shift = _fold(b, bn)
    Ho, Wo = H // 2, W // 2
    body_n = nb * (Ho + 2 * dp) * (Wo + 2 * dp) * ldo
    buf = torch.full((GUARD + body_n + GUARD,), float("nan"), device="cuda")
    body = buf[GUARD:GUARD + body_n].view(nb, Ho + 2 * dp, Wo + 2 * dp, ldo)
    body[:] = 0.0
    body[..., N:] = -7.0
    body[:, dp:dp + Ho, dp:dp + Wo, :N] = float("nan")
    _op(_bordered(x), w, None, _dev(scale), _dev(shift), 1, 1, 1, body, dp, ldo)
    assert torch.isnan(buf[:GUARD]).all() and torch.isnan(buf[-GUARD:]).all(), "a guard float of dst was written"
    assert (body[..., N:] == -7.0).all(), "the gap behind a pixel was written"
    inner = torch.zeros((Ho + 2 * dp, Wo + 2 * dp), dtype=torch.bool, device="cuda")
    inner[dp:dp + Ho, dp:dp + Wo] = True
    assert (body[:, ~inner][..., :N] == 0.0).all(), "a border pixel of dst is no longer zero"
    got = body[:, dp:dp + Ho, dp:dp + Wo, :N].contiguous()
    _check(got, x, w, scale, shift, 1, 1, what=("dst", H, W, Cin, N))
    assert torch.equal(got, _plain(_bordered(x), w, None, _dev(scale), _dev(shift), 1, 1, 1))


def test_a_nan_stays_a_nan():
    """a NaN at pixel (1, 1) of a 5 x 5 map reaches the un-pooled pixels [0, 3) x [0, 3), so both floor-pool windows of row / column
    0 and 1; the dropped last row and column never enter"""
    torch = _torch()
    for Cin in (1, 16):
        x, w, b, bn = _inputs(1, 5, 5, Cin, 8, 3 + Cin)
        x[0, 1, 1, 0] = np.nan
        scale, shift = (_dev(v) for v in _fold(b, bn))
        got = _plain(_bordered(x), w, None, scale, shift, 1, 1, 1)
        assert torch.isnan(got).all(), Cin
        x[0, 1, 1, 0] = 0.0
        x[0, 4, 4, 0] = np.nan  # reaches un-pooled rows / columns 3 and 4 only: window (1, 1)
        got = _plain(_bordered(x), w, None, scale, shift, 1, 1, 1)
        nan_px = torch.isnan(got).all(dim=3)[0].cpu().numpy()
        assert (nan_px == np.array([[False, False], [False, True]])).all(), (Cin, nan_px)


@pytest.mark.parametrize("Cin, N", [(16, 64), (64, 192), (1, 64)])
def test_a_null_scale_is_the_old_entry_bit_for_bit(Cin, N):
    from s3prl_amd import _lib

    torch = _torch()
    lib = _lib.load()
    x, w, b, _ = _inputs(3, 12, 8, Cin, N, 99 + Cin)
    xb, bias = _bordered(x), _dev(b)
    wh = np.ascontiguousarray(w, dtype=np.float32)
    for pool in (0, 1):
        old = torch.full((3, 12 >> pool, 8 >> pool, N), float("nan"), device="cuda")
        _lib.check(lib.s3enc_op_conv2d3x3(_ptr(xb), C.c_void_p(wh.ctypes.data), _ptr(bias), 3, 12, 8, Cin, N, 1, pool, _ptr(old), 0, N, None),
                   "s3enc_op_conv2d3x3")
        torch.cuda.synchronize()
        for floor in ((0, 1) if pool else (0,)):
            assert torch.equal(_plain(xb, w, bias, None, None, 1, pool, floor), old), (pool, floor)


def test_refusals_by_message():
    from s3prl_amd import _lib

    torch = _torch()

    def refused(match, Cin=16, N=8, H=4, W=4, pool=1, floor=1, bias=False, scale=True, shift=True):
        x, w, b, bn = _inputs(1, H, W, Cin, N, 1)
        sc, sh = (_dev(v) for v in _fold(b, bn))
        out = torch.zeros((H * W * N + 8,), device="cuda")
        with pytest.raises(_lib.S3EncError, match=match):
            _op(_bordered(x), w, _dev(b) if bias else None, sc if scale else None, sh if shift else None, 1, pool, floor, out, 0, N)

    refused("pool_floor needs pool", pool=0)
    refused("pool_floor must be 0 or 1", floor=2)
    refused("smaller than one 2 x 2 pool window", H=1)
    refused("H and W must be even under pool", H=5, floor=0)
    refused("needs both scale and shift", shift=False)
    refused("the shift carries the bias", bias=True)
    refused("Cin must be 1 .* or a multiple of 16", Cin=24)
