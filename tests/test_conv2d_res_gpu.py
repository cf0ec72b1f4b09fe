"""s3enc_op_conv2d_res on the MI355X, every call through the C ABI: the general form of conv2d.hip — k x k taps, k = 3 or 1, at padding
(k - 1) / 2 and stride 1 or 2, the per-channel affine, an optional residual added before the ReLU — against float64 pixel by pixel
on maps from 1 x 1 to 13 x 9 (odd and even, so that stride 2 rounds both ways), with Cin of 16 / 64 / 128 and Cout below / at /
across both n-tile widths, batches whose tiles span examples and end ragged; and bit for bit where it must be: k = 3, stride 1
without a residual is s3enc_op_conv2d3x3_affine, an example's bits depend neither on B, nor on its position, nor on the n-tile width
key, and nothing outside the destination's interior is written.

The per-pixel rule is test_conv2d_gpu.py's: a pixel's relative error over its Cout values stays below max(OP_TOL, 8 x the error of
torch's own fp32 conv2d at that group of pixels), and no element is off by more than 50 OP_TOL (1 + |ref|)."""

import ctypes as C

import numpy as np
import pytest

import posconv_ref as PR

pytestmark = pytest.mark.gpu

OP_TOL = 2e-5  # the project's op bound
GUARD = 64

MAPS = [(1, 1), (2, 2), (2, 3), (3, 3), (4, 7), (5, 4), (8, 13), (13, 9)]
# (Cin, Cout, B): Cin of 16 / 64 / 128, Cout of 64 / 68 / 128 / 192 — the 64-wide tile, a ragged n-tile, both widths; B so that the
# 64-row tiles span examples and the last one is ragged on every map
WIDTHS = [(16, 64, 5), (64, 68, 3), (128, 128, 3), (64, 192, 7), (16, 128, 2)]


def _torch():
    import torch

    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _dev(a):
    return None if a is None else _torch().from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def _out_hw(H, W, k, s):
    p = (k - 1) // 2
    return (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1


def _inputs(nb, H, W, Cin, N, k, s, seed, loud=30.0):
    """unit-variance channel-last images (example 1 is loud), weights 1 / sqrt(k k Cin), a folded BatchNorm with running variances
    well away from zero, and a residual at the scale of the convolution's output"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((nb, H, W, Cin)).astype(np.float32)
    if nb > 1:
        x[1] *= loud
    w = (rng.standard_normal((N, Cin, k, k)) / np.sqrt(k * k * Cin)).astype(np.float32)
    scale = (1.0 + 0.2 * rng.standard_normal(N)) / np.sqrt(rng.uniform(0.5, 2.0, N) + 1e-5)
    shift = 0.2 * rng.standard_normal(N) - 0.3 * rng.standard_normal(N) * scale
    Ho, Wo = _out_hw(H, W, k, s)
    res = rng.standard_normal((nb, Ho, Wo, N)).astype(np.float32)
    if nb > 1:
        res[1] *= loud
    return x, w, scale, shift, res


def _bordered(x):
    torch = _torch()
    nb, H, W, Cc = x.shape
    xb = torch.zeros((nb, H + 2, W + 2, Cc), device="cuda")
    xb[:, 1:H + 1, 1:W + 1] = torch.from_numpy(x).cuda()
    return xb


def _op(xb, w, scale, shift, res, k, s, act, dst, dst_pad, ldo, bias=None):
    from s3prl_amd import _lib

    lib = _lib.load()
    nb, H, W = xb.shape[0], xb.shape[1] - 2, xb.shape[2] - 2
    N, Cin = w.shape[:2]
    wh = np.ascontiguousarray(w, dtype=np.float32)
    _lib.check(lib.s3enc_op_conv2d_res(_ptr(xb), C.c_void_p(wh.ctypes.data), _ptr(bias), _ptr(scale), _ptr(shift), _ptr(res), nb, H, W, Cin,
                                       N, k, s, act, _ptr(dst), dst_pad, ldo, None), "s3enc_op_conv2d_res")
    _torch().cuda.synchronize()


def _plain(xb, w, scale, shift, res, k, s, act=1):
    """the op into a NaN-filled plain (B, Ho, Wo, N) tensor"""
    torch = _torch()
    Ho, Wo = _out_hw(xb.shape[1] - 2, xb.shape[2] - 2, k, s)
    out = torch.full((xb.shape[0], Ho, Wo, w.shape[0]), float("nan"), device="cuda")
    _op(xb, w, scale, shift, res, k, s, act, out, 0, w.shape[0])
    return out


def _torch_ref(x, w, scale, shift, res, k, s, act, dtype):
    """conv2d -> affine -> + residual -> ReLU in `dtype` on the GPU, channel-last"""
    torch = _torch()
    F = torch.nn.functional
    y = F.conv2d(torch.from_numpy(x).cuda().to(dtype).permute(0, 3, 1, 2), torch.from_numpy(w).cuda().to(dtype), None, stride=s,
                 padding=(k - 1) // 2)
    y = y * torch.from_numpy(scale).cuda().to(dtype)[None, :, None, None] + torch.from_numpy(shift).cuda().to(dtype)[None, :, None, None]
    if res is not None:
        y = y + torch.from_numpy(res).cuda().to(dtype).permute(0, 3, 1, 2)
    if act:
        y = torch.relu(y)
    return y.permute(0, 2, 3, 1).contiguous()


def _check(got, x, w, scale, shift, res, k, s, act, what=()):
    torch = _torch()
    ref = _torch_ref(x, w, scale, shift, res, k, s, act, torch.float64)
    theirs = _torch_ref(x, w, scale.astype(np.float32), shift.astype(np.float32), res, k, s, act, torch.float32)
    nb, Ho, Wo, N = ref.shape
    assert got.shape == ref.shape, (got.shape, ref.shape)
    ours = PR.frame_scores(got.reshape(nb, Ho * Wo, N), ref.reshape(nb, Ho * Wo, N), OP_TOL).cpu().numpy()
    them = PR.frame_scores(theirs.reshape(nb, Ho * Wo, N), ref.reshape(nb, Ho * Wo, N), OP_TOL).cpu().numpy()
    print(f"conv2d_res {what}: worst pixel ours {ours[1]:.2e} theirs {them[1]:.2e}, whole {ours[0]:.2e}, elements off {int(ours[3])}")
    assert ours[1] < max(OP_TOL, 8 * them[1]), (what, ours, them)
    assert ours[3] == 0, (what, ours)


@pytest.mark.parametrize("H, W", MAPS)
def test_every_map_stride_kernel_and_width_per_pixel(H, W):
    for Cin, N, nb in WIDTHS:
        for k in (3, 1):
            for s in (1, 2):
                for with_res in (0, 1):
                    x, w, scale, shift, res = _inputs(nb, H, W, Cin, N, k, s, 1000 * H + 10 * W + Cin + N + nb + 7 * k + s)
                    res = res if with_res else None
                    got = _plain(_bordered(x), w, _dev(scale), _dev(shift), _dev(res), k, s)
                    assert tuple(got.shape[1:3]) == _out_hw(H, W, k, s)
                    _check(got, x, w, scale, shift, res, k, s, 1, what=(H, W, Cin, N, nb, k, s, with_res))


def test_the_released_maps_once():
    """the ResNet's own layer shapes at a few windows: 51 x 32 x 64 at stride 1 with the residual, and each stride-2 entry with its
    1 x 1 shortcut: 51 x 32 -> 26 x 16, 26 x 16 -> 13 x 8, 13 x 8 -> 7 x 4"""
    for H, W, Cin, N, k, s, with_res in [(51, 32, 64, 64, 3, 1, 1), (51, 32, 64, 128, 3, 2, 0), (51, 32, 64, 128, 1, 2, 0),
                                         (26, 16, 128, 256, 3, 2, 0), (13, 8, 256, 512, 1, 2, 0), (7, 4, 512, 512, 3, 1, 1)]:
        x, w, scale, shift, res = _inputs(3, H, W, Cin, N, k, s, 4242 + H + k)
        res = res if with_res else None
        got = _plain(_bordered(x), w, _dev(scale), _dev(shift), _dev(res), k, s)
        _check(got, x, w, scale, shift, res, k, s, 1, what=("released", H, W, Cin, N, k, s, with_res))


@pytest.mark.parametrize("H, W, Cin, N", [(4, 7, 16, 64), (13, 9, 64, 68), (8, 13, 128, 128), (5, 4, 64, 192)])
def test_stride_1_kernel_3_without_a_residual_is_the_affine_entry_bit_for_bit(H, W, Cin, N):
    from s3prl_amd import _lib

    torch = _torch()
    lib = _lib.load()
    x, w, scale, shift, _ = _inputs(5, H, W, Cin, N, 3, 1, 99 + Cin)
    xb, sc, sh = _bordered(x), _dev(scale), _dev(shift)
    wh = np.ascontiguousarray(w, dtype=np.float32)
    for act in (0, 1):
        old = torch.full((5, H, W, N), float("nan"), device="cuda")
        _lib.check(lib.s3enc_op_conv2d3x3_affine(_ptr(xb), C.c_void_p(wh.ctypes.data), None, _ptr(sc), _ptr(sh), 5, H, W, Cin, N, act, 0, 0,
                                                 _ptr(old), 0, N, None), "s3enc_op_conv2d3x3_affine")
        torch.cuda.synchronize()
        assert torch.isfinite(old).all() and torch.equal(_plain(xb, w, sc, sh, None, 3, 1, act), old), act
    bias = _dev(shift)
    old = torch.full((5, H, W, N), float("nan"), device="cuda")
    _lib.check(lib.s3enc_op_conv2d3x3_affine(_ptr(xb), C.c_void_p(wh.ctypes.data), _ptr(bias), None, None, 5, H, W, Cin, N, 1, 0, 0,
                                             _ptr(old), 0, N, None), "s3enc_op_conv2d3x3_affine")
    torch.cuda.synchronize()
    new = torch.full((5, H, W, N), float("nan"), device="cuda")
    _op(xb, w, None, None, None, 3, 1, 1, new, 0, N, bias=bias)
    assert torch.equal(new, old), "a null scale"


@pytest.mark.parametrize("H, W, Cin, N, k, s", [(13, 9, 64, 64, 3, 2), (4, 7, 16, 68, 3, 1), (8, 13, 128, 128, 1, 2), (5, 4, 64, 192, 3, 2)])
def test_an_examples_bits_depend_on_nothing_but_the_example(H, W, Cin, N, k, s):
    """Another B, another batch position (examples start inside a tile and straddle two), enough examples for the tall tiles, and
    the 128-wide n-tile instead of the 64-wide one (tuning key conv2d_n64)."""
    from s3prl_amd import _lib

    torch = _torch()
    lib = _lib.load()
    x, w, scale, shift, res = _inputs(5, H, W, Cin, N, k, s, 1234 + H)
    sc, sh = _dev(scale), _dev(shift)
    run = lambda xs, rs: _plain(_bordered(xs), w, sc, sh, _dev(rs), k, s)  # noqa: E731
    full = run(x, res)
    assert torch.isfinite(full).all()
    assert torch.equal(run(x, res), full)
    for ub in range(5):
        assert torch.equal(run(x[ub:ub + 1], res[ub:ub + 1])[0], full[ub]), ("alone", ub)
    perm = [3, 0, 4, 2, 1]
    permuted = run(x[perm], res[perm])
    for j, i in enumerate(perm):
        assert torch.equal(permuted[j], full[i]), ("permuted", j, i)
    Ho, Wo = _out_hw(H, W, k, s)
    reps = -(-(256 * 300) // (5 * Ho * Wo))  # enough rows for the 256-row tiles on a chip of up to 300 CUs
    many, many_res = np.concatenate([x] * reps)[:5 * reps - 1], np.concatenate([res] * reps)[:5 * reps - 1]
    wide = run(many, many_res)
    assert torch.equal(wide[:5], full) and torch.equal(wide[-4:], full[:4])
    _lib.check(lib.s3enc_set_tuning(b"conv2d_n64", 0), "s3enc_set_tuning")
    try:
        assert torch.equal(run(x, res), full), "the 128-wide n-tile gives other bits"
        assert torch.equal(run(many, many_res)[:5], full)
    finally:
        _lib.check(lib.s3enc_set_tuning(b"conv2d_n64", 1), "s3enc_set_tuning")


@pytest.mark.parametrize("H, W, Cin, N, k, s", [(7, 5, 64, 64, 3, 2), (13, 9, 16, 68, 3, 1), (4, 7, 128, 128, 1, 2)])
def test_border_gap_and_guard_are_untouched(H, W, Cin, N, k, s):
    torch = _torch()
    nb, dp, ldo = 3, 2, N + 8
    x, w, scale, shift, res = _inputs(nb, H, W, Cin, N, k, s, 55 + H)
    Ho, Wo = _out_hw(H, W, k, s)
    body_n = nb * (Ho + 2 * dp) * (Wo + 2 * dp) * ldo
    buf = torch.full((GUARD + body_n + GUARD,), float("nan"), device="cuda")
    body = buf[GUARD:GUARD + body_n].view(nb, Ho + 2 * dp, Wo + 2 * dp, ldo)
    body[:] = 0.0
    body[..., N:] = -7.0
    body[:, dp:dp + Ho, dp:dp + Wo, :N] = float("nan")
    _op(_bordered(x), w, _dev(scale), _dev(shift), _dev(res), k, s, 1, body, dp, ldo)
    assert torch.isnan(buf[:GUARD]).all() and torch.isnan(buf[-GUARD:]).all(), "a guard float of dst was written"
    assert (body[..., N:] == -7.0).all(), "the gap behind a pixel was written"
    inner = torch.zeros((Ho + 2 * dp, Wo + 2 * dp), dtype=torch.bool, device="cuda")
    inner[dp:dp + Ho, dp:dp + Wo] = True
    assert (body[:, ~inner][..., :N] == 0.0).all(), "a border pixel of dst is no longer zero"
    got = body[:, dp:dp + Ho, dp:dp + Wo, :N].contiguous()
    _check(got, x, w, scale, shift, res, k, s, 1, what=("dst", H, W, Cin, N, k, s))
    assert torch.equal(got, _plain(_bordered(x), w, _dev(scale), _dev(shift), _dev(res), k, s))


def test_a_1x1_convolution_never_reads_the_border():
    torch = _torch()
    x, w, scale, shift, _ = _inputs(3, 5, 4, 64, 64, 1, 2, 9)
    xb = _bordered(x)
    want = _plain(xb, w, _dev(scale), _dev(shift), None, 1, 2)
    xb[:, 0] = xb[:, -1] = float("nan")
    xb[:, :, 0] = xb[:, :, -1] = float("nan")
    assert torch.isfinite(want).all() and torch.equal(_plain(xb, w, _dev(scale), _dev(shift), None, 1, 2), want)


def test_refusals_by_message():
    from s3prl_amd import _lib

    torch = _torch()

    def refused(match, Cin=16, N=8, H=4, W=4, k=3, s=1):
        x, w, scale, shift, _ = _inputs(1, H, W, Cin, N, 3 if k not in (1, 3) else k, 1 if s not in (1, 2) else s, 1)
        out = torch.zeros((H * W * N + 8,), device="cuda")
        with pytest.raises(_lib.S3EncError, match=match):
            _op(_bordered(x), w, _dev(scale), _dev(shift), None, k, s, 1, out, 0, N)

    refused("the kernel size must be 3 or 1", k=5)
    refused("the stride must be 1 or 2", s=3)
    refused("Cin must be 1 .* or a multiple of 16", Cin=24)
    refused("Cout must be a multiple of 4", N=6)
