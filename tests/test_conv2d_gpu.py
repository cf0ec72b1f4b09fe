"""s3enc_op_conv2d3x3 on the MI355X, every call through the C ABI: the 3 x 3 / padding-1 convolution with bias -> ReLU -> optional
2 x 2 max-pool against float64 pixel by pixel (maps of fewer pixels than one MFMA tile, exactly one tile, a ragged last tile; widths
below / at / across the 128-column tile; Cin of one to eight 64-byte steps per tap), corner / edge / interior pixels scored as
separate groups under a loud neighbour, the untouched border / gap / guard bytes of the destination, and bit for bit where it must
be: an example's bits depend on nothing but the example, and the pooled output is the max over the un-pooled output of the same
op.  The Cin = 1 first-layer kernel gets the same treatment."""

import ctypes as C

import numpy as np
import pytest

import posconv_ref as PR

pytestmark = pytest.mark.gpu

OP_TOL = 2e-5  # the project's op bound
GUARD = 64     # NaN floats in front of and behind a destination: nothing outside it may be written

MAPS = [(2, 2), (4, 2), (6, 4), (12, 8), (10, 6), (24, 16)]
# every Cin of 16 / 48 / 64 / 128, every Cout of 4 / 64 / 96 / 128 / 192 and every B of 1 / 3 / 5 at least once
WIDTHS = [(16, 4, 1), (48, 64, 3), (64, 96, 5), (128, 128, 3), (64, 192, 1), (16, 128, 5), (128, 192, 3)]


def _torch():
    import torch

    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _inputs(nb, H, W, Cin, N, seed, loud=30.0):
    """channel-last images of unit variance — example 1 is `loud` times louder, so that a read across an example's border shows
    in its neighbours — weights 1 / sqrt(9 Cin), a bias"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((nb, H, W, Cin)).astype(np.float32)
    if nb > 1:
        x[1] *= loud
    w = (rng.standard_normal((N, Cin, 3, 3)) / np.sqrt(9 * Cin)).astype(np.float32)
    b = (0.1 * rng.standard_normal(N)).astype(np.float32)
    return x, w, b


def _bordered(x, fill=0.0):
    """(B, H, W, C) host -> device (B, H + 2, W + 2, C) with `fill` in the border"""
    torch = _torch()
    nb, H, W, Cc = x.shape
    xb = torch.full((nb, H + 2, W + 2, Cc), fill, device="cuda")
    xb[:, 1:H + 1, 1:W + 1] = torch.from_numpy(x).cuda()
    return xb


def _op(xb, w, bias, act, pool, dst, dst_pad, ldo):
    from s3prl_amd import _lib

    lib = _lib.load()
    nb, H, W = xb.shape[0], xb.shape[1] - 2, xb.shape[2] - 2
    N, Cin = w.shape[:2]
    wh = np.ascontiguousarray(w, dtype=np.float32)
    _lib.check(lib.s3enc_op_conv2d3x3(_ptr(xb), C.c_void_p(wh.ctypes.data), _ptr(bias), nb, H, W, Cin, N, act, pool, _ptr(dst), dst_pad,
                                      ldo, None), "s3enc_op_conv2d3x3")
    _torch().cuda.synchronize()


def _plain(xb, w, bias, act=1, pool=0):
    """the op into a NaN-filled plain (B, Ho, Wo, N) tensor"""
    torch = _torch()
    H, W = xb.shape[1] - 2, xb.shape[2] - 2
    out = torch.full((xb.shape[0], H >> pool, W >> pool, w.shape[0]), float("nan"), device="cuda")
    _op(xb, w, bias, act, pool, out, 0, w.shape[0])
    return out


def _torch_conv(x, w, b, act, pool, dtype):
    """torch's conv2d (+ ReLU, + max_pool2d) on the GPU in `dtype`, channel-last (B, Ho, Wo, N)"""
    torch = _torch()
    F = torch.nn.functional
    y = F.conv2d(torch.from_numpy(x).cuda().to(dtype).permute(0, 3, 1, 2), torch.from_numpy(w).cuda().to(dtype),
                 torch.from_numpy(b).cuda().to(dtype), padding=1)
    if act:
        y = torch.relu(y)
    if pool:
        y = F.max_pool2d(y, 2, 2)
    return y.permute(0, 2, 3, 1).contiguous()


def _groups(Ho, Wo):
    """flat pixel indices of the corner, edge and interior pixels of an Ho x Wo map"""
    yy, xx = np.meshgrid(np.arange(Ho), np.arange(Wo), indexing="ij")
    ey, ex = (yy == 0) | (yy == Ho - 1), (xx == 0) | (xx == Wo - 1)
    flat = lambda m: np.flatnonzero(m.reshape(-1))
    return {"corner": flat(ey & ex), "edge": flat((ey | ex) & ~(ey & ex)), "interior": flat(~(ey | ex))}


def _check(got, x, w, b, act, pool, what=()):
    """the op rule per pixel and per group of pixels: ours < max(OP_TOL, 8 theirs), no element off by more than 50 tol (1 + |ref|)"""
    torch = _torch()
    ref = _torch_conv(x, w, b, act, pool, torch.float64)
    theirs = _torch_conv(x, w, b, act, pool, torch.float32)
    nb, Ho, Wo, N = ref.shape
    assert got.shape == ref.shape, (got.shape, ref.shape)
    g3, r3, t3 = got.reshape(nb, Ho * Wo, N), ref.reshape(nb, Ho * Wo, N), theirs.reshape(nb, Ho * Wo, N)
    for name, idx in _groups(Ho, Wo).items():
        if not len(idx):
            continue
        sel = torch.from_numpy(idx).cuda()
        ours = PR.frame_scores(g3[:, sel], r3[:, sel], OP_TOL).cpu().numpy()
        them = PR.frame_scores(t3[:, sel], r3[:, sel], OP_TOL).cpu().numpy()
        print(f"conv2d3x3 {what} {name}: worst pixel ours {ours[1]:.2e} theirs {them[1]:.2e}, whole {ours[0]:.2e}, elements off {int(ours[3])}")
        assert ours[1] < max(OP_TOL, 8 * them[1]), (what, name, ours, them)
        assert ours[3] == 0, (what, name, ours)
    return ref


@pytest.mark.parametrize("pool", [0, 1])
@pytest.mark.parametrize("H, W", MAPS)
def test_every_map_and_width_per_pixel(H, W, pool):
    torch = _torch()
    for Cin, N, nb in WIDTHS:
        x, w, b = _inputs(nb, H, W, Cin, N, 1000 * H + 10 * W + Cin + N + nb + pool)
        got = _plain(_bordered(x), w, torch.from_numpy(b).cuda(), 1, pool)
        _check(got, x, w, b, 1, pool, what=(H, W, Cin, N, nb, pool))


@pytest.mark.parametrize("pool", [0, 1])
def test_no_activation_and_no_bias(pool):
    torch = _torch()
    x, w, b = _inputs(3, 10, 6, 48, 96, 5 + pool)
    got = _plain(_bordered(x), w, None, 0, pool)
    _check(got, x, w, np.zeros_like(b), 0, pool, what=("linear", pool))
    assert (got < 0).any()


@pytest.mark.parametrize("pool", [0, 1])
def test_a_read_across_an_example_border_would_show(pool):
    """The border holds zeros and the neighbour is loud (the groups of _check); the same call with a NaN border poisons exactly the
    outputs whose taps reach the border."""
    torch = _torch()
    H, W = 12, 8
    x, w, b = _inputs(3, H, W, 64, 64, 31 + pool, loud=1000.0)
    bias = torch.from_numpy(b).cuda()
    got = _plain(_bordered(x), w, bias, 1, pool)
    _check(got, x, w, b, 1, pool, what=("border", pool))
    poisoned = _plain(_bordered(x, fill=float("nan")), w, bias, 1, pool)
    Ho, Wo = H >> pool, W >> pool
    g = _groups(Ho, Wo)
    reach = np.zeros(Ho * Wo, bool)
    reach[np.concatenate([g["corner"], g["edge"]])] = True
    nan_px = torch.isnan(poisoned).any(dim=3).reshape(3, -1).cpu().numpy()
    assert (nan_px == reach[None, :]).all()
    keep = torch.from_numpy(~reach).cuda()
    assert torch.equal(poisoned.reshape(3, Ho * Wo, -1)[:, keep], got.reshape(3, Ho * Wo, -1)[:, keep])


@pytest.mark.parametrize("pool", [0, 1])
@pytest.mark.parametrize("H, W, Cin, N", [(6, 4, 64, 96), (24, 16, 16, 192), (16, 16, 1, 64)])
def test_border_pixels_gap_and_guard_are_untouched(H, W, Cin, N, pool):
    torch = _torch()
    nb, dp, ldo = 3, 2, N + 8
    x, w, b = _inputs(nb, H, W, Cin, N, 55 + H + pool)
    Ho, Wo = H >> pool, W >> pool
    body_n = nb * (Ho + 2 * dp) * (Wo + 2 * dp) * ldo
    buf = torch.full((GUARD + body_n + GUARD,), float("nan"), device="cuda")
    body = buf[GUARD:GUARD + body_n].view(nb, Ho + 2 * dp, Wo + 2 * dp, ldo)
    body[:] = 0.0
    body[..., N:] = -7.0
    body[:, dp:dp + Ho, dp:dp + Wo, :N] = float("nan")
    _op(_bordered(x), w, torch.from_numpy(b).cuda(), 1, pool, body, dp, ldo)
    assert torch.isnan(buf[:GUARD]).all() and torch.isnan(buf[-GUARD:]).all(), "a guard float of dst was written"
    assert (body[..., N:] == -7.0).all(), "the gap behind a pixel was written"
    inner = torch.zeros((Ho + 2 * dp, Wo + 2 * dp), dtype=torch.bool, device="cuda")
    inner[dp:dp + Ho, dp:dp + Wo] = True
    assert (body[:, ~inner][..., :N] == 0.0).all(), "a border pixel of dst is no longer zero"
    got = body[:, dp:dp + Ho, dp:dp + Wo, :N].contiguous()
    _check(got, x, w, b, 1, pool, what=("dst", H, W, Cin, N, pool))
    assert torch.equal(got, _plain(_bordered(x), w, torch.from_numpy(b).cuda(), 1, pool))


@pytest.mark.parametrize("H, W, Cin, N", [(2, 2, 16, 4), (6, 4, 48, 96), (12, 8, 64, 192), (10, 6, 128, 128), (16, 16, 1, 64)])
def test_pooled_equals_the_max_over_the_unpooled_output(H, W, Cin, N):
    torch = _torch()
    x, w, b = _inputs(3, H, W, Cin, N, 77 + H)
    xb, bias = _bordered(x), torch.from_numpy(b).cuda()
    for act in (0, 1):
        full = _plain(xb, w, bias, act, 0)
        pooled = _plain(xb, w, bias, act, 1)
        want = torch.nn.functional.max_pool2d(full.permute(0, 3, 1, 2), 2, 2).permute(0, 2, 3, 1)
        assert torch.equal(pooled, want), (act, H, W, Cin, N)


@pytest.mark.parametrize("pool", [0, 1])
@pytest.mark.parametrize("H, W, Cin, N", [(12, 8, 64, 192), (6, 4, 48, 96), (16, 16, 1, 64)])
def test_an_examples_bits_depend_on_nothing_but_the_example(H, W, Cin, N, pool):
    """Another B, another batch position (an example starts in the middle of a tile and straddles two), the 128-row tile where B = 5
    runs 64-row tiles, another n-tile split; two runs agree."""
    torch = _torch()
    x, w, b = _inputs(5, H, W, Cin, N, 1234 + H + pool)
    bias = torch.from_numpy(b).cuda()
    full = _plain(_bordered(x), w, bias, 1, pool)
    assert torch.isfinite(full).all()
    assert torch.equal(_plain(_bordered(x), w, bias, 1, pool), full)  # run twice
    for ub in range(5):
        alone = _plain(_bordered(x[ub:ub + 1]), w, bias, 1, pool)
        assert torch.equal(alone[0], full[ub]), ("alone", ub)
    perm = [3, 0, 4, 2, 1]
    permuted = _plain(_bordered(x[perm]), w, bias, 1, pool)
    for j, i in enumerate(perm):
        assert torch.equal(permuted[j], full[i]), ("permuted", j, i)
    reps = -(-(128 * 2 * 300) // (5 * H * W))  # enough pixels for the 128-row tiles on a chip of up to 300 CUs
    many = np.concatenate([x] * reps)[:5 * reps - 1]
    wide = _plain(_bordered(many), w, bias, 1, pool)
    assert torch.equal(wide[:5], full) and torch.equal(wide[-4:], full[:4])
    narrow = _plain(_bordered(x), w[:N // 2], bias[:N // 2].contiguous(), 1, pool)
    assert torch.equal(narrow, full[..., :N // 2])


@pytest.mark.parametrize("pool", [0, 1])
@pytest.mark.parametrize("H, W", [(16, 16), (96, 64)])
def test_first_layer_per_pixel(H, W, pool):
    torch = _torch()
    x, w, b = _inputs(3, H, W, 1, 64, 9 + H + pool)
    got = _plain(_bordered(x), w, torch.from_numpy(b).cuda(), 1, pool)
    _check(got, x, w, b, 1, pool, what=("first", H, W, pool))


def test_a_nan_stays_a_nan():
    torch = _torch()
    for Cin in (1, 16):
        x, w, b = _inputs(1, 4, 4, Cin, 8, 3 + Cin)
        x[0, 1, 1, 0] = np.nan
        for pool in (0, 1):
            got = _plain(_bordered(x), w, torch.from_numpy(b).cuda(), 1, pool)
            nan_px = torch.isnan(got).all(dim=3)[0].cpu().numpy()
            want = np.zeros((4, 4), bool)
            want[0:3, 0:3] = True
            if pool:
                want = want.reshape(2, 2, 2, 2).any(axis=(1, 3))
            assert (nan_px == want).all(), (Cin, pool, nan_px)


def test_refusals_by_message():
    from s3prl_amd import _lib

    torch = _torch()

    def refused(match, Cin=16, N=8, H=4, W=4, act=1, pool=0, ldo=None, off=0, dp=0):
        x, w, b = _inputs(1, H, W, Cin, N, 1)
        xb = _bordered(x)
        out = torch.zeros(((H + 2 * dp) * (W + 2 * dp) * (ldo or N) + 8,), device="cuda")
        with pytest.raises(_lib.S3EncError, match=match):
            _op(xb, w, torch.from_numpy(b).cuda(), act, pool, out[off:], dp, ldo or N)

    refused("Cin must be 1 .* or a multiple of 16", Cin=24)
    refused("Cout must be a multiple of 4", N=6, ldo=8)
    refused("H and W must be even under pool", H=5, pool=1)
    refused("H and W must be even under pool", W=3, pool=1)
    refused("16-byte aligned", off=1)
    refused("pixel pitch is smaller than Cout", ldo=4)
    refused("act must be", act=2)
    refused("pool must be", pool=2)
