"""s3enc_op_conv_taps on the MI355X, every call through the C ABI: the two-run masked-tap convolution against float64 frame by
frame (every odd mask of k = 15, single runs k = 3 and k = 1, widths below / across / a multiple of the 128-column tile, lengths
below P and either side of the tile heights), the utterance borders under loud neighbours, the untouched border / gap / guard
bytes, the three destinations, the pre-activation residual, and bit for bit where it must be: skip = dense, and a row's bits
depend on nothing but its utterance."""

import ctypes as C

import numpy as np
import pytest

import posconv_ref as PR

pytestmark = pytest.mark.gpu

OP_TOL = 2e-5  # the project's op bound
GUARD = 3      # NaN rows in front of and behind a destination: nothing outside its rows may be written
B = 3


def _torch():
    import torch

    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _inputs(T, Cin, N, k, seed, nb=B, loud=30.0):
    """x with unit variance — utterance 1 is `loud` times louder, so that a read across an utterance border shows in its
    neighbours' first and last P frames — weights 1 / sqrt(live fan-in is not known here: C k), a bias"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((nb, T, Cin)).astype(np.float32)
    if nb > 1:
        x[1] *= loud
    w = (rng.standard_normal((N, Cin, k)) / np.sqrt(Cin * k)).astype(np.float32)
    b = (0.1 * rng.standard_normal(N)).astype(np.float32)
    return x, w, b


def _bordered(x, P, fill=0.0):
    """(B, T, C) host -> device (B, T + 2P, C) with `fill` in the borders"""
    torch = _torch()
    nb, T, Cc = x.shape
    xb = torch.full((nb, T + 2 * P, Cc), fill, device="cuda")
    xb[:, P:P + T] = torch.from_numpy(x).cuda()
    return xb


def _op(xb, w, bias, T, k, mask=0, act=0, res=None, ld_res=0, dst=None, dst_pad=0, ldo=0, state=None, sm=None, sum_init=1, dense=0):
    from s3prl_amd import _lib

    torch = _torch()
    lib = _lib.load()
    N, Cin, _ = w.shape
    wh = np.ascontiguousarray(w, dtype=np.float32)
    _lib.check(lib.s3enc_op_conv_taps(_ptr(xb), C.c_void_p(wh.ctypes.data), _ptr(bias), xb.shape[0], T, Cin, N, k, mask, act, _ptr(res),
                                      ld_res, _ptr(dst), dst_pad, ldo, _ptr(state), _ptr(sm), sum_init, dense, None), "s3enc_op_conv_taps")
    torch.cuda.synchronize()


def _state(xb, w, bias, T, k, **kw):
    torch = _torch()
    out = torch.full((xb.shape[0], T, w.shape[0]), float("nan"), device="cuda")
    _op(xb, w, bias, T, k, state=out, **kw)
    return out


def _masked(w, mask):
    k = w.shape[2]
    wm = w.copy()
    head = (k - mask) // 2
    wm[:, :, head:head + mask] = 0
    return wm


def _ref64(x, w, b, mask, act, res=None):
    """float64 on the GPU: conv1d over the masked weights [+ res], then the activation.  (B, T, N)"""
    torch = _torch()
    k = w.shape[2]
    y = torch.nn.functional.conv1d(torch.from_numpy(x).cuda().double().transpose(1, 2), torch.from_numpy(_masked(w, mask)).cuda().double(),
                                   torch.from_numpy(b).cuda().double(), padding=(k - 1) // 2).transpose(1, 2)
    if res is not None:
        y = y + torch.from_numpy(res).cuda().double()
    return torch.relu(y) if act == 1 else torch.tanh(y) if act == 2 else y


def _theirs(x, w, b, mask, act, res=None):
    """torch.nn.functional.conv1d in CPU fp32 on the same operands"""
    torch = _torch()
    k = w.shape[2]
    y = torch.nn.functional.conv1d(torch.from_numpy(x).transpose(1, 2), torch.from_numpy(_masked(w, mask)), torch.from_numpy(b),
                                   padding=(k - 1) // 2).transpose(1, 2)
    if res is not None:
        y = y + torch.from_numpy(res)
    return torch.relu(y) if act == 1 else torch.tanh(y) if act == 2 else y


def _check(got, x, w, b, mask, act, res=None, what=()):
    """the op rule per frame: ours < max(OP_TOL, 8 theirs), no element off by more than 50 tol (1 + |ref|)"""
    ref = _ref64(x, w, b, mask, act, res)
    ours = PR.frame_scores(got, ref, OP_TOL).cpu().numpy()
    theirs = PR.frame_scores(_theirs(x, w, b, mask, act, res).cuda(), ref, OP_TOL).cpu().numpy()
    print(f"conv_taps {what}: worst frame ours {ours[1]:.2e} (frame {int(ours[2])}) theirs {theirs[1]:.2e}, whole {ours[0]:.2e}, "
          f"elements off {int(ours[3])}")
    assert ours[1] < max(OP_TOL, 8 * theirs[1]), (what, ours, theirs)
    assert ours[3] == 0, (what, ours)
    return ref


@pytest.mark.parametrize("T", [1, 5, 63, 64, 65, 129])
@pytest.mark.parametrize("mask", [0, 1, 3, 5, 7, 9, 11, 13])
def test_every_mask_of_k15_per_frame(mask, T):
    """k = 15, C = 64 -> N = 192 (across the 128-column tile), tanh, three utterances of which the middle one is 30 times louder:
    every frame — the first and last P of every utterance among them — against float64."""
    x, w, b = _inputs(T, 64, 192, 15, 100 * mask + T)
    got = _state(_bordered(x, 7), w, _torch().from_numpy(b).cuda(), T, 15, mask=mask, act=2)
    _check(got, x, w, b, mask, 2, what=("k15", mask, T))


@pytest.mark.parametrize("T", [1, 5, 64, 129])
@pytest.mark.parametrize("Cin, N", [(16, 64), (80, 512), (64, 192), (80, 64)])
@pytest.mark.parametrize("k, mask, act", [(15, 7, 2), (3, 0, 1), (1, 0, 0)])
def test_widths_and_single_runs_per_frame(k, mask, act, Cin, N, T):
    x, w, b = _inputs(T, Cin, N, k, 7000 + 13 * k + Cin + N + T)
    got = _state(_bordered(x, (k - 1) // 2), w, _torch().from_numpy(b).cuda(), T, k, mask=mask, act=act)
    _check(got, x, w, b, mask, act, what=(k, mask, act, Cin, N, T))


@pytest.mark.parametrize("T", [5, 65])
def test_a_read_across_an_utterance_border_would_show(T):
    """The borders hold zeros and the neighbours are loud: the first and last P frames of the quiet utterances stay within the
    bound, and the same call with NaN borders poisons exactly the frames whose live taps reach a border."""
    torch = _torch()
    k, mask, P = 15, 5, 7
    x, w, b = _inputs(T, 64, 64, k, 31 + T, loud=1000.0)
    bias = torch.from_numpy(b).cuda()
    got = _state(_bordered(x, P), w, bias, T, k, mask=mask)
    ref = _check(got, x, w, b, mask, 0, what=("border", T))
    edge = list(range(min(P, T))) + list(range(max(T - P, 0), T))
    for ub in (0, 2):
        sc = PR.frame_scores(got[ub:ub + 1, edge], ref[ub:ub + 1, edge], OP_TOL).cpu().numpy()
        assert sc[1] < OP_TOL and sc[3] == 0, (ub, sc)
    poisoned = _state(_bordered(x, P, fill=float("nan")), w, bias, T, k, mask=mask)
    live = [j - P for j in range(k) if not (k - mask) // 2 <= j < (k + mask) // 2]
    reach = np.array([any(t + o < 0 or t + o >= T for o in live) for t in range(T)])
    nan_rows = torch.isnan(poisoned).any(dim=2).cpu().numpy()
    assert (nan_rows == reach[None, :]).all()
    assert torch.equal(poisoned[:, ~torch.from_numpy(reach).cuda()], got[:, ~torch.from_numpy(reach).cuda()])


@pytest.mark.parametrize("T", [5, 65])
def test_border_rows_gap_and_guard_rows_are_untouched(T):
    torch = _torch()
    k, mask, P, N, dp, ldo = 15, 9, 7, 192, 4, 192 + 8
    x, w, b = _inputs(T, 64, N, k, 55 + T)
    buf = torch.full((GUARD + B * (T + 2 * dp) + GUARD, ldo), float("nan"), device="cuda")
    body = buf[GUARD:GUARD + B * (T + 2 * dp)].view(B, T + 2 * dp, ldo)
    body[:] = -7.0
    st = torch.full((GUARD + B * T + GUARD, N), float("nan"), device="cuda")
    sm = torch.full((GUARD + B * T + GUARD, N), float("nan"), device="cuda")
    _op(_bordered(x, P), w, torch.from_numpy(b).cuda(), T, k, mask=mask, act=2, dst=body, dst_pad=dp, ldo=ldo,
        state=st[GUARD:GUARD + B * T], sm=sm[GUARD:GUARD + B * T], sum_init=1)
    assert torch.isnan(buf[:GUARD]).all() and torch.isnan(buf[-GUARD:]).all(), "a guard row of dst was written"
    for t in (st, sm):
        assert torch.isnan(t[:GUARD]).all() and torch.isnan(t[-GUARD:]).all(), "a guard row was written"
    assert (body[:, :dp] == -7.0).all() and (body[:, dp + T:] == -7.0).all(), "a border row of dst was written"
    assert (body[:, :, N:] == -7.0).all(), "the gap behind a row was written"
    got = body[:, dp:dp + T, :N]
    _check(got, x, w, b, mask, 2, what=("dst", T))
    assert torch.equal(got, st[GUARD:GUARD + B * T].view(B, T, N)) and torch.equal(got, sm[GUARD:GUARD + B * T].view(B, T, N))


def test_three_destinations_in_one_call_equal_three_calls_and_sum_accumulates():
    torch = _torch()
    T, k, mask, P, N = 65, 15, 7, 7, 192
    x, w, b = _inputs(T, 64, N, k, 77)
    xb, bias = _bordered(x, P), torch.from_numpy(b).cuda()
    dst = torch.zeros((B, T + 2 * P, N), device="cuda")
    st = torch.full((B, T, N), float("nan"), device="cuda")
    base = torch.from_numpy(np.random.default_rng(1).standard_normal((B, T, N)).astype(np.float32)).cuda()
    sm = base.clone()
    _op(xb, w, bias, T, k, mask=mask, act=2, dst=dst, dst_pad=P, ldo=N, state=st, sm=sm, sum_init=0)
    d1 = torch.zeros_like(dst)
    _op(xb, w, bias, T, k, mask=mask, act=2, dst=d1, dst_pad=P, ldo=N)
    s1 = _state(xb, w, bias, T, k, mask=mask, act=2)
    m1 = base.clone()
    _op(xb, w, bias, T, k, mask=mask, act=2, sm=m1, sum_init=0)
    assert torch.equal(dst, d1) and torch.equal(st, s1) and torch.equal(sm, m1)
    assert torch.equal(sm, base + st)                  # accumulate: one fp32 addition
    m2 = torch.full((B, T, N), float("nan"), device="cuda")
    _op(xb, w, bias, T, k, mask=mask, act=2, sm=m2, sum_init=1)
    assert torch.equal(m2, st)                         # init: the old contents (NaN) are not read
    assert not dst[:, :P].any() and not dst[:, P + T:].any()


@pytest.mark.parametrize("mask", [1, 5, 7, 13])
@pytest.mark.parametrize("T, N", [(5, 64), (129, 192), (64, 512)])
def test_skip_equals_dense(mask, T, N):
    """gfx950's fp32 MFMA is an fmaf chain: multiplying the masked taps by stored zeros changes no value"""
    x, w, b = _inputs(T, 64, N, 15, 900 + mask + T)
    xb, bias = _bordered(x, 7), _torch().from_numpy(b).cuda()
    skip = _state(xb, w, bias, T, 15, mask=mask, act=2)
    dense = _state(xb, w, bias, T, 15, mask=mask, act=2, dense=1)
    assert np.array_equal(skip.cpu().numpy(), dense.cpu().numpy())
    # and the mask is applied, not trusted: arbitrary values in the hole of the weights change nothing
    w2 = w.copy()
    w2[:, :, (15 - mask) // 2:(15 + mask) // 2] = 1e6
    assert np.array_equal(_state(xb, w2, bias, T, 15, mask=mask, act=2).cpu().numpy(), skip.cpu().numpy())
    assert np.array_equal(_state(xb, w2, bias, T, 15, mask=mask, act=2, dense=1).cpu().numpy(), skip.cpu().numpy())


def test_a_rows_bits_depend_on_nothing_but_its_utterance():
    """Another B, another batch position, another T that moves the row to another tile (and tile height), another n-tile split;
    two runs agree."""
    torch = _torch()
    T, k, mask, P, N = 129, 15, 5, 7, 192
    x, w, b = _inputs(T, 64, N, k, 1234, nb=5)
    bias = torch.from_numpy(b).cuda()
    full = _state(_bordered(x, P), w, bias, T, k, mask=mask, act=2)
    assert torch.isfinite(full).all()
    assert torch.equal(_state(_bordered(x, P), w, bias, T, k, mask=mask, act=2), full)  # run twice
    for ub in (0, 3, 4):
        alone = _state(_bordered(x[ub:ub + 1], P), w, bias, T, k, mask=mask, act=2)
        assert torch.equal(alone[0], full[ub]), ("alone", ub)
    perm = [3, 0, 4, 2, 1]
    permuted = _state(_bordered(x[perm], P), w, bias, T, k, mask=mask, act=2)
    for j, i in enumerate(perm):
        assert torch.equal(permuted[j], full[i]), ("permuted", j, i)
    many = np.concatenate([x] * 60)[:299]  # enough tiles for the 128-row tile where B = 5 runs 64-row tiles (or the reverse)
    wide = _state(_bordered(many, P), w, bias, T, k, mask=mask, act=2)
    assert torch.equal(wide[:5], full) and torch.equal(wide[295:299], full[:4])
    # a longer utterance whose first T rows see the same windows: zeros behind row T + P keep rows [0, T - P) equal
    longer = np.concatenate([x, np.zeros((5, 200, 64), np.float32)], axis=1)
    lg = _state(_bordered(longer, P), w, bias, T + 200, k, mask=mask, act=2)
    assert torch.equal(lg[:, :T], full)  # the rows behind T are zeros, as the border was
    shifted = np.concatenate([np.zeros((5, 70, 64), np.float32), x], axis=1)  # row t moves to row t + 70: another tile, another lane
    sh = _state(_bordered(shifted, P), w, bias, T + 70, k, mask=mask, act=2)
    assert torch.equal(sh[:, 70:], full)
    # the n-tile: the first 64 output channels alone (one narrow tile) against columns [0, 64) of the 192-wide call
    narrow = _state(_bordered(x, P), w[:64], bias[:64].contiguous(), T, k, mask=mask, act=2)
    assert torch.equal(narrow, full[:, :, :64])


@pytest.mark.parametrize("act", [1, 2])
@pytest.mark.parametrize("k, mask", [(1, 0), (15, 5)])
def test_residual_goes_in_before_the_activation(act, k, mask):
    torch = _torch()
    T, N = 65, 192
    x, w, b = _inputs(T, 64, N, k, 4321 + act + k)
    res = (1.5 * np.random.default_rng(act).standard_normal((B, T, N))).astype(np.float32)
    ld_res = N + 4
    dres = torch.full((B, T, ld_res), float("nan"), device="cuda")
    dres[:, :, :N] = torch.from_numpy(res).cuda()
    got = _state(_bordered(x, (k - 1) // 2), w, torch.from_numpy(b).cuda(), T, k, mask=mask, act=act, res=dres, ld_res=ld_res)
    _check(got, x, w, b, mask, act, res, what=("res", act, k))
    after = _ref64(x, w, b, mask, act) + torch.from_numpy(res).cuda().double()  # what launch_gemm's epilogue would give
    assert PR.frame_scores(got, after, OP_TOL).cpu().numpy()[1] > 0.05


def test_tanh_holds_for_tiny_and_saturated_arguments():
    """a k = 1 identity-like conv feeds tanh arguments from 1e-30 to 40: tiny ones come back as themselves, saturated ones as +-1"""
    torch = _torch()
    T, Cn = 64, 64
    args = np.concatenate([np.logspace(-30, -3, 24), np.linspace(0.01, 40.0, 40)]).astype(np.float32)
    x = np.zeros((1, T, Cn), np.float32)
    x[0, :, 0] = args * np.where(np.arange(T) % 2, -1, 1)
    w = np.zeros((64, Cn, 1), np.float32)
    w[np.arange(64), 0, 0] = 1.0  # every output channel copies input channel 0
    got = _state(_bordered(x, 0), w, None, T, 1, act=2).cpu().numpy().astype(np.float64)
    want = np.tanh(x[0, :, :1].astype(np.float64))
    assert np.abs(got[0] - want).max() <= 4 * np.finfo(np.float32).eps
    assert np.all(np.abs(got[0] - want) <= 4 * np.finfo(np.float32).eps * np.abs(want))  # relative: tiny arguments keep their digits
    assert np.abs(got[0][-1]).max() == 1.0
