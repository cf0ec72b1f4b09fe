"""s3enc_op_lstm_bidir on the MI355X, every call through the C ABI: the batch-shared bidirectional LSTM step against float64 per
utterance and per frame (live rows, zero tails, gap and guard bytes), the backward half on ragged lengths, and bit for bit where it
must be — an utterance's rows depend on nothing but the utterance."""

import ctypes as C

import numpy as np
import pytest

from oracle import encoder_oracle as O

import cpc_ref

pytestmark = pytest.mark.gpu

FP32_TOL = 1e-4  # the project's fixture bound (tests/test_apc_gpu.py)
GUARD = 3        # NaN rows in front of and behind an output buffer: nothing outside the B * T rows may be written
T = 9


def _torch():
    import torch

    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def _dev(x):
    return _torch().from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda()


def _lens(B):
    """1, T and ragged middles; for B = 1 the ragged 5 (so that len - 1 - t differs from T - 1 - t)"""
    base = [5, T, 1, 7, 2, 8, 3, 6, 4]
    return [base[b % len(base)] for b in range(B)]


def _inputs(B, H, seed):
    """pre with a standard deviation of 2 (gates far outside their linear range), recurrent weights 1.5 / sqrt(H)"""
    rng = np.random.default_rng(seed)
    pre = (2.0 * rng.standard_normal((2, B, T, 4 * H))).astype(np.float32)
    w = (rng.standard_normal((2, 4 * H, H)) * (1.5 / np.sqrt(H))).astype(np.float32)
    return pre, w


def _op(pre_f, pre_b, w, lens, B, H, ld_pre=None, out=None, ldo=None, t_rows=T):
    from s3prl_amd import _lib

    torch = _torch()
    lib = _lib.load()
    ld_pre, ldo = ld_pre or 4 * H, ldo or 2 * H
    if out is None:
        out = torch.full((B, t_rows, ldo), float("nan"), device="cuda")
    wf, wb = np.ascontiguousarray(w[0], dtype=np.float32), np.ascontiguousarray(w[1], dtype=np.float32)
    ln = (C.c_int32 * B)(*lens)
    _lib.check(lib.s3enc_op_lstm_bidir(_ptr(pre_f), _ptr(pre_b), C.c_void_p(wf.ctypes.data), C.c_void_p(wb.ctypes.data),
                                       C.cast(ln, C.c_void_p), B, t_rows, H, ld_pre, _ptr(out), ldo, None), "s3enc_op_lstm_bidir")
    torch.cuda.synchronize()
    return out


def _ref64(pre, w, lens):
    """float64 per utterance over its own length: the forward stack as it stands, the backward stack on the utterance's rows
    flipped and flipped back (the reference's flipBatch); zeros behind the length.  -> (B, T, 2H)"""
    _, B, Tn, H4 = pre.shape
    H = H4 // 4
    out = np.zeros((B, Tn, 2 * H))
    for b, n in enumerate(lens):
        out[b, :n, :H] = cpc_ref.lstm_from_pre(pre[0, b:b + 1, :n].astype(np.float64), w[0].astype(np.float64))[0]
        out[b, :n, H:] = cpc_ref.lstm_from_pre(pre[1, b:b + 1, :n][:, ::-1].astype(np.float64), w[1].astype(np.float64))[0][::-1]
    return out


@pytest.mark.parametrize("B", [1, 3, 33, 65])  # 33 / 65: one utterance past a 32-wide batch tile, two and four tiles per workgroup
@pytest.mark.parametrize("H", [64, 192, 1024])  # 192: two k blocks per register stage instead of four
def test_lstm_bidir_op_against_float64(H, B):
    """T = 9, lengths with 1, T and ragged middles, row strides larger than the rows: every live row within FP32_TOL of float64, per
    utterance and per frame and per half; tail rows exactly 0 in both halves; the gap behind a row and the guard rows untouched."""
    torch = _torch()
    lens = _lens(B)
    pre, w = _inputs(B, H, 9000 + 10 * H + B)
    ld_pre, ldo = 4 * H + 12, 2 * H + 8
    dpre = torch.full((2, B, T, ld_pre), float("nan"), device="cuda")
    dpre[..., :4 * H] = _dev(pre)
    out = torch.full((GUARD + B * T + GUARD, ldo), float("nan"), device="cuda")
    body = out[GUARD:GUARD + B * T].view(B, T, ldo)
    body[:, :, 2 * H:] = -7.0
    _op(dpre[0], dpre[1], w, lens, B, H, ld_pre=ld_pre, out=body, ldo=ldo)
    h = out.cpu().numpy()
    assert np.isnan(h[:GUARD]).all() and np.isnan(h[-GUARD:]).all(), "a guard row was written"
    got = h[GUARD:-GUARD].reshape(B, T, ldo)
    assert (got[:, :, 2 * H:] == -7.0).all(), "the gap behind a row was written"
    got = got[:, :, :2 * H]
    ref = _ref64(pre, w, lens)
    worst_u = worst_f = 0.0
    for b, n in enumerate(lens):
        assert np.array_equal(got[b, n:], np.zeros((T - n, 2 * H), dtype=np.float32)), (b, "tail rows must be exactly 0 in both halves")
        for half, sl in (("fwd", slice(0, H)), ("bwd", slice(H, 2 * H))):
            eu = O.rel_err(got[b, :n, sl], ref[b, :n, sl])
            ef = max(O.rel_err(got[b, t, sl], ref[b, t, sl]) for t in range(n))
            worst_u, worst_f = max(worst_u, eu), max(worst_f, ef)
            assert eu < FP32_TOL and ef < FP32_TOL, (H, B, b, n, half, eu, ef)
    print(f"lstm_bidir H={H} B={B}: worst per utterance {worst_u:.2e}, worst per frame {worst_f:.2e}")


def test_backward_half_runs_from_each_utterances_own_last_row():
    """Two utterances with the SAME pre rows and different lengths: the backward half of the shorter one must equal a run of its
    own rows alone at T = its length (where len - 1 - t and T - 1 - t coincide), and must differ from the longer one's rows."""
    torch = _torch()
    H, n = 64, 4
    pre, w = _inputs(1, H, 9100)
    pre2 = np.concatenate([pre, pre], axis=1)  # (2, B = 2, T, 4H)
    d2 = _dev(pre2)
    both = _op(d2[0], d2[1], w, [T, n], 2, H)
    short = _op(_dev(pre[0][:, :n]), _dev(pre[1][:, :n]), w, [n], 1, H, t_rows=n)
    assert torch.isfinite(both[1, :n]).all()
    assert torch.equal(both[1, :n], short[0])
    assert torch.equal(both[1, :n, :H], both[0, :n, :H]), "the forward halves see the same rows"
    assert not torch.equal(both[1, :n, H:], both[0, :n, H:]), "the backward halves start from different rows"
    ref = _ref64(pre2, w, [T, n])
    assert O.rel_err(both[1, :n, H:].cpu().numpy(), ref[1, :n, H:]) < FP32_TOL


@pytest.mark.parametrize("H", [128, 1024])
def test_an_utterances_rows_depend_on_nothing_but_the_utterance(H):
    """Bit for bit: utterances of a B = 33 ragged batch equal the same utterance run alone, run at T = its own length, at another
    batch position (another column of another batch tile), in a four-tile batch and next to other lengths; two runs agree."""
    torch = _torch()
    B = 33
    lens = _lens(B)
    pre, w = _inputs(B, H, 9200 + H)
    d = _dev(pre)
    full = _op(d[0], d[1], w, lens, B, H)
    assert torch.isfinite(full).all()
    assert torch.equal(_op(d[0], d[1], w, lens, B, H), full)  # run twice
    for b in (0, 1, 2, 13, 31, 32):
        n = lens[b]
        alone = _op(d[0, b:b + 1].contiguous(), d[1, b:b + 1].contiguous(), w, [n], 1, H)
        assert torch.equal(alone[0], full[b]), ("alone", b)
        short = _op(d[0, b:b + 1, :n].contiguous(), d[1, b:b + 1, :n].contiguous(), w, [n], 1, H, t_rows=n)
        assert torch.equal(short[0], full[b, :n]), ("T = its own length", b)
    perm = np.roll(np.arange(B), 7)[::-1].copy()  # 32 -> a column of the first tile, 0 .. -> elsewhere
    idx = torch.from_numpy(perm).cuda()
    permuted = _op(d[0][idx].contiguous(), d[1][idx].contiguous(), w, [lens[i] for i in perm], B, H)
    for j, i in enumerate(perm):
        assert torch.equal(permuted[j], full[i]), ("permuted", j, i)
    big = torch.cat([d, d], dim=1)[:, :65].contiguous()  # B = 65: four batch tiles, utterance b again at column 33 + b
    bl = (lens + lens)[:65]
    wide = _op(big[0], big[1], w, bl, 65, H)
    assert torch.equal(wide[:33], full) and torch.equal(wide[33:65], full[:32])
    other = [T if n != T else 2 for n in lens]  # every other length changes; utterance 5 keeps its own
    other[5] = lens[5]
    assert torch.equal(_op(d[0], d[1], w, other, B, H)[5], full[5])


def test_refusals_name_their_reason():
    from s3prl_amd import _lib

    torch = _torch()
    lib = _lib.load()
    H, B = 64, 2
    pre, w = _inputs(B, H, 9300)
    d = _dev(pre)
    out = torch.zeros((B, T, 2 * H + 4), device="cuda")
    wf = np.ascontiguousarray(w[0])
    wp = C.c_void_p(wf.ctypes.data)

    base = out.data_ptr()

    def call(lens=(T, 3), Bn=B, Hn=H, ld_pre=4 * H, o=base, ldo=2 * H):
        ln = (C.c_int32 * len(lens))(*lens)
        return lib.s3enc_op_lstm_bidir(_ptr(d[0]), _ptr(d[1]), wp, wp, C.cast(ln, C.c_void_p), Bn, T, Hn, ld_pre, C.c_void_p(o), ldo, None)

    assert call() == 0
    assert call(Hn=96) != 0 and b"multiple of 64" in lib.s3enc_last_error()
    assert call(Hn=1088) != 0 and b"at most 1024" in lib.s3enc_last_error()
    assert call(o=base + 4) != 0 and b"16-byte aligned" in lib.s3enc_last_error()
    assert call(o=base, ldo=2 * H + 2) != 0 and b"ldo must be a multiple of 4" in lib.s3enc_last_error()
    assert call(o=base, ldo=2 * H - 4) != 0 and b"smaller than the row" in lib.s3enc_last_error()
    assert call(o=base, ld_pre=4 * H - 1) != 0 and b"smaller than the row" in lib.s3enc_last_error()
    assert call(o=base, lens=(T + 1, 3)) != 0 and b"1..T" in lib.s3enc_last_error()
    assert call(o=base, lens=(0, 3)) != 0 and b"1..T" in lib.s3enc_last_error()
    assert call(o=base, lens=(1,) * 129, Bn=129) != 0 and b"B above 128" in lib.s3enc_last_error()
