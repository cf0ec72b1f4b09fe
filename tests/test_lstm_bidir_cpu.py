"""CPU-side checks of the batch-shared bidirectional LSTM op: the symbol is exported, the W_hh packer matches its definition, the
refusals that need no device carry their reason, and the older recurrent ops keep their own limit."""

import ctypes as C

import numpy as np
import pytest


def _lib():
    import os

    from s3prl_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g

        g.build()
    return _lib, _lib.load()


def _vp(a):
    return C.c_void_p(a.ctypes.data)


@pytest.mark.parametrize("H", [64, 192, 1024])
def test_whh_packer_against_its_definition(H):
    """[H / 8 slices][H / 8 k blocks][64 lanes][4]: lane l of slice s, k block kb holds w[(l & 31) / 8 * H + 8 s + (l & 7)][8 kb + 4 (l >> 5) + j]
    — every element of weight_hh exactly once, a slice's 32 gate rows contiguous."""
    _, lib = _lib()
    w = np.arange(4 * H * H, dtype=np.float32).reshape(4 * H, H)  # exact integers below 2^24: every element is its own index
    out = np.full(4 * H * H, -1.0, dtype=np.float32)
    assert lib.s3enc_pack_lstm_bidir_whh(_vp(w), H, _vp(out)) == 0
    s, kb, l, j = np.meshgrid(np.arange(H // 8), np.arange(H // 8), np.arange(64), np.arange(4), indexing="ij")
    want = w[((l & 31) // 8) * H + 8 * s + (l & 7), 8 * kb + 4 * (l >> 5) + j]
    assert np.array_equal(out.reshape(want.shape), want)
    assert np.array_equal(np.sort(out), w.ravel())
    rows = (out.reshape(H // 8, -1) // H).astype(np.int64)  # the rows slice 3 holds: units 24..31 of the four gates
    assert sorted(set(rows[3].tolist())) == sorted(g * H + 24 + u for g in range(4) for u in range(8))


def test_packer_refuses_bad_widths():
    _, lib = _lib()
    one = (C.c_float * 4)()
    assert lib.s3enc_pack_lstm_bidir_whh(one, 96, one) != 0 and b"multiple of 64" in lib.s3enc_last_error()
    assert lib.s3enc_pack_lstm_bidir_whh(one, 1088, one) != 0 and b"at most 1024" in lib.s3enc_last_error()
    assert lib.s3enc_pack_lstm_bidir_whh(None, 64, one) != 0 and b"null" in lib.s3enc_last_error()


def test_op_refuses_before_touching_a_device():
    _, lib = _lib()
    buf = (C.c_float * 64)()
    base = C.addressof(buf)
    base += (-base) % 16
    one = C.c_void_p(base)
    ln = (C.c_int32 * 1)(1)
    lp = C.cast(ln, C.c_void_p)

    def call(H=64, B=1, ld_pre=256, out=one, ldo=128, pre=one, lens=lp):
        return lib.s3enc_op_lstm_bidir(pre, one, one, one, lens, B, 1, H, ld_pre, out, ldo, None)

    assert call(pre=None) != 0 and b"null argument" in lib.s3enc_last_error()
    assert call(lens=None) != 0 and b"null argument" in lib.s3enc_last_error()
    assert call(B=0) != 0 and b"bad shape" in lib.s3enc_last_error()
    assert call(H=96) != 0 and b"multiple of 64" in lib.s3enc_last_error()
    assert call(H=1088) != 0 and b"at most 1024" in lib.s3enc_last_error()
    assert call(B=129) != 0 and b"B above 128" in lib.s3enc_last_error()
    assert call(ld_pre=255) != 0 and b"smaller than the row" in lib.s3enc_last_error()
    assert call(ldo=124) != 0 and b"smaller than the row" in lib.s3enc_last_error()
    assert call(ldo=130) != 0 and b"ldo must be a multiple of 4" in lib.s3enc_last_error()
    assert call(out=C.c_void_p(base + 4)) != 0 and b"16-byte aligned" in lib.s3enc_last_error()
    ln[0] = 2
    assert call() != 0 and b"1..T" in lib.s3enc_last_error()


def test_abi_version_and_the_old_ops_limit_stay():
    """The new op has a limit of its own: the ABI version is still 8 and s3enc_op_rnn / s3enc_op_rnn_len still stop at 512."""
    m, lib = _lib()
    assert lib.s3enc_version() == m.ABI_VERSION == 8
    one = (C.c_float * 4)()
    ln = (C.c_int32 * 1)(1)
    assert lib.s3enc_op_rnn(0, one, one, None, 1, 1, 576, 2304, one, 576, None) != 0 and b"at most 512" in lib.s3enc_last_error()
    assert lib.s3enc_op_rnn_len(0, one, one, None, C.cast(ln, C.c_void_p), None, 0, 1, 1, 576, 2304, one, 576, None) != 0
    assert b"at most 512" in lib.s3enc_last_error()
