"""The fp32 positional conv at group widths 24 and 40 (posconv_kernel<24>, <40>: the LightHuBERT subnets, 384 / 640 channels in 16
groups), frame by frame.

These widths are no multiple of the kernel's 16-wide tiles: behind the Dg / 16 full input-channel chunks comes one half chunk of 8
channels (two MFMAs on 8-byte operands) and the last output-channel tile has 8 real columns whose other 8 lanes mirror them and are
never stored.  They have an op entry of their own, s3enc_op_posconv_narrow: s3enc_op_posconv keeps refusing every width but 32, 48
and 64, as tests/test_posconv_edges_gpu.py pins it.  What can go wrong is local to a channel range (the half chunk dropped or read
from the wrong slot, the mirror lanes stored over a neighbour group) as well as to a frame range, so every launch is scored per
frame AND per (batch, group) block against float64 on the operands the kernel sees (tests/posconv_ref.py), with the scorer and the
bands of tests/test_posconv_edges_gpu.py: whole tensor TOL, per frame and per block 2 TOL, per element 50 TOL (1 + |ref|), TOL =
test_ops_gpu.TOL["fp32"].  Every launch writes into a NaN-prefilled buffer with guard rows in front and behind.

On the commit before these widths the entry does not exist and the engine refuses the configuration."""

import ctypes as C
import zlib

import numpy as np
import pytest

from posconv_ref import TAIL, UTT, conv_branch_ref, draw, embed
from test_ops_gpu import TOL, _dev, _ptr, _torch
from test_posconv_edges_gpu import BAND, GUARD, _engine_case, _guards, _Scorer

pytestmark = pytest.mark.gpu

WIDTHS = (24, 40)
T_EDGES = (1, 2, 15, 16, 17, 31, 32, 33, 127, 128, 129, 257)  # MFMA tile 16, wave 32, workgroup 128: -1, +0, +1; three tiles
K_TAPS = (1, 3, 4, 8, 128)
SHIFTS = (0, 1, 16, 17, 127, 128, 129)


def _launch(mode, dx, w, dbias, B, T, D, G, K):
    """One s3enc_op_posconv_narrow into a NaN-prefilled (GUARD + B*T + GUARD, D) buffer; returns (rc, buffer)."""
    torch = _torch()
    from s3prl_amd import _lib

    assert dx.is_contiguous() and tuple(dx.shape) == (B, T, D) and w.flags.c_contiguous and w.shape == (D, D // G, K)
    buf = torch.full((GUARD + B * T + GUARD, D), float("nan"), device="cuda")
    out = C.c_void_p(buf.data_ptr() + GUARD * D * 4)
    rc = _lib.load().s3enc_op_posconv_narrow(_lib.DTYPES[mode], _ptr(dx), w.ctypes.data_as(C.c_void_p), _ptr(dbias), B, T, D, G, K, out, None)
    return rc, buf


def _score_op(sc, mode, x, w, bias, G, what, blocks=False):
    """Launch the op on (x, w, bias) and queue its scores against float64 on the fp32 operands."""
    torch = _torch()
    from s3prl_amd import _lib

    B, T, D = x.shape
    ref = torch.from_numpy(conv_branch_ref(x, w, bias, G)).cuda()
    dx = _dev(x)
    rc, buf = _launch(mode, dx, w, _dev(bias), B, T, D, G, w.shape[2])
    _lib.check(rc, f"s3enc_op_posconv_narrow {what}")
    sc.add(what, buf[GUARD:-GUARD].view(B, T, D).double() - dx.double(), ref, _guards(buf), G if blocks else None)


def test_the_band_is_the_fp32_band_of_the_op_tests():
    assert BAND["fp32"] is TOL["fp32"] or BAND["fp32"] == TOL["fp32"]


@pytest.mark.parametrize("K", (3, 4))
@pytest.mark.parametrize("Dg", WIDTHS)
def test_every_tile_edge_in_T(Dg, K):
    """B = 2, G = 16 (the XCD-aware map): T one below, at and one above every frame tile, at an odd and an even tap count."""
    B, G = 2, 16
    D = G * Dg
    x, w, bias = draw(np.random.default_rng(zlib.crc32(f"pcnarrow/A/{Dg}/{K}".encode())), B, max(T_EDGES), D, G, K)
    sc = _Scorer("narrow-A", "fp32", f"Dg={Dg} K={K}")
    for T in T_EDGES:
        _score_op(sc, "fp32", np.ascontiguousarray(x[:, :T]), w, bias, G, f"Dg {Dg} K {K} T {T}", blocks=True)
    sc.finish()


@pytest.mark.parametrize("Dg", WIDTHS)
def test_every_tap_count(Dg):
    """K = 1 (no double buffering at all), 3, 4, 8 one frame past one and two workgroup tiles; K = 128 (the released width) at T = 129,
    and at T = 17 and 1 where the window reaches past the utterance on both sides."""
    B, G = 2, 16
    D = G * Dg
    sc = _Scorer("narrow-B", "fp32", f"Dg={Dg}")
    cases = [(K, T) for K in K_TAPS[:-1] for T in (129, 257)] + [(128, 129), (128, 17), (128, 1)]
    draws = {}
    for K, T in cases:
        if K not in draws:
            draws[K] = draw(np.random.default_rng(zlib.crc32(f"pcnarrow/B/{Dg}/{K}".encode())), B, 257 if K < 128 else 129, D, G, K)
        x, w, bias = draws[K]
        _score_op(sc, "fp32", np.ascontiguousarray(x[:, :T]), w, bias, G, f"Dg {Dg} K {K} T {T}", blocks=True)
    sc.finish()


@pytest.mark.parametrize("Dg", WIDTHS)
def test_both_work_maps(Dg):
    """G = 16: the XCD-aware map; G = 3: the plain (frame tile, group, batch) order.  B = 1 and 3, two and three frame tiles; a
    mis-mapped (batch, group) shows in its block score."""
    K = 8
    sc = _Scorer("narrow-C", "fp32", f"Dg={Dg}")
    for G in (16, 3):
        D = G * Dg
        x, w, bias = draw(np.random.default_rng(zlib.crc32(f"pcnarrow/C/{Dg}/{G}".encode())), 3, 257, D, G, K)
        for B in (1, 3):
            for T in (130, 257):
                _score_op(sc, "fp32", np.ascontiguousarray(x[:B, :T]), w, bias, G, f"Dg {Dg} G {G} B {B} T {T}", blocks=True)
    sc.finish()


@pytest.mark.parametrize("K", (8, 128))
@pytest.mark.parametrize("Dg", WIDTHS)
def test_frame_bits_do_not_depend_on_the_tile_position(Dg, K):
    """An utterance of 70 frames behind s zero rows: its frames equal the s = 0 run bit for bit (per accumulator the k order is the
    full chunks, then the half chunk, taps ascending — the same in every tile; zero rows add exact zeros).  No tolerance."""
    torch = _torch()
    from s3prl_amd import _lib

    B, G = 2, 16
    D = G * Dg
    u, w, bias = draw(np.random.default_rng(zlib.crc32(f"pcnarrow/D/{Dg}/{K}".encode())), B, UTT, D, G, K)
    dbias = _dev(bias)
    base, flags = None, []
    for s in SHIFTS:
        T = s + UTT + TAIL
        rc, buf = _launch("fp32", _dev(embed(u, s)), w, dbias, B, T, D, G, K)
        _lib.check(rc, f"s3enc_op_posconv_narrow Dg {Dg} K {K} shift {s}")
        got = buf[GUARD:-GUARD].view(B, T, D)[:, s:s + UTT]
        if base is None:
            base = got.clone()
        g_nan, g_fin = _guards(buf)
        ndiff = (got.contiguous().view(torch.int32) != base.view(torch.int32)).any(dim=2).sum().double()
        flags.append(torch.stack([g_nan, g_fin, ndiff]))
    fails = [f"Dg {Dg} K {K} shift {s}: guards kept {g_nan == 1.0}, inside finite {g_fin == 1.0}, {int(ndiff)} of {B * UTT} frames differ"
             for s, (g_nan, g_fin, ndiff) in zip(SHIFTS, torch.stack(flags).cpu().numpy()) if g_nan != 1.0 or g_fin != 1.0 or ndiff != 0]
    print(f"PCNARROW part=D Dg={Dg} K={K} launches={len(SHIFTS)} failures={len(fails)}")
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("D", (384, 640))
def test_engine_posconv_taps(D):
    """The engine's own call (K = conv_pos = 128 with the left padding passed explicitly, the call the 16-bit modes pad with zero taps)
    on a one-layer HuBERT handle of width D in 16 groups: `posconv` minus `proj` per frame against the float64 branch of the `proj`
    tap with the folded weight.  One ragged batch: one frame past two tiles, one past one tile, a single frame."""
    import torch

    from oracle import encoder_oracle as O
    from s3prl_amd.encoder import HipEncoder
    from s3prl_amd.synth import synth_wavs

    frames = (257, 129, 1)
    cfg, weights = _engine_case("tiny_hubert", D, 16, 128)
    lengths = [320 * (t - 1) + 400 for t in frames]
    enc = HipEncoder(cfg, weights, dtype="fp32")
    try:
        hs = enc.forward([torch.from_numpy(w).cuda() for w in synth_wavs(lengths, 78)])
        torch.cuda.synchronize()
        B, T = len(frames), max(frames)
        assert tuple(hs.shape[1:]) == (B, T, D)
        proj = enc.debug_tap("proj").reshape(B, T, D)
        pc = enc.debug_tap("posconv").reshape(B, T, D)
    finally:
        enc.close()
    assert np.isfinite(proj).all() and np.isfinite(pc).all()
    w = O.fold_weight_norm(weights["encoder.pos_conv.0.weight_g"], weights["encoder.pos_conv.0.weight_v"])
    ref = conv_branch_ref(proj, w, weights["encoder.pos_conv.0.bias"], 16)
    sc = _Scorer("narrow-E", "fp32", f"D={D}")
    sc.add(f"engine D {D} G 16 conv_pos 128", torch.from_numpy(pc.astype(np.float64) - proj.astype(np.float64)).cuda(),
           torch.from_numpy(ref).cuda(), None, 16)
    sc.finish()


@pytest.mark.parametrize("mode", ("bf16", "fp16", "fp32x3"))
@pytest.mark.parametrize("Dg", WIDTHS)
def test_the_16_bit_and_split_modes_are_refused_by_name(Dg, mode):
    """posconv16_kernel is not built at 24 and 40: the op says so and writes nothing (K * Dg is a multiple of 128, K even: the shape is
    one the 16-bit kernel would otherwise take)."""
    torch = _torch()
    from s3prl_amd import _lib

    B, T, G, K = 2, 33, 16, 16
    x, w, bias = draw(np.random.default_rng(6), B, T, G * Dg, G, K)
    rc, buf = _launch(mode, _dev(x), w, _dev(bias), B, T, G * Dg, G, K)
    torch.cuda.synchronize()
    msg = _lib.load().s3enc_last_error().decode()
    assert rc != 0 and f"group width {Dg} is built for fp32 only" in msg, (rc, msg)
    assert bool(torch.isnan(buf).all()), "the refused call wrote into the output"


@pytest.mark.parametrize("Dg", (32, 48, 56))
def test_the_other_widths_are_not_this_entry_s(Dg):
    """32 and 48 belong to s3enc_op_posconv, 56 to no kernel: refused by name, nothing written."""
    torch = _torch()
    from s3prl_amd import _lib

    B, T, G, K = 2, 33, 8, 16
    x, w, bias = draw(np.random.default_rng(7), B, T, G * Dg, G, K)
    rc, buf = _launch("fp32", _dev(x), w, _dev(bias), B, T, G * Dg, G, K)
    torch.cuda.synchronize()
    msg = _lib.load().s3enc_last_error().decode()
    assert rc != 0 and "s3enc_op_posconv_narrow: D / groups must be 24 or 40" in msg, (rc, msg)
    assert bool(torch.isnan(buf).all()), "the refused call wrote into the output"
