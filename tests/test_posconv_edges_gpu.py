"""Frame edges, K pipelines and work maps of the positional conv (posconv.hip), frame by frame.

posconv_kernel<32|48|64> (exact fp32, 128 frames per workgroup, 32 per wave, 16 per MFMA tile), posconv16_kernel (bf16 / fp16,
256 frames per workgroup, 64 per wave, one weight stage per 128 k) and its split-precision X3 form (128 frames) have tile-local
paths that a whole-tensor score cannot see: one tap dropped on the last frames of a tile, a wrong weight stage when K * Dg / 128 is
1 or odd, a mis-mapped (batch, group) block.  tests/test_ops_gpu.py::test_posconv scores four shapes once each.  These tests run
s3enc_op_posconv (and, in part E, the engine's own zero-tap-padded call) at every tile edge in T, every stage count, both work maps,
and score EVERY FRAME on its own against float64 on the operands the kernel sees (tests/posconv_ref.py, pinned on the CPU by
tests/test_posconv_ref_cpu.py).

Bands.  The reference is built from the operands the kernel sees (x and w rounded to the operand type, fp32 bias; fp32x3 splits the
unrounded operands), so in every mode the only error left is fp32 accumulation: bf16 and fp16 are held to the fp32 band, as
test_col_edges_gpu.py holds the 16-bit GEMMs (`SHARP`).  Whole tensor TOL, per frame 2 * TOL, per element 50 * TOL * (1 + |ref|),
TOL = TOL["fp32"] = 2e-5 (fp32x3: TOL["fp32x3"] = 4e-5).  torch's CPU fp32 conv1d on the same operands is about 4e-7 per frame from
float64 on these shapes, so the bands leave roughly 50x for a different summation order — and none for a dropped tap (8e-3).

Every launch writes into a NaN-prefilled buffer with three guard rows in front and behind: the guards stay NaN, every row inside
is finite.  Scores are computed on the device; a test id makes one host copy."""

import ctypes as C
import zlib

import numpy as np
import pytest

from posconv_ref import TAIL, UTT, conv_branch_ref, draw, embed, frame_scores
from test_ops_gpu import TOL, _dev, _ptr, _round, _torch

pytestmark = pytest.mark.gpu

MODES = ("fp32", "bf16", "fp16", "fp32x3")
BAND = {"fp32": TOL["fp32"], "bf16": TOL["fp32"], "fp16": TOL["fp32"], "fp32x3": TOL["fp32x3"]}
GUARD = 3  # NaN rows in front of and behind every output

# part A: 16 / 32 / 64 / 128 / 256 frames (MFMA tile, fp32 wave, 16-bit wave, fp32 / X3 workgroup, 16-bit workgroup) -1, +0, +1
T_EDGES = (1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 385)
# part B: K per Dg with 1, 2, 3 and many weight stages of 128 k (stage count K * Dg / 128); odd K: fp32 only, nothing is trimmed
K_STAGES = {32: (4, 8, 12, 16, 128), 48: (8, 16, 24, 128), 64: (2, 4, 6, 16, 128)}
K_ODD = (1, 3, 15, 31)
# part D: offsets of the embedded utterance
SHIFTS = (0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 255, 256, 257)
SHIFTS_K128 = (0, 63, 64, 129, 257)


def _launch(mode, dx, w, dbias, B, T, D, G, K):
    """One s3enc_op_posconv into a NaN-prefilled (GUARD + B*T + GUARD, D) buffer; returns (rc, buffer)."""
    torch = _torch()
    from s3prl_amd import _lib

    lib = _lib.load()
    assert dx.is_contiguous() and tuple(dx.shape) == (B, T, D) and w.flags.c_contiguous and w.shape == (D, D // G, K)
    buf = torch.full((GUARD + B * T + GUARD, D), float("nan"), device="cuda")
    out = C.c_void_p(buf.data_ptr() + GUARD * D * 4)
    rc = lib.s3enc_op_posconv(_lib.DTYPES[mode], _ptr(dx), w.ctypes.data_as(C.c_void_p), _ptr(dbias), B, T, D, G, K, out, None)
    return rc, buf


def _guards(buf):
    """(guard rows all NaN, rows inside all finite) as two device scalars."""
    torch = _torch()
    return (torch.isnan(buf[:GUARD]).all() & torch.isnan(buf[-GUARD:]).all()).double(), torch.isfinite(buf[GUARD:-GUARD]).all().double()


class _Scorer:
    """Queues the device-side scores of the launches of one test id; finish() copies them once, prints the worst values and asserts."""

    def __init__(self, part, mode, tag):
        self.part, self.mode, self.tag, self.tol = part, mode, tag, BAND[mode]
        self.names, self.stats = [], []

    def add(self, what, branch, ref, guards=None, G=None):
        """branch: (B, T, D) fp32 or float64 on the device, the conv branch (output minus residual); ref: float64, same shape."""
        torch = _torch()
        g_nan, g_fin = guards if guards is not None else (torch.ones((), device="cuda", dtype=torch.float64),) * 2
        self.stats.append(torch.cat([frame_scores(branch, ref, self.tol, G), torch.stack([g_nan, g_fin])]))
        T = ref.shape[1]
        self.names.append((what, T, G))

    def finish(self):
        torch = _torch()
        rows = torch.stack(self.stats).cpu().numpy()
        fails, w_all, w_fr = [], 0.0, 0.0
        for (what, T, G), (whole, fmax, farg, nbad, bmax, barg, g_nan, g_fin) in zip(self.names, rows):
            b, t = divmod(int(farg), T)
            where = f"worst frame (b {b}, t {t}; t % 16 / 64 / 128 / 256 = {t % 16} / {t % 64} / {t % 128} / {t % 256}) {fmax:.3e}"
            if g_nan != 1.0:
                fails.append(f"{what}: a guard row in front of or behind the output was written")
            if g_fin != 1.0:
                fails.append(f"{what}: NaN / inf inside the output (a row left unwritten?); {where}")
            if not whole <= self.tol:
                fails.append(f"{what}: whole tensor {whole:.3e} > {self.tol:.1e}; {where}")
            if not fmax <= 2.0 * self.tol:
                fails.append(f"{what}: {where} > {2.0 * self.tol:.1e}")
            if nbad != 0:
                fails.append(f"{what}: {int(nbad)} elements off by more than 50 * {self.tol:.1e} * (1 + |ref|); {where}")
            if G and not bmax <= 2.0 * self.tol:
                fails.append(f"{what}: (batch {int(barg) // G}, group {int(barg) % G}) block {bmax:.3e} > {2.0 * self.tol:.1e}")
            w_all, w_fr = max(w_all, float(whole)), max(w_fr, float(fmax))
        print(f"PCEDGE part={self.part} mode={self.mode} {self.tag} launches={len(rows)} whole={w_all:.3e} frame={w_fr:.3e} "
              f"band={self.tol:.1e}/{2.0 * self.tol:.1e}")
        assert not fails, f"{len(fails)} failures, first 12:\n" + "\n".join(fails[:12])


def _score_op(sc, mode, x, w, bias, G, what, blocks=False):
    """Launch the op on (x, w, bias) and queue its scores against float64 on the operands of `mode`."""
    torch = _torch()
    from s3prl_amd import _lib

    B, T, D = x.shape
    K = w.shape[2]
    ref = torch.from_numpy(conv_branch_ref(_round(x, mode), _round(w, mode), bias, G)).cuda()
    dx, dbias = _dev(x), _dev(bias)
    rc, buf = _launch(mode, dx, w, dbias, B, T, D, G, K)
    _lib.check(rc, f"s3enc_op_posconv {what}")
    branch = buf[GUARD:-GUARD].view(B, T, D).double() - dx.double()  # the conv branch, so that the residual hides nothing
    sc.add(what, branch, ref, _guards(buf), G if blocks else None)


# ---- A: every tile edge in T ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Dg", [32, 48, 64])
@pytest.mark.parametrize("mode", MODES)
def test_every_tile_edge_in_T(mode, Dg):
    """B = 2, G = 8 (the XCD-aware map), K = 16: T one below, at and one above every frame tile of the three kernels."""
    B, G, K = 2, 8, 16
    D = G * Dg
    rng = np.random.default_rng(zlib.crc32(f"pcedge/A/{Dg}".encode()))
    x, w, bias = draw(rng, B, max(T_EDGES), D, G, K)
    sc = _Scorer("A", mode, f"Dg={Dg}")
    for T in T_EDGES:
        _score_op(sc, mode, np.ascontiguousarray(x[:, :T]), w, bias, G, f"{mode} Dg {Dg} K {K} T {T}")
    sc.finish()


# ---- B: every K pipeline shape ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Dg", [32, 48, 64])
@pytest.mark.parametrize("mode", MODES)
def test_every_K_pipeline_shape(mode, Dg):
    """One frame past a tile of either kernel (T = 129, 257) at 1, 2, 3 and many weight stages, in fp32 also at odd K; K = 128 at
    T = 17 and T = 1, where the window reaches past the utterance on both sides."""
    B, G = 2, 8
    D = G * Dg
    sc = _Scorer("B", mode, f"Dg={Dg}")
    cases = [(K, T) for K in K_STAGES[Dg] + (K_ODD if mode == "fp32" else ()) for T in (129, 257)] + [(128, 17), (128, 1)]
    draws = {}
    for K, T in cases:
        if K not in draws:
            draws[K] = draw(np.random.default_rng(zlib.crc32(f"pcedge/B/{Dg}/{K}".encode())), B, 257, D, G, K)
        x, w, bias = draws[K]
        _score_op(sc, mode, np.ascontiguousarray(x[:, :T]), w, bias, G, f"{mode} Dg {Dg} K {K} ({K * Dg / 128:g} stages) T {T}")
    sc.finish()


# ---- C: both work maps ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_both_work_maps(mode):
    """The plain (frame tile, group, batch) order (G % 8 != 0) and the XCD-aware one (G = 8, 16, 24) at B = 1 and 3, two and three
    frame tiles; scored per (batch, group) block as well."""
    Dg, K = 32, 16
    sc = _Scorer("C", mode, f"Dg={Dg}")
    for G in (1, 3, 8, 16, 24):
        D = G * Dg
        x, w, bias = draw(np.random.default_rng(zlib.crc32(f"pcedge/C/{G}".encode())), 3, 300, D, G, K)
        for B in (1, 3):
            for T in (130, 300):
                _score_op(sc, mode, np.ascontiguousarray(x[:B, :T]), w, bias, G, f"{mode} G {G} B {B} T {T}", blocks=True)
    sc.finish()


# ---- D: a frame's bits do not depend on where it sits ---------------------------------------------------------------------------
@pytest.mark.parametrize("Dg", [32, 48, 64])
@pytest.mark.parametrize("mode", MODES)
def test_frame_bits_do_not_depend_on_the_tile_position(mode, Dg):
    """An utterance of 70 frames behind s zero rows (T = s + 70 + 16): its frames equal the s = 0 run bit for bit.  The fp32 kernel sums
    taps and channels in one order per accumulator, the 16-bit kernels sum k in an order that does not depend on t, zero rows add
    exact zeros — so any difference is a tile-position-dependent path.  No tolerance."""
    torch = _torch()
    from s3prl_amd import _lib

    B, G = 2, 8
    D = G * Dg
    fails, differing, flags, names = [], 0, [], []
    for K, shifts in ((16, SHIFTS),) + (((128, SHIFTS_K128),) if Dg == 48 else ()):
        u, w, bias = draw(np.random.default_rng(zlib.crc32(f"pcedge/D/{Dg}/{K}".encode())), B, UTT, D, G, K)
        dbias = _dev(bias)
        base = None
        for s in shifts:
            T = s + UTT + TAIL
            rc, buf = _launch(mode, _dev(embed(u, s)), w, dbias, B, T, D, G, K)
            _lib.check(rc, f"s3enc_op_posconv {mode} Dg {Dg} K {K} shift {s}")
            got = buf[GUARD:-GUARD].view(B, T, D)[:, s:s + UTT]
            if base is None:
                assert s == 0
                base = got.clone()
            g_nan, g_fin = _guards(buf)
            # (bit patterns: -0.0 == 0.0 and NaN != NaN under a float compare)
            diff = (got.contiguous().view(torch.int32) != base.view(torch.int32)).any(dim=2)  # (B, UTT): frames that differ
            first = torch.where(diff.any(), diff.reshape(-1).double().argmax(), torch.full((), -1, device="cuda"))
            flags.append(torch.stack([g_nan, g_fin, diff.sum().double(), first.double()]))
            names.append((K, s))
    for (K, s), (g_nan, g_fin, ndiff, first) in zip(names, torch.stack(flags).cpu().numpy()):
        what = f"{mode} Dg {Dg} K {K} shift {s}"
        if g_nan != 1.0 or g_fin != 1.0:
            fails.append(f"{what}: guard rows written or NaN / inf inside")
        if ndiff != 0:
            differing += 1
            b, i = divmod(int(first), UTT)
            t = s + i
            fails.append(f"{what}: {int(ndiff)} of {B * UTT} frames differ from the unshifted run, first (b {b}, utterance frame {i}, "
                         f"t {t}; t % 16 / 64 / 128 / 256 = {t % 16} / {t % 64} / {t % 128} / {t % 256})")
    print(f"PCEDGE part=D mode={mode} Dg={Dg} launches={len(names)} differing={differing} failures={len(fails)}")
    assert not fails, "\n".join(fails[:12])


# ---- E: the engine's own path (zero-tap padding, pos_pad kept from the real kernel), through the debug taps --------------------
def _grid_weight_v(rng, D, Dg, K):
    """weight_v on the bf16 grid with 1e-3 <= |v| (an fp16 normal, and far below fp16's largest): both 16-bit roundings return it."""
    import torch

    scale = 2.0 ** np.round(np.log2(3.0 / np.sqrt(Dg * K)))  # a power of two keeps the grid
    v = torch.from_numpy((rng.standard_normal((D, Dg, K)) * scale).astype(np.float32)).to(torch.bfloat16).float().numpy()
    small = np.abs(v) < 1e-3
    v[small] = np.where(v[small] < 0, -1.0, 1.0).astype(np.float32) * np.float32(2.0 ** -9)
    return v


def _engine_case(name, D, G, conv_pos):
    from s3prl_amd.synth import named_config, synth_weights

    cfg = named_config(name)
    cfg.encoder_layers = 1
    if D is not None:
        cfg.encoder_embed_dim, cfg.encoder_attention_heads, cfg.conv_pos_groups, cfg.conv_pos = D, D // 64, G, conv_pos
    cfg.validate()
    weights = synth_weights(cfg, zlib.crc32(f"pcedge/E/{name}/{D}/{G}/{conv_pos}".encode()) % 1000)
    if cfg.pos_conv_depth <= 1:
        rng = np.random.default_rng(zlib.crc32(f"pcedge/E/v/{D}/{G}/{conv_pos}".encode()))
        v = _grid_weight_v(rng, cfg.encoder_embed_dim, cfg.encoder_embed_dim // cfg.conv_pos_groups, cfg.conv_pos)
        weights["encoder.pos_conv.0.weight_v"] = v
        weights["encoder.pos_conv.0.weight_g"] = np.sqrt((v.astype(np.float64) ** 2).sum(axis=(0, 1), keepdims=True)).astype(np.float32)
    return cfg, weights


E_FRAMES = (257, 129, 1)  # one ragged batch: one frame past a 16-bit tile, one past an fp32 / X3 tile, a single frame
E_CASES = [(("tiny_hubert",) + c, m) for c in ((128, 4, 15), (192, 4, 3), (192, 4, 20), (128, 2, 31)) for m in MODES] + \
          [(("tiny_data2vec", None, None, None), m) for m in ("fp32", "fp32x3")]


@pytest.mark.parametrize("case,mode", E_CASES, ids=[f"{c[0]}-{c[1]}-{c[2]}-{c[3]}-{m}" for c, m in E_CASES])
def test_engine_posconv_taps(case, mode):
    """The engine's call: in the 16-bit and fp32x3 modes conv_pos = 15, 3, 20, 31 are packed as 16, 8, 24, 32 taps (zero taps appended
    until K is even and K * Dg a multiple of 128) with the real kernel's left padding 7, 1, 10, 15.  Scored per frame: `posconv` minus
    `proj` (the kernel's fp32 input) against the float64 branch of the `proj` tap with the folded weight.  The batch is one launch of
    T = 257 rows per utterance: the shorter utterances are valid rows in front of zero rows inside it, not launches of their own
    (part B runs the op at T = 1).  The taps are engine buffers without guard rows, so the guard scores do not apply here.

    weight_v lies on the bf16 grid with |v| >= 1e-3 and weight_g[k] = ||v[:, :, k]|| rounded to fp32, so the engine's fold
    w = v * (g / ||v||) moves w by at most one fp32 ulp and cannot move a 16-bit rounding: the 16-bit operand IS v (asserted below).

    tiny_data2vec (conv -> un-affine LayerNorm -> GELU, three times): fp32 and fp32x3 only — in the 16-bit modes the later stages
    round an fp32 intermediate that a float64 reference cannot reproduce bit for bit; those modes keep the suite's existing bounds."""
    import torch

    from oracle import encoder_oracle as O
    from s3prl_amd.encoder import HipEncoder
    from s3prl_amd.synth import synth_wavs

    name, D, G, conv_pos = case
    cfg, weights = _engine_case(name, D, G, conv_pos)
    Dm, Gm = cfg.encoder_embed_dim, cfg.conv_pos_groups
    lengths = [320 * (t - 1) + 400 for t in E_FRAMES]
    wavs = synth_wavs(lengths, 77)
    enc = HipEncoder(cfg, weights, dtype=mode)
    try:
        hs = enc.forward([torch.from_numpy(w).cuda() for w in wavs])
        torch.cuda.synchronize()
        B, T = len(E_FRAMES), max(E_FRAMES)
        assert tuple(hs.shape[1:]) == (B, T, Dm)
        proj = enc.debug_tap("proj").reshape(B, T, Dm)
        pc = enc.debug_tap("posconv").reshape(B, T, Dm)
    finally:
        enc.close()
    assert np.isfinite(proj).all(), f"{mode} {name}: NaN / inf in the `proj` tap"
    assert np.isfinite(pc).all(), f"{mode} {name}: NaN / inf in the `posconv` tap, first at (b, t, c) = {np.argwhere(~np.isfinite(pc))[0].tolist()}"
    for b, n in enumerate(lengths):  # (the family's mask rule may keep a frame more than the conv stack computes from n samples)
        t = cfg.valid_frames(n, max(lengths))
        assert E_FRAMES[b] <= t <= E_FRAMES[b] + 1 and not proj[b, t:].any() and proj[b, :t].any(), "proj: padded frames zero, valid ones not"
    if cfg.pos_conv_depth > 1:
        W64 = {k: v.astype(np.float64) for k, v in weights.items() if "pos_conv" in k}
        ref = O.pos_conv(cfg, W64, proj.astype(np.float64))
    else:
        v, g = weights["encoder.pos_conv.0.weight_v"], weights["encoder.pos_conv.0.weight_g"]
        w = O.fold_weight_norm(g, v)  # float64 fold, rounded to fp32 as the engine's
        assert w.dtype == np.float32 and (np.abs(w - v) <= np.spacing(np.abs(v))).all()
        if mode in ("bf16", "fp16"):
            assert np.array_equal(_round(w, mode), v), "the 16-bit operand is weight_v itself"
        ref = conv_branch_ref(_round(proj, mode), _round(w, mode), weights["encoder.pos_conv.0.bias"], Gm)
    sc = _Scorer("E", mode, f"{name} D={Dm} G={Gm} conv_pos={cfg.conv_pos}")
    sc.add(f"{mode} {name} D {Dm} G {Gm} conv_pos {cfg.conv_pos}", torch.from_numpy(pc.astype(np.float64) - proj.astype(np.float64)).cuda(),
           torch.from_numpy(ref).cuda(), None, Gm)
    sc.finish()


# ---- F: refusals ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,D,G,K,why", [(m, 256, 8, 15, "odd_K") for m in MODES[1:]] + [(m, 384, 8, 4, "partial_stage") for m in MODES[1:]]
                         + [(m, 320, 8, 16, "Dg40") for m in MODES])
def test_refusals_leave_the_output_untouched(mode, D, G, K, why):
    """What the implicit-GEMM kernels cannot run (odd K, K * Dg not a multiple of 128) and a group width no kernel is built for:
    non-zero with a message, and not one element of the NaN-prefilled output written.  (The engine pads such a K with zero taps.)"""
    torch = _torch()
    from s3prl_amd import _lib

    lib = _lib.load()
    B, T = 2, 33
    x, w, bias = draw(np.random.default_rng(5), B, T, D, G, K)
    rc, buf = _launch(mode, _dev(x), w, _dev(bias), B, T, D, G, K)
    torch.cuda.synchronize()
    assert rc != 0, f"{mode} D {D} G {G} K {K} ({why}) was accepted"
    msg = lib.s3enc_last_error()
    assert msg and b"posconv" in msg, msg
    assert bool(torch.isnan(buf).all()), f"{mode} ({why}): the refused call wrote into the output"
