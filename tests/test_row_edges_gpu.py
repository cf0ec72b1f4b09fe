"""Row edges: every tiled kernel works in 32-row blocks — a wave owns 32 rows and walks them in passes — and the last block of a call is
usually partial.  That is where a cross-lane read or a masked store goes wrong, and where a Frobenius norm over the whole tensor does
not look (one wrong row out of 15 968 moves it by under 1 %).  These tests sweep the row residue M % 32 through the GEMM epilogues,
LayerNorm 1 folded into fc2's residual epilogue (gemm16.hip res_ln_*) and attention, score every ROW on its own, and check that
nothing is written past the last row or column (NaN-prefilled guard rows / columns)."""

import dataclasses
import functools
import zlib

import numpy as np
import pytest

from attention_ref import ATT_TOL, assert_rows, row_errors  # noqa: F401  (the per-row score, shared with the attention row sweep)
from oracle import encoder_oracle as O
from test_ops_gpu import TOL, _attention_ref, _dev, _ptr, _round, _torch

pytestmark = pytest.mark.gpu

GUARD = 32  # NaN rows behind the last row of every output buffer


# ---- shared helpers ---------------------------------------------------------------------------------------------------------------
def guarded(rows, cols, dtype, ldo=None):
    """A NaN-prefilled (rows + GUARD, ldo) device buffer and its (rows, cols) view (row stride ldo)."""
    torch = _torch()
    buf = torch.full((rows + GUARD, ldo or cols), float("nan"), device="cuda", dtype=dtype)
    return buf, buf[:rows, :cols]


def assert_guards(buf, rows, cols, what):
    """The guard rows behind row `rows` - 1 and the guard columns right of column `cols` - 1 are still NaN."""
    torch = _torch()
    hit = ~torch.isnan(buf[rows:].float())
    if hit.any():
        r, c = (int(x) for x in hit.nonzero()[0])
        raise AssertionError(f"{what}: {int(hit.sum())} writes into the guard rows behind row {rows - 1} (rows % 32 = {rows % 32}), "
                             f"first at guard row {r}, column {c}")
    if buf.shape[1] > cols:
        hit = ~torch.isnan(buf[:rows, cols:].float())
        if hit.any():
            r, c = (int(x) for x in hit.nonzero()[0])
            raise AssertionError(f"{what}: {int(hit.sum())} writes into the guard columns (ldo {buf.shape[1]} > N {cols}), "
                                 f"first at row {r}, column {cols + c}")


def _set(lib, key, value):
    from s3prl_amd import _lib

    _lib.check(lib.s3enc_set_tuning(key.encode(), int(value)), f"s3enc_set_tuning {key}")


# ---- (a, b, c) LayerNorm 1 folded into fc2 -------------------------------------------------------------------------------------
# HuBERT-base is post-LN: with ln1_fold (default 1) the 16-bit modes' fc2 rebuilds LN1(y) in its residual epilogue from per-row
# (mean, rstd) that a pass reads from another lane.  Two layers keep the real fc2 shape (N = 768, K = 3072: gemm16_big).
LN1_RESIDUES = [0, 1, 9, 16, 17, 18, 21, 25, 26, 27, 29, 31]


@functools.lru_cache(maxsize=None)
def _model(layers):
    from s3prl_amd.synth import named_config, synth_weights

    cfg = dataclasses.replace(named_config("hubert_base"), encoder_layers=layers)
    return cfg, synth_weights(cfg, 0)


def _samples(T):
    """An utterance length of exactly T frames (T = (n - 400) // 320 + 1), half a hop away from either frame boundary."""
    return 400 + 320 * (T - 1) + 160


def _batches(cfg, Ts, ragged=False):
    """One B = 1 batch per T (M = T); `ragged`: plus a B = 3 batch of T = 91 frames, B * T % 32 = 17, with two shorter utterances."""
    torch = _torch()
    from s3prl_amd.synth import synth_wavs

    lens = [[_samples(T)] for T in Ts]
    if ragged:
        lens.append([_samples(91) - 1000, _samples(91), _samples(40)])
    out = []
    for i, ls in enumerate(lens):
        assert cfg.num_frames(max(ls)) == (Ts[i] if i < len(Ts) else 91)
        out.append([torch.from_numpy(w).cuda() for w in synth_wavs(ls, 100 + i)])
    return out


def _fold_runs(cfg, weights, dtype, batches, tune):
    """{fold: [hidden states of every batch]} with ln1_fold = 1 and 0 under the tuning `tune`, plus the bytes per launch that the
    `layernorm:ln1` profile entry counted on the first batch."""
    torch = _torch()
    from s3prl_amd import _lib
    from s3prl_amd.encoder import HipEncoder

    lib = _lib.load()
    outs, ln1 = {}, {}
    for fold in (1, 0):
        _set(lib, "ln1_fold", fold)
        for k, v in tune.items():
            _set(lib, k, v)
        enc = HipEncoder(cfg, weights, dtype=dtype)
        try:
            outs[fold] = [enc.forward(b).clone() for b in batches]
            enc.profile_enable(True)
            enc.profile_reset()
            enc.forward(batches[0])
            torch.cuda.synchronize()
            e = [p for p in enc.profile_read() if p["name"] == "layernorm:ln1"]
            enc.profile_enable(False)
            assert len(e) == 1 and e[0]["launches"] == cfg.encoder_layers, e
            ln1[fold] = e[0]["bytes"] / e[0]["launches"]
        finally:
            enc.close()
    return outs, ln1


def _fold_failures(cfg, outs, batches, what):
    """One line per batch whose folded forward is not bit-identical to the unfolded one: M % 32, the first state that differs and its
    differing rows (later states spread a wrong frame to every frame through attention)."""
    fails = []
    for o1, o0 in zip(outs[1], outs[0]):
        assert _torch().isfinite(o1).all(), f"{what}: non-finite states"
        if _torch().equal(o1, o0):
            continue
        NS, B, T, D = o1.shape
        diff = (o1 != o0).any(dim=-1).cpu().numpy()  # (NS, B, T)
        s = int(np.argmax(diff.any(axis=(1, 2))))
        rows = [int(i * T + t) for i, t in zip(*np.nonzero(diff[s]))]
        fails.append(f"M = {B * T} (M % 32 = {B * T % 32}): state {s} differs first, in rows {rows[:6]}{' ...' if len(rows) > 6 else ''}")
    return fails


def _check_ln1_bytes(cfg, batches, ln1, what):
    M = len(batches[0]) * cfg.num_frames(max(int(w.numel()) for w in batches[0]))
    D, es = cfg.encoder_embed_dim, 2
    assert ln1[1] == M * D * (4 + es), f"{what}: ln1_fold = 1 did not fold (layernorm:ln1 {ln1[1]:.0f} bytes per launch)"
    assert ln1[0] == M * D * (8 + es), f"{what}: ln1_fold = 0 folded (layernorm:ln1 {ln1[0]:.0f} bytes per launch)"


@pytest.mark.parametrize("dtype,mx", [("bf16", None), ("fp16", None), ("fp16x2", 14), ("fp16x2", 0)])
def test_ln1_fold_is_bit_identical_at_every_row_residue(dtype, mx):
    """ln1_fold = 1 against 0, bit for bit, at M = T = 64 + r for r = 0..31 and on a ragged B = 3 batch with B*T % 32 = 17, in
    every 16-bit mode (fp16x2: with its default MX second term, and with two fp16 terms, gemm16_mx = 0).  The fold must really run."""
    from s3prl_amd import _lib

    cfg, weights = _model(2)
    Ts = [64 + 17] + [64 + r for r in range(32) if r != 17]  # (the first batch is the one profiled: a residue that used to break)
    batches = _batches(cfg, Ts, ragged=True)
    lib = _lib.load()
    try:
        outs, ln1 = _fold_runs(cfg, weights, dtype, batches, {} if mx is None else {"gemm16_mx": mx})
    finally:
        _set(lib, "ln1_fold", 1)
        _set(lib, "gemm16_mx", 14)
    what = f"{dtype}" + ("" if mx is None else f" gemm16_mx = {mx}")
    fails = _fold_failures(cfg, outs, batches, what)
    assert not fails, f"{what}: ln1_fold = 1 differs from ln1_fold = 0 at\n  " + "\n  ".join(fails)
    _check_ln1_bytes(cfg, batches, ln1, what)


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_ln1_fold_is_bit_identical_in_every_gemm16_big_mode(dtype):
    """The same bit-identity with fc2 forced through every large-tile configuration (gemm16_big 1, 2, 4-10: the 256 / 192 / 128-row
    tiles, one-shot and persistent, the OVL epilogue of 32-column staging rounds, the row-per-lane modes) at the residues where a
    cross-lane read of the stats can land on a lane that is past M."""
    from s3prl_amd import _lib

    cfg, weights = _model(2)
    Ts = [64 + r for r in [17] + [r for r in LN1_RESIDUES if r != 17]]
    batches = _batches(cfg, Ts)
    lib = _lib.load()
    fails = []
    try:
        for mode in (1, 2, 4, 5, 6, 7, 8, 9, 10):
            outs, ln1 = _fold_runs(cfg, weights, dtype, batches, {"gemm16_big": mode})
            what = f"{dtype} gemm16_big = {mode}"
            fails += [f"{what}: {f}" for f in _fold_failures(cfg, outs, batches, what)]
            _check_ln1_bytes(cfg, batches, ln1, what)
    finally:
        _set(lib, "ln1_fold", 1)
        _set(lib, "gemm16_big", 3)
    assert not fails, "ln1_fold = 1 differs from ln1_fold = 0 at\n  " + "\n  ".join(fails)


# worst per-frame error over all 13 hidden states of HuBERT-base (12 layers, synthetic weights, one 16 000-sample utterance: T = 49,
# M % 32 = 17) against the float64 oracle, measured on the MI355X with ln1_fold = 0: fp16x2 4.04e-4, bf16 1.16e-2 (the same with the
# fold).  The bound is twice that; a row whose residual lost its LayerNorm is off by O(1).
PER_FRAME_BOUND = {"fp16x2": 8.1e-4, "bf16": 2.3e-2}


@pytest.mark.parametrize("dtype", ["fp16x2", "bf16"])
def test_one_second_utterance_matches_the_oracle_frame_by_frame(dtype):
    """The user-visible case: a post-LN base model, one utterance at a time, T = 49 — every frame of every state near the oracle."""
    torch = _torch()
    from s3prl_amd.encoder import HipEncoder
    from s3prl_amd.synth import synth_wavs

    cfg, weights = _model(12)
    wavs = synth_wavs([16000], 21)
    enc = HipEncoder(cfg, weights, dtype=dtype)
    try:
        hs = enc.forward([torch.from_numpy(w).cuda() for w in wavs]).cpu().numpy()
    finally:
        enc.close()
    assert hs.shape[2] == 49
    ref = O.forward(cfg, weights, wavs, dtype=np.float64)
    for l, r in enumerate(ref):
        assert_rows(hs[l, 0], r[0], PER_FRAME_BOUND[dtype], f"{dtype} hidden state {l}")


# ---- (d, e) GEMM epilogues at every row residue --------------------------------------------------------------------------------
GEMM_N, GEMM_K = 768, 256
M_SWEEP = [32] + list(range(1, 32)) + list(range(512, 544))  # every tile height (256 / 192 / 128 / 64) ends partial at every residue
M_MAX = max(M_SWEEP)
WIDE = GEMM_N + 64  # ldo of the epilogues that also check guard columns

# the epilogue instantiations gemm16.hip's run_epilogue selects between: name -> (act, residual, row_limit, out32, out16, ldo)
EPI16 = {
    "row_limit": (1, True, True, True, True, GEMM_N),     # the generic form
    "act_out16": (1, False, False, False, True, GEMM_N),  # conv1-5, fc1
    "out16": (0, False, False, False, True, WIDE),        # q|k|v
    "res_out32": (0, True, False, True, False, GEMM_N),   # out_proj, fc2
    "act_out32": (1, False, False, True, False, WIDE),    # the last conv
    "out32_out16": (0, False, False, True, True, GEMM_N),  # (generic: both outputs)
}
# the fp32-output kernels (gemm.hip, gemmt.hip, gemm_x3.hip); act 3 = swish
EPI32 = {
    "row_limit": (1, True, True, True, False, GEMM_N),
    "out32": (0, False, False, True, False, WIDE),
    "res_out32": (0, True, False, True, False, GEMM_N),
    "act_out32": (1, False, False, True, False, WIDE),
    "swish_out32": (3, True, False, True, False, WIDE),
}
# family -> (s3enc_op_gemm dtype code, operand rounding, TOL key, tuning key, its modes, its default)
FAMILIES = {
    "fp32": (0, "fp32", "fp32", "gemm32_big", (0, 1, 2, 3, 4, 5), 1),
    "bf16": (1, "bf16", "bf16", "gemm16_big", (0, 1, 2, 4, 5, 6, 7, 8, 9, 10), 3),
    "fp16": (2, "fp16", "fp16", "gemm16_big", (0, 1, 2, 4, 5, 6, 7, 8, 9, 10), 3),
    "fp16x2": (4, "fp16", "fp16", None, (None,), None),
    "fp16x2_mx": (5, "fp16", "fp16", None, (None,), None),
    "fp32x3": (3, "fp32", "fp32x3", "gemm_x3_tile", (0, 1, 2, 4), 1),
}


def _limit(M):
    return (3 * M) // 4  # rows >= limit are zeroed (the padded frames of proj)


def _gemm_operands(family):
    """Device operands at M_MAX rows and the float64 pre-activation product; every smaller M uses the leading rows."""
    torch = _torch()
    code, rnd = FAMILIES[family][:2]
    rng = np.random.default_rng(zlib.crc32(f"row_edges/{family}".encode()))
    A = _round(rng.standard_normal((M_MAX, GEMM_K)).astype(np.float32), rnd)
    W = (rng.standard_normal((GEMM_N, GEMM_K)) / np.sqrt(GEMM_K)).astype(np.float32)
    bias = rng.standard_normal(GEMM_N).astype(np.float32)
    res = rng.standard_normal((M_MAX, WIDE)).astype(np.float32)
    if code == 4:  # [hi | lo] fp16 halves per row: the product is with hi + lo
        Wt = torch.from_numpy(W)
        hi = Wt.half()
        lo = (Wt - hi.float()).half()
        dW = torch.cat([hi, lo], dim=1).contiguous().cuda()
        W64 = hi.double().numpy() + lo.double().numpy()
    elif code in (1, 2):
        dW, W64 = _dev(W, rnd), _round(W, rnd).astype(np.float64)
    else:  # fp32 / fp32x3 / the MX entry take the fp32 weight (the latter two pack it inside the call)
        dW, W64 = _dev(W), W.astype(np.float64)
    ops = dict(A=_dev(A, rnd), W=dW, bias=_dev(bias), res={ldo: _dev(np.ascontiguousarray(res[:, :ldo])) for ldo in (GEMM_N, WIDE)})
    lin = A.astype(np.float64) @ W64.T + bias
    return ops, lin, res.astype(np.float64)


def _gemm_ref(lin, res, M, act, use_res, use_lim):
    y = lin[:M].copy()
    if act == 1:
        y = O.gelu(y)
    elif act == 3:
        y = y / (1.0 + np.exp(-y))  # x * sigmoid(x)
    if use_res:
        y = y + res[:M, :GEMM_N]
    if use_lim:
        y[_limit(M):] = 0
    return y


@pytest.mark.parametrize("family", list(FAMILIES))
def test_gemm_epilogues_at_every_row_residue(family):
    """s3enc_op_gemm at N = 768, K = 256 and M = 32, 1..31, 512..543 in every epilogue instantiation and every kernel mode of the
    family, against float64: the TOL band and element check of test_gemm, a per-row bound, and untouched guard rows / columns.
    fp32: every gemm32_big mode also bit-identical to mode 0 (the 128x128 kernel) at every M.  fp32x3 at M >= 128."""
    torch = _torch()
    from s3prl_amd import _lib

    lib = _lib.load()
    code, rnd, tk, key, modes, default = FAMILIES[family]
    tol = TOL[tk]
    epis = EPI32 if code in (0, 3) else EPI16
    if code == 3:
        epis = {k: v for k, v in epis.items() if v[0] != 3}  # (swish: the exact-fp32 kernels only)
    ms = [m for m in M_SWEEP if m >= 128] if code == 3 else M_SWEEP
    ops, lin, res = _gemm_operands(family)
    t16 = torch.bfloat16 if rnd == "bf16" else torch.float16
    try:
        for M in ms:
            lim = torch.tensor([_limit(M)], dtype=torch.int32, device="cuda")
            for name, (act, use_res, use_lim, o32, o16, ldo) in epis.items():
                ref = _gemm_ref(lin, res, M, act, use_res, use_lim)
                first = None
                for mode in modes:
                    what = f"{family} gemm M = {M} (M % 32 = {M % 32}) {name}" + ("" if key is None else f" {key} = {mode}")
                    if key is not None:
                        _set(lib, key, mode)
                    b32, v32 = guarded(M, GEMM_N, torch.float32, ldo) if o32 else (None, None)
                    b16, v16 = guarded(M, GEMM_N, t16, ldo) if o16 else (None, None)
                    rc = lib.s3enc_op_gemm(code, _ptr(ops["A"]), GEMM_K, M * GEMM_K, _ptr(ops["W"]), _ptr(ops["bias"]), M, GEMM_N, GEMM_K,
                                           1, act, _ptr(ops["res"][ldo]) if use_res else None, _ptr(lim) if use_lim else None,
                                           _ptr(b32), _ptr(b16), ldo, M * ldo, None)
                    _lib.check(rc, what)
                    torch.cuda.synchronize()
                    if o32:
                        assert_guards(b32, M, GEMM_N, what + " out32")
                        got = v32.cpu().numpy()
                        assert_rows(got, ref, 2 * tol, what + " out32")
                        err = O.rel_err(got, ref)
                        assert err < tol, f"{what}: rel-err {err:.3e}"
                        bad = np.abs(got - ref) > 50 * tol * (1 + np.abs(ref))
                        assert not bad.any(), f"{what}: {bad.sum()} elements off, first at {np.argwhere(bad)[0]}"
                        if code == 0:
                            if first is None:
                                first = v32.clone()
                            else:
                                assert torch.equal(first, v32), f"{what}: differs from gemm32_big = 0"
                    if o16:
                        assert_guards(b16, M, GEMM_N, what + " out16")
                        assert_rows(v16.float().cpu().numpy(), ref, 4 * tol, what + " out16")
    finally:
        if key is not None:
            _set(lib, key, default)


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_gemm_swish_is_refused_by_the_16bit_kernels(dtype):
    """act = 3 (swish) exists in the exact-fp32 kernels only: a 16-bit call is an error, and nothing is written."""
    torch = _torch()
    from s3prl_amd import _lib

    lib = _lib.load()
    ops, _, _ = _gemm_operands(dtype)
    M = 100
    b32, _ = guarded(M, GEMM_N, torch.float32)
    rc = lib.s3enc_op_gemm(_lib.DTYPES[dtype], _ptr(ops["A"]), GEMM_K, M * GEMM_K, _ptr(ops["W"]), _ptr(ops["bias"]), M, GEMM_N, GEMM_K,
                           1, 3, None, None, _ptr(b32), None, GEMM_N, M * GEMM_N, None)
    torch.cuda.synchronize()
    assert rc != 0, f"{dtype} gemm with act = 3 was accepted"
    assert torch.isnan(b32).all(), f"{dtype} gemm with act = 3 wrote its output"


# ---- (f) attention row edges ---------------------------------------------------------------------------------------------------
def _valid(T, r):
    """Ragged valid lengths whose residues mod 32 are 1, 17 or 31 (and the full T)."""
    return np.array([T, (33, 49, 63)[r % 3], (1, 17, 31)[(r + 1) % 3]], dtype=np.int32)


@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16", "fp32x3"])
def test_attention_rows_at_every_residue(dtype):
    """s3enc_op_attention at T = 64 + r, r = 0..31 (B = 3, ragged valid), every query row against float64, guard rows after B*T."""
    torch = _torch()
    from s3prl_amd import _lib

    lib = _lib.load()
    B, H = 3, 2
    D = 64 * H
    for r in range(32):
        T = 64 + r
        rng = np.random.default_rng(500 + r)
        qkv = rng.standard_normal((B * T, 3 * D)).astype(np.float32)
        qkv[:, :D] *= 0.35
        qkv[T // 2, D:2 * D] *= 4.0
        valid = _valid(T, r)
        qr = _round(qkv, dtype).astype(np.float64)
        qdev = qkv
        if dtype in ("bf16", "fp16"):  # (q pre-scaled by log2(e) for the 16-bit kernels, as in test_attention)
            log2e = 1.4426950408889634
            qdev = qkv.copy()
            qdev[:, :D] = _round(qkv[:, :D] * np.float32(log2e), dtype)
            qr[:, :D] = qdev[:, :D].astype(np.float64) / log2e
        ref = _attention_ref(qr, valid, B, T, H)
        dq = _dev(qdev, dtype)
        buf, out = guarded(B * T, D, dq.dtype)
        dvalid = torch.from_numpy(valid).cuda()
        what = f"attention {dtype} T = {T} (T % 32 = {r}, B*T % 32 = {B * T % 32}) valid {valid.tolist()}"
        _lib.check(lib.s3enc_op_attention(_lib.DTYPES[dtype], _ptr(dq), _ptr(out), _ptr(dvalid), B, T, H, None, 0, None, None), what)
        torch.cuda.synchronize()
        assert_guards(buf, B * T, D, what)
        got = out.float().cpu().numpy()
        assert_rows(got, ref, 2 * ATT_TOL[dtype], what, T=T)
        assert O.rel_err(got, ref) < ATT_TOL[dtype], what


@pytest.mark.parametrize("T", [64, 65, 81, 95, 96, 127, 128, 129, 160, 255, 256, 257])
def test_relpos_attention_rows_at_row_edges(T):
    """s3enc_op_relpos_attention (Conformer rel_pos, fp32) with H = 16 at T = 0 and other residues mod 32, ragged valid: every query row
    against float64 (conformer_ref.relpos_scores), guard rows after B*T.  T > 128 (H = 3): a second and a third 128-query block, whose
    S_rel ring starts at a block-dependent window row, one utterance's valid inside the second block."""
    torch = _torch()
    import conformer_ref as R
    from s3prl_amd import _lib

    lib = _lib.load()
    B, H = 3, 16 if T <= 128 else 3
    D = 64 * H
    rng = np.random.default_rng(900 + T)
    qkv = rng.standard_normal((B, T, 3 * D)).astype(np.float32)
    qkv[..., :D] *= 0.3
    P = (0.5 * rng.standard_normal((2 * T - 1, D))).astype(np.float32)
    qadd = (0.1 * rng.standard_normal((H, 64))).astype(np.float32)
    valid = _valid(T, T % 32)
    if T > 128:
        valid[1] = min(130, T - 1)
    buf, out = guarded(B * T, D, torch.float32)
    dvalid = torch.from_numpy(valid).cuda()
    dqkv, dP, dqadd = _dev(qkv), _dev(P), _dev(qadd)
    what = f"relpos attention T = {T} (T % 32 = {T % 32}) valid {valid.tolist()}"
    _lib.check(lib.s3enc_op_relpos_attention(_ptr(dqkv), _ptr(out), _ptr(dvalid), B, T, H, _ptr(dP), _ptr(dqadd), None), what)
    torch.cuda.synchronize()
    assert_guards(buf, B * T, D, what)
    x = qkv.astype(np.float64)
    sh = lambda t: t.reshape(B, T, H, 64).transpose(0, 2, 1, 3)  # noqa: E731
    q, k, v = sh(x[..., :D]), sh(x[..., D:2 * D]), sh(x[..., 2 * D:])
    s = R.relpos_scores(q, k, P.astype(np.float64).reshape(2 * T - 1, H, 64), qadd.astype(np.float64))
    ref = (R.softmax_masked(s, valid) @ v).transpose(0, 2, 1, 3).reshape(B * T, D)
    got = out.cpu().numpy()
    assert_rows(got, ref, 4e-5, what, T=T)
    assert O.rel_err(got, ref) < 2e-5, what
