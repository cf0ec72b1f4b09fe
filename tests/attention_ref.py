"""float64 yardstick of the attention row sweep (tests/test_attention_rows_gpu.py), numpy only: the operand draw, the float64
reference softmax(q k^T + gate * table[clamp(j - i)] + key mask) v of s3enc_op_attention, the operands each compute dtype sees,
a CPU restatement of the flash form with that dtype's roundings, named faults of the reference, the per-row score, and the list
of cases the sweep runs.  tests/test_attention_ref_cpu.py pins the reference against torch's float64
scaled_dot_product_attention, shows that the restatement sits under a quarter of each row band at every case, and feeds the
per-row score the faults it exists for (no GPU needed).

Rows are the (B*T, H*64) rows of the op's output: row b * T + t is query t of utterance b, all heads side by side.  A query
block is the 128 queries of one workgroup (attention.hip QT); key tiles are 32 keys (fp32) or 64 keys in two 32-key halves
(bf16, fp16, fp32x3)."""

import collections
import functools

import numpy as np

LOG2E = 1.4426950408889634
QT = 128  # queries per workgroup
DTYPES = ("fp32", "bf16", "fp16", "fp32x3")
ATT_TOL = {"fp32": 2e-5, "bf16": 1.5e-2, "fp16": 2e-3, "fp32x3": 5e-5}  # test_attention's whole-tensor bands


def row_band(dtype):
    """the per-row bound: twice the whole-tensor band (the rule of test_row_edges_gpu.py)"""
    return 2 * ATT_TOL[dtype]


# ---- the per-row score ------------------------------------------------------------------------------------------------------------
def row_errors(got, ref, floor=1e-3):
    """Per-row error ||got[m] - ref[m]|| / max(||ref[m]||, floor) of two (rows, cols) arrays."""
    got = np.asarray(got, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    return np.linalg.norm(got - ref, axis=1) / np.maximum(np.linalg.norm(ref, axis=1), floor)


def row_name(m, rows, T):
    at = f"row {m} of {rows} (row % 32 = {m % 32}, rows % 32 = {rows % 32})"
    if T:
        b, t = divmod(m, T)
        at += f" = utterance {b}, query {t} (query block {t // QT}, query % 32 = {t % 32}, T % 32 = {T % 32}, T % 64 = {T % 64})"
    return at


def assert_rows(got, ref, bound, what, floor=1e-3, T=None):
    """max over rows of row_errors < bound; a failure names the worst row and its residue mod 32 — with T (rows are B utterances
    of T queries) also its utterance, query, query block and the residues of T.  A row that is not finite fails."""
    got = np.asarray(got, dtype=np.float64)
    rows = len(ref)
    bad = ~np.isfinite(got).all(axis=1)
    if bad.any():
        m = int(np.argmax(bad))
        raise AssertionError(f"{what}: {row_name(m, rows, T)} is not finite ({int(bad.sum())} such rows)")
    e = row_errors(got, ref, floor)
    m = int(np.argmax(e))
    assert e[m] < bound, f"{what}: worst {row_name(m, rows, T)}: per-row error {e[m]:.3e} >= {bound:.1e}"
    return float(e[m])


def rel_err(got, ref):
    """the whole-tensor score (oracle.encoder_oracle.rel_err): ||got - ref|| / ||ref||"""
    got = np.asarray(got, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    return float(np.linalg.norm(got - ref) / np.linalg.norm(ref))


# ---- operands ---------------------------------------------------------------------------------------------------------------------
def round_bf16(x):
    """fp32 -> bf16 -> fp32, round to nearest even"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    return ((u + (((u >> 16) & 1) + 0x7FFF)) & 0xFFFF0000).astype(np.uint32).view(np.float32)


def round_to(x, dtype):
    """an fp32 array rounded to the 16-bit operand type; fp32 and fp32x3 see it unrounded (x3 splits, it does not round)"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    if dtype == "bf16":
        return round_bf16(x)
    if dtype == "fp16":
        return x.astype(np.float16).astype(np.float32)
    assert dtype in ("fp32", "fp32x3"), dtype
    return x


def draw(rng, B, T, H, R):
    """test_attention's recipe: qkv (B*T, 3*H*64) ~ N(0, 1) with q scaled by 0.35 and key T // 2 of utterance 0 scaled by 4 (the
    online-softmax rescale); a second key of utterance 0 scaled by 4 at valid[0] - 1 = T - 1, the last key of the partial last
    tile, so that the softmax reference has to move inside the masked tile (left alone where it is key T // 2 again: T <= 2);
    with a bias (R is not None) table (H, 2R + 1) ~ N(0, 1) and gate (B, H, T) = 1 + U(0, 1).  -> qkv, table, gate (fp32)"""
    D = 64 * H
    qkv = rng.standard_normal((B * T, 3 * D)).astype(np.float32)
    qkv[:, :D] *= 0.35
    qkv[T // 2, D:2 * D] *= 4.0
    if T - 1 != T // 2:
        qkv[T - 1, D:2 * D] *= 4.0
    table = gate = None
    if R is not None:
        table = rng.standard_normal((H, 2 * R + 1)).astype(np.float32)
        gate = (1 + rng.random((B, H, T))).astype(np.float32)
    return qkv, table, gate


def operands(qkv, dtype):
    """-> (what the kernel is given, fp32 values exact in `dtype`; what the reference sees, float64), as test_attention builds
    them: fp32 / fp32x3 unrounded; bf16 / fp16 rounded, with q * log2(e) taken in fp32 and rounded ONCE (the 16-bit kernels work
    on base-2 scores) and the reference on exactly that operand divided by log2(e)."""
    D = qkv.shape[1] // 3
    qdev = round_to(qkv, dtype)
    qref = qdev.astype(np.float64)
    if dtype in ("bf16", "fp16"):
        qdev = qdev.copy()
        qdev[:, :D] = round_to(qkv[:, :D] * np.float32(LOG2E), dtype)
        qref[:, :D] = qdev[:, :D].astype(np.float64) / LOG2E
    return qdev, qref


# ---- the reference ----------------------------------------------------------------------------------------------------------------
def heads(qkv, B, T, H):
    D = 64 * H
    return tuple(qkv[:, i * D:(i + 1) * D].reshape(B, T, H, 64).transpose(0, 2, 1, 3) for i in range(3))


def bias_index(T, R, clamp=None):
    """[i][j] -> clamp(j - i, -clamp, clamp) + R, the table column of (query i, key j); clamp defaults to R"""
    c = R if clamp is None else clamp
    return np.clip(np.arange(T)[None, :] - np.arange(T)[:, None], -c, c) + R


def _attend(qkv, keys, B, T, H, bias):
    """softmax(q k^T + bias + mask) v in float64; keys (B, T) bool, the live keys; bias (B, H, T, T) or None"""
    q, k, v = heads(np.asarray(qkv, dtype=np.float64), B, T, H)
    s = q @ k.transpose(0, 1, 3, 2)
    if bias is not None:
        s = s + bias
    s = np.where(keys[:, None, None, :], s, -np.inf)
    s = s - s.max(-1, keepdims=True)
    p = np.exp(s)
    p /= p.sum(-1, keepdims=True)
    return (p @ v).transpose(0, 2, 1, 3).reshape(B * T, 64 * H)


def live_keys(valid, T):
    return np.arange(T)[None, :] < np.asarray(valid)[:, None]


def gated_bias(table, gate, B, T, H, R, idx=None):
    """(B, H, T, T) float64: gate[b][h][i] * table[h][clamp(j - i, -R, R) + R]; gate None is 1"""
    idx = bias_index(T, R) if idx is None else idx
    gt = np.ones((B, H, T)) if gate is None else np.asarray(gate, dtype=np.float64)
    return gt[..., None] * np.asarray(table, dtype=np.float64)[:, idx][None]


def attention_ref(qkv, valid, B, T, H, table=None, gate=None, R=None):
    """The math of test_ops_gpu._attention_ref in float64 -> (B*T, H*64).  Every query row is computed, the padded ones
    (t >= valid[b]) like the rest — the kernels do the same."""
    bias = None if table is None else gated_bias(table, gate, B, T, H, R)
    return _attend(qkv, live_keys(valid, T), B, T, H, bias)


# ---- the flash form restated with a dtype's roundings -----------------------------------------------------------------------------
def _split(x):
    hi = round_bf16(x)
    return hi, round_bf16(x - hi)


def restate(qdev, valid, B, T, H, table, gate, R, dtype, x3_operands=False):
    """What a correct kernel of `dtype` computes, up to the order of its sums, on the CPU: `qdev` is operands(...)[0].  Scores,
    bias, softmax and row sum in float32 (bf16 / fp16: base-2 scores, the bias times gate * log2(e), exp2); the un-normalised
    probabilities rounded to the operand type before P.V (fp32x3: split into hi + lo bf16, both terms kept) while the row sum
    adds the unrounded ones; the result divided by the float32 row sum and, bf16 / fp16, rounded to the output type.  This is the
    reference alone: it never runs on the GPU.
    x3_operands (fp32x3 only): q, k and v are split into hi + lo bf16 as well and each product keeps three of its four terms
    (hi hi + hi lo + lo hi), as attn_x3_kernel forms them — the operand error of that mode (x = hi + lo + r, |r| <= 2^-17 |x|,
    and the lo lo term), which the float64 reference on unrounded operands does not see."""
    f32 = np.float32
    q, k, v = heads(np.ascontiguousarray(qdev, dtype=f32), B, T, H)
    kt = np.ascontiguousarray(k.transpose(0, 1, 3, 2))
    base2 = dtype in ("bf16", "fp16")
    assert not x3_operands or dtype == "fp32x3"
    if x3_operands:
        (qh, ql), (kh, kl) = _split(q), _split(kt)
        s = (qh @ kh + (qh @ kl + ql @ kh)).astype(f32)
    else:
        s = q @ kt
    assert s.dtype == f32
    if table is not None:
        gt = np.ones((B, H, T), dtype=f32) if gate is None else np.asarray(gate, dtype=f32)
        if base2:
            gt = gt * f32(LOG2E)
        s = s + gt[..., None] * np.asarray(table, dtype=f32)[:, bias_index(T, R)][None]
    s = np.where(live_keys(valid, T)[:, None, None, :], s, f32(-np.inf)).astype(f32)
    s = s - s.max(-1, keepdims=True)
    p = (np.exp2(s) if base2 else np.exp(s)).astype(f32)
    lsum = p.sum(-1, keepdims=True, dtype=f32)
    if x3_operands:
        (ph, pl), (vh, vl) = _split(p), _split(np.ascontiguousarray(v))
        o = (ph @ vh + (ph @ vl + pl @ vh)).astype(f32)
    elif dtype == "fp32x3":
        ph, pl = _split(p)
        o = (ph @ v + pl @ v).astype(f32)
    else:
        o = round_to(p, dtype) @ v
    assert o.dtype == f32 and lsum.dtype == f32
    o = (o / lsum).transpose(0, 2, 1, 3).reshape(B * T, 64 * H)
    return round_to(o, dtype) if base2 else o


# ---- the cases --------------------------------------------------------------------------------------------------------------------
B, H = 3, 3  # 9 (batch, head) units: not a multiple of the 8 XCDs, the padded work map runs
LENGTHS = (1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 160, 191, 255, 256, 257, 300)
MODES = ("none", "R=0", "R=3", "R=T-2", "R=T-1", "R=T+70")
VALID_POOL = (1, 17, 31, 32, 33, 63, 64, 65, 129, 130)  # and T - 1
RESIDUES = (1, 31, 32, 33, 63, 0)  # of valid mod 64, each to be met with and without bias

Case = collections.namedtuple("Case", "T mode R valid seed")


def _mode_R(T, mode):
    return {"none": None, "R=0": 0, "R=3": 3, "R=T-2": T - 2, "R=T-1": T - 1, "R=T+70": T + 70}[mode]


def _cases():
    """Per T: no bias, then R = 0 (must equal no bias), 3 (clamps almost everywhere), T - 2 (clamps the extreme pair only),
    T - 1 (the exact window), T + 70 (a table wider than any window) — a negative R and an R already listed for this T dropped.
    valid = [T, v1, v2], v1 and v2 walking the pool {1, 17, 31, 32, 33, 63, 64, 65, 129, 130, T - 1} within [1, T] by length
    and mode."""
    out = []
    for i, T in enumerate(LENGTHS):
        pool = sorted({v for v in VALID_POOL + (T - 1,) if 1 <= v <= T})
        seen = set()
        for j, mode in enumerate(MODES):
            R = _mode_R(T, mode)
            if R is not None and (R < 0 or R in seen):
                continue
            seen.add(R)
            v1, v2 = pool[(2 * (i + j)) % len(pool)], pool[(2 * (i + j) + 1) % len(pool)]
            out.append(Case(T, mode, R, (T, v1, v2), 1000 * T + j))
    return tuple(out)


CASES = _cases()


def _check_cases():
    for biased in (False, True):
        vs = {v for c in CASES if (c.R is not None) == biased for v in c.valid}
        assert 1 in vs, biased
        assert {v % 64 for v in vs} >= set(RESIDUES), (biased, sorted(vs))
    assert any(c.T >= 160 and QT <= v < min(2 * QT, c.T) for c in CASES for v in c.valid[1:])  # valid inside the second query block
    assert all(1 <= v <= c.T for c in CASES for v in c.valid) and all(c.valid[0] == c.T for c in CASES)
    assert len({(c.T, c.R) for c in CASES}) == len(CASES)


_check_cases()


def cases_of(mode):
    return [c for c in CASES if c.mode == mode]


@functools.lru_cache(maxsize=None)
def case_inputs(case):
    """-> qkv, table, gate, valid of a case (read-only arrays, drawn once)"""
    qkv, table, gate = draw(np.random.default_rng(case.seed), B, case.T, H, case.R)
    valid = np.array(case.valid, dtype=np.int32)
    for a in (qkv, table, gate, valid):
        if a is not None:
            a.setflags(write=False)
    return qkv, table, gate, valid


@functools.lru_cache(maxsize=None)
def _case_reference(case, rounding, biased):
    qkv, table, gate, valid = case_inputs(case)
    ref = attention_ref(operands(qkv, rounding)[1], valid, B, case.T, H, *((table, gate, case.R) if biased else ()))
    ref.setflags(write=False)
    return ref


def case_reference(case, dtype, biased=True):
    """attention_ref on operands(qkv, dtype), computed once per case and operand rounding (fp32 and fp32x3 share theirs) and left
    unchanged; biased = False: the same operands without the bias (what R = 0 must equal)"""
    return _case_reference(case, "fp32" if dtype == "fp32x3" else dtype, bool(biased and case.R is not None))


# ---- faults: the reference with one thing wrong -----------------------------------------------------------------------------------
# fault(qref, valid, B, T, H, table, gate, R) -> (the wrong result, bool (B*T) the rows it is wrong in), or None where the fault
# cannot show at this shape.
def _rows(B, T, ts=None, bs=None):
    m = np.zeros((B, T), dtype=bool)
    m[(slice(None) if bs is None else bs), (slice(None) if ts is None else ts)] = True
    return m.reshape(-1)


def _splice(good, bad, rows):
    out = good.copy()
    out[rows] = bad[rows]
    return out


def _fault_bias_shift(qref, valid, B, T, H, table, gate, R):
    """the bias window one entry off for the queries of the last query block (a wrong rel0 / bias_off of that block)"""
    if table is None or R < 1:
        return None
    q0 = (T - 1) // QT * QT
    idx = np.clip(bias_index(T, R) + 1, 0, 2 * R)
    bad = _attend(qref, live_keys(valid, T), B, T, H, gated_bias(table, gate, B, T, H, R, idx))
    rows = _rows(B, T, ts=slice(q0, T))
    return _splice(attention_ref(qref, valid, B, T, H, table, gate, R), bad, rows), rows


def _with_gate(qref, valid, B, T, H, table, gate, R, gate2, ts):
    rows = _rows(B, T, ts=ts)
    return _splice(attention_ref(qref, valid, B, T, H, table, gate, R), attention_ref(qref, valid, B, T, H, table, gate2, R), rows), rows


def _fault_gate_last(qref, valid, B, T, H, table, gate, R):
    """the last query, T - 1, takes row T - 2's gate (the clamped row q_c one short)"""
    if table is None or T < 2:
        return None
    g2 = np.array(gate, dtype=np.float64)
    g2[:, :, T - 1] = g2[:, :, T - 2]
    return _with_gate(qref, valid, B, T, H, table, gate, R, g2, [T - 1])


def _fault_gate_block_first(qref, valid, B, T, H, table, gate, R):
    """the first query of every query block after the first takes the gate of the row before it"""
    ts = list(range(QT, T, QT))
    if table is None or not ts:
        return None
    g2 = np.array(gate, dtype=np.float64)
    g2[:, :, ts] = g2[:, :, [t - 1 for t in ts]]
    return _with_gate(qref, valid, B, T, H, table, gate, R, g2, ts)


def _fault_clamp(qref, valid, B, T, H, table, gate, R):
    """|key - query| clamped at R - 1 instead of R: wrong wherever a live key is R or more away, invisible at R >= T"""
    if table is None or R < 1:
        return None
    bias = gated_bias(table, gate, B, T, H, R, bias_index(T, R, clamp=R - 1))
    bad = _attend(qref, live_keys(valid, T), B, T, H, bias)
    d = np.abs(np.arange(T)[None, :] - np.arange(T)[:, None]) >= R  # [i][j]
    rows = np.stack([(d & (np.arange(T)[None, :] < v)).any(1) for v in valid]).reshape(-1)
    return bad, rows


def _fault_mask_late(qref, valid, B, T, H, table, gate, R):
    """the key mask one key late: key valid[b] is live"""
    v2 = np.minimum(np.asarray(valid) + 1, T)
    if (v2 == valid).all():
        return None
    bad = attention_ref(qref, v2, B, T, H, table, gate, R)
    return bad, _rows(B, T, bs=np.flatnonzero(v2 != valid))


def _fault_half_dropped(qref, valid, B, T, H, table, gate, R):
    """the second 32-key half of a 64-key tile skipped where it holds one live key (valid % 64 == 33: `two` decided with <= )"""
    hit = np.flatnonzero(np.asarray(valid) % 64 == 33)
    if not len(hit):
        return None
    keys = live_keys(valid, T)
    for b in hit:
        keys[b, valid[b] - 1] = False
    bias = None if table is None else gated_bias(table, gate, B, T, H, R)
    return _attend(qref, keys, B, T, H, bias), _rows(B, T, bs=hit)


def _fault_nan_row(qref, valid, B, T, H, table, gate, R):
    """one query row, the last of the middle utterance, never written (NaN)"""
    bad = attention_ref(qref, valid, B, T, H, table, gate, R)
    rows = _rows(B, T, ts=[T - 1], bs=[B // 2])
    bad[rows] = np.nan
    return bad, rows


FAULTS = {
    "bias window shifted in the last query block": _fault_bias_shift,
    "gate of the last query from row T-2": _fault_gate_last,
    "gate of a block's first query from the row before": _fault_gate_block_first,
    "clamp at R-1": _fault_clamp,
    "key mask one key late": _fault_mask_late,
    "second 32-key half dropped at valid % 64 == 33": _fault_half_dropped,
    "one row left NaN": _fault_nan_row,
}
