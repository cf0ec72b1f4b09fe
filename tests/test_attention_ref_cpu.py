"""Pins the yardstick of tests/test_attention_rows_gpu.py (tests/attention_ref.py), no GPU: (a) the float64 reference is torch's
float64 scaled_dot_product_attention with the gated, clamped table and the key padding as an additive mask; (b) on the sweep's
draw the flash form restated with each dtype's roundings stays under a quarter of that dtype's row band at every case — the inputs
are fair and the band has room for a correct kernel; (c) the per-row score names the row of each fault the sweep exists for, where
the whole-tensor score lets the two gate faults through; (d) a NaN row counts as failed."""

import re

import numpy as np
import pytest
import torch

import attention_ref as A

B, H = A.B, A.H


def _case(T, mode):
    (c,) = [c for c in A.CASES if c.T == T and c.mode == mode]
    return c


# ---- (a) ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,mode", [(65, "none"), (257, "R=3"), (160, "R=T-1"), (33, "R=T+70"), (1, "R=0")])
def test_attention_ref_is_torch_sdpa_in_float64(T, mode):
    """no bias, a clamped bias, two unclamped ones and the one-frame batch: agreement to 1e-12"""
    from test_ops_gpu import _attention_ref

    c = _case(T, mode)
    qkv, table, gate, valid = A.case_inputs(c)
    x = qkv.astype(np.float64)
    ref = A.attention_ref(x, valid, B, T, H, table, gate, c.R)
    q, k, v = (torch.from_numpy(np.ascontiguousarray(t)) for t in A.heads(x, B, T, H))
    mask = torch.zeros((B, H, T, T), dtype=torch.float64)
    if table is not None:
        i, j = np.arange(T)[:, None], np.arange(T)[None, :]
        col = np.minimum(np.maximum(j - i, -c.R), c.R) + c.R  # written out again, not taken from the module under test
        mask += torch.from_numpy(gate.astype(np.float64))[..., None] * torch.from_numpy(table.astype(np.float64))[:, col][None]
    for b in range(B):
        mask[b, :, :, valid[b]:] = float("-inf")
    want = torch.nn.functional.scaled_dot_product_attention(q, k, v, attn_mask=mask, scale=1.0)
    want = want.permute(0, 2, 1, 3).reshape(B * T, 64 * H).numpy()
    assert ref.dtype == np.float64 and ref.shape == want.shape
    assert np.abs(ref - want).max() <= 1e-12
    # the function the existing attention tests score against is the same math
    theirs = _attention_ref(x.copy(), valid, B, T, H, None if table is None else table.astype(np.float64),
                            None if gate is None else gate.astype(np.float64), R=c.R)
    assert np.abs(ref - theirs).max() <= 1e-12


def test_operands_round_as_torch_does_and_once():
    qkv = A.case_inputs(_case(65, "none"))[0]
    D = 64 * H
    t = torch.from_numpy(qkv.copy())
    for dtype, tt in (("bf16", torch.bfloat16), ("fp16", torch.float16)):
        assert np.array_equal(A.round_to(qkv, dtype), t.to(tt).float().numpy())
        qdev, qref = A.operands(qkv, dtype)
        assert np.array_equal(qdev, torch.from_numpy(qdev).to(tt).float().numpy())  # exact in the operand type
        assert np.array_equal(qdev[:, :D], (t[:, :D] * np.float32(A.LOG2E)).to(tt).float().numpy())
        assert np.array_equal(qref[:, :D], qdev[:, :D].astype(np.float64) / A.LOG2E) and np.array_equal(qref[:, D:], qdev[:, D:])
    for dtype in ("fp32", "fp32x3"):
        qdev, qref = A.operands(qkv, dtype)
        assert np.array_equal(qdev, qkv) and np.array_equal(qref, qkv.astype(np.float64))


def test_the_case_list_is_what_the_sweep_claims():
    assert {c.T for c in A.CASES} == set(A.LENGTHS) and {c.mode for c in A.CASES} == set(A.MODES)
    assert [c.R for c in A.CASES if c.T == 1] == [None, 0, 3, 71]          # R = T - 2 < 0 and R = T - 1 = 0 dropped
    assert [c.R for c in A.CASES if c.T == 2] == [None, 0, 3, 1, 72]       # R = T - 2 = 0 dropped
    assert [c.R for c in A.CASES if c.T == 300] == [None, 0, 3, 298, 299, 370]
    assert A.cases_of("none") + A.cases_of("R=0") + A.cases_of("R=3") + A.cases_of("R=T-2") + A.cases_of("R=T-1") + \
        A.cases_of("R=T+70") == sorted(A.CASES, key=lambda c: A.MODES.index(c.mode))
    c = _case(257, "R=3")
    qkv = A.case_inputs(c)[0]
    k = qkv[:, 64 * H:128 * H]
    loud = np.flatnonzero(np.linalg.norm(k, axis=1) > 2.5 * np.median(np.linalg.norm(k, axis=1)))
    assert loud.tolist() == [257 // 2, 256]  # the two loud keys of utterance 0: T // 2 and valid[0] - 1


# ---- (b) ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", A.DTYPES)
def test_the_restated_flash_form_sits_under_a_quarter_of_the_row_band(dtype):
    """Every case of CASES; the smallest reference row norm stays far above the per-row floor of 1e-3.  Measured worst rows: fp32
    2.6e-6 (band 4e-5), bf16 2.6e-3 (3e-2), fp16 3.5e-4 (4e-3), fp32x3 3.0e-6 (1e-4).
    fp32x3 with q, k and v split into hi + lo bf16 as well (restate(..., x3_operands=True): three of four terms per product, what
    attn_x3_kernel multiplies) is printed beside it and NOT held to the quarter: its worst row is 7.5e-5 (T = 127, R = 0, a query
    of utterance 0, the one with the two loud keys), above 2.5e-5 at 76 of the 99 cases and 3.0e-5 on this draw even without a
    loud key.  That is the mode's operand error (|r| <= 2^-17 |x| per operand and the dropped lo lo term, on scores of a few
    units), which the reference on unrounded operands does not see — the same quantity the 16-bit modes keep out of their score
    by handing the reference the rounded operands.  No draw of this recipe brings it under a quarter of 1e-4; the row band of
    fp32x3 has a factor 1.3 of room over it, not 4."""
    band = A.row_band(dtype)
    worst, worst_at, least, worst_x3, worst_x3_at = 0.0, None, np.inf, 0.0, None
    for c in A.CASES:
        qkv, table, gate, valid = A.case_inputs(c)
        qdev = A.operands(qkv, dtype)[0]
        ref = A.case_reference(c, dtype)
        got = A.restate(qdev, valid, B, c.T, H, table, gate, c.R, dtype)
        assert got.shape == ref.shape and got.dtype == np.float32
        row = A.assert_rows(got, ref, band / 4, f"restated {dtype} T = {c.T} {c.mode} valid {c.valid}", T=c.T)
        assert A.rel_err(got, ref) < A.ATT_TOL[dtype] / 4
        least = min(least, float(np.linalg.norm(ref, axis=1).min()))
        if row > worst:
            worst, worst_at = row, c
        if dtype == "fp32x3":
            e = float(A.row_errors(A.restate(qdev, valid, B, c.T, H, table, gate, c.R, dtype, x3_operands=True), ref).max())
            if e > worst_x3:
                worst_x3, worst_x3_at = e, c
    print(f"restated {dtype}: worst row {worst:.2e} at T = {worst_at.T} {worst_at.mode} (band {band:.1e}), smallest |ref row| {least:.2f}")
    if dtype == "fp32x3":
        print(f"restated fp32x3 with split q, k, v: worst row {worst_x3:.2e} at T = {worst_x3_at.T} {worst_x3_at.mode}")
    assert least > 1.0


def test_r0_is_the_bias_free_result():
    """a bias constant along a query's keys does not move its softmax"""
    for T in (2, 129):
        c = _case(T, "R=0")
        assert np.abs(A.case_reference(c, "fp32") - A.case_reference(c, "fp32", biased=False)).max() < 1e-12


# ---- (c) ----------------------------------------------------------------------------------------------------------------------------
# where each fault can show: (T, mode) cases of CASES
FAULT_CASES = {
    "bias window shifted in the last query block": [(257, "R=3"), (257, "R=T-1"), (300, "R=T+70"), (65, "R=3")],
    "gate of the last query from row T-2": [(257, "R=T-2"), (257, "R=T-1"), (300, "R=T-2"), (300, "R=T+70"), (127, "R=3")],
    "gate of a block's first query from the row before": [(257, "R=3"), (257, "R=T-1"), (300, "R=3"), (300, "R=T-2"), (129, "R=T-1")],
    "clamp at R-1": [(257, "R=3"), (257, "R=T-2"), (65, "R=T-2"), (300, "R=3")],
    "key mask one key late": [(257, "none"), (257, "R=3"), (33, "none"), (300, "R=T-1")],
    "second 32-key half dropped at valid % 64 == 33": [(33, "none"), (33, "R=3"), (33, "R=T-1")],
    "one row left NaN": [(257, "R=3"), (1, "none")],
}
GATE_FAULTS = ("gate of the last query from row T-2", "gate of a block's first query from the row before")
LOOSEST = A.row_band("bf16")


def _apply(name, T, mode):
    c = _case(T, mode)
    qkv, table, gate, valid = A.case_inputs(c)
    qref = A.operands(qkv, "fp32")[1]
    return c, A.FAULTS[name](qref, valid, B, T, H, table, gate, c.R), A.case_reference(c, "fp32")


@pytest.mark.parametrize("name", list(A.FAULTS))
def test_the_row_score_names_each_fault_at_its_row(name):
    """Each fault moves some row past the bf16 row band, the loosest, and assert_rows names a row the fault touched, with its
    query block.  The whole-tensor score is printed beside it; the two gate faults stay under the bf16 whole-tensor bound."""
    assert set(FAULT_CASES) == set(A.FAULTS)
    hidden = []
    for T, mode in FAULT_CASES[name]:
        c, res, ref = _apply(name, T, mode)
        assert res is not None, (name, T, mode)
        bad, rows = res
        assert rows.shape == (B * T,) and rows.any()
        clean = A.row_errors(bad[~rows], ref[~rows])
        assert clean.size == 0 or clean.max() < 1e-12  # the fault is where it says and nowhere else
        whole = A.rel_err(bad, ref)
        with pytest.raises(AssertionError) as err:
            A.assert_rows(bad, ref, LOOSEST, f"{name}, T = {T} {mode}", T=T)
        msg = str(err.value)
        m, b, t, blk = (int(x) for x in re.search(r"row (\d+) of \d+ .* utterance (\d+), query (\d+) \(query block (\d+),", msg).groups())
        assert m == b * T + t and blk == t // A.QT and rows[m], msg
        if name == "one row left NaN":
            assert "is not finite" in msg and not whole <= A.ATT_TOL["bf16"]
            worst = float("nan")
        else:
            worst = float(A.row_errors(bad, ref).max())
            assert worst > LOOSEST
        if name == "bias window shifted in the last query block":
            assert blk == (T - 1) // A.QT
        if name == "gate of a block's first query from the row before":
            assert t % A.QT == 0 and t > 0
        if name == "gate of the last query from row T-2":
            assert t == T - 1
        print(f"{name}: T = {T} {mode} valid {c.valid}: whole-tensor {whole:.2e}, worst row {worst:.2e} at utterance {b} query {t}")
        if whole < A.ATT_TOL["bf16"]:
            hidden.append((T, mode))
    if name in GATE_FAULTS:  # the reason this file exists: a row wrong by tenths of itself inside the whole-tensor bf16 bound
        assert hidden, name


def test_clamp_at_r_minus_1_shows_up_to_t_minus_1_and_not_from_t_on():
    """A clamp at R - 1 moves every pair R or more apart.  The farthest pair, (query 0, key T - 1) and its mirror, is T - 1 apart: the
    fault shows at R = T - 2 (queries 0, 1, T - 2, T - 1, past the bf16 row band) and still moves queries 0 and T - 1 at R = T - 1
    (the exact window is not wide enough to hide it), and is invisible only from R = T on, where no key is R away — the list's
    R = T + 70."""
    for T in (65, 257):
        for mode, touched in (("R=T-2", (0, 1, T - 2, T - 1)), ("R=T-1", (0, T - 1)), ("R=T+70", ())):
            c, (bad, rows), ref = _apply("clamp at R-1", T, mode)
            e = A.row_errors(bad, ref)
            print(f"clamp at R-1: T = {T} {mode}: worst row {e.max():.2e}, rows touched {int(rows.sum())}")
            assert {int(m) % T for m in np.flatnonzero(rows)} <= set(touched)
            if touched:  # (at R = T - 1 one key of T moves for two queries: there, but not always past a band — 8.6e-3 at T = 257)
                assert e.max() > (LOOSEST if mode == "R=T-2" else 1e-6) and rows[int(np.argmax(e))] and e[~rows].max() == 0.0
            else:
                assert c.R >= T and not rows.any() and np.array_equal(bad, ref)


def test_faults_say_where_they_cannot_show():
    c = _case(65, "none")
    qkv, table, gate, valid = A.case_inputs(c)
    for name in ("bias window shifted in the last query block", "clamp at R-1") + GATE_FAULTS:
        assert A.FAULTS[name](qkv.astype(np.float64), valid, B, 65, H, None, None, None) is None
    c = _case(65, "R=3")
    qkv, table, gate, valid = A.case_inputs(c)
    assert A.FAULTS[GATE_FAULTS[1]](qkv.astype(np.float64), valid, B, 65, H, table, gate, 3) is None  # one query block
    assert 33 not in [v % 64 for v in c.valid]
    assert A.FAULTS["second 32-key half dropped at valid % 64 == 33"](qkv.astype(np.float64), valid, B, 65, H, table, gate, 3) is None


# ---- (d) ----------------------------------------------------------------------------------------------------------------------------
def test_a_nan_row_counts_as_failed():
    c = _case(33, "none")
    ref = A.case_reference(c, "fp32")
    got = ref.copy()
    got[40, 7] = np.nan
    with pytest.raises(AssertionError, match=r"row 40 of 99 .* utterance 1, query 7 .* is not finite \(1 such rows\)"):
        A.assert_rows(got, ref, 1e9, "nan", T=33)
    got[40, 7] = np.inf
    with pytest.raises(AssertionError, match="is not finite"):
        A.assert_rows(got, ref, 1e9, "inf", T=33)
    assert A.assert_rows(ref, ref, 1e-12, "same", T=33) == 0.0
