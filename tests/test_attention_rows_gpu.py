"""s3enc_op_attention per query row against float64, over more than one 128-query block, with the WavLM bias and its gate, at every
clamp regime and at T below one key tile — the cases of tests/attention_ref.py (CASES: B = 3, H = 3, T = 1 .. 300, ragged valid at
the edges of the 32- and 64-key tiles), whose yardstick tests/test_attention_ref_cpu.py pins without a GPU.

Per case: the output goes into a NaN-prefilled buffer with 32 guard rows behind row B*T; every query row — the padded ones, t >=
valid[b], are computed by the kernels and scored like the rest — is held to the row band 2 * ATT_TOL[dtype] against
attention_ref on operands(...), the whole tensor to ATT_TOL[dtype]; R = 0 is also scored against the bias-free reference (a bias
constant along a query's keys is softmax-invariant); and for fp32, bf16 and fp16 the persistent form (tuning key attn_persist = 1)
must give the one-shot grid's bits, so it inherits the per-row score at every shape (fp32x3 has no persistent form).

Worst row measured on the MI355X per dtype and bias mode (the bands are the project's, not derived from these):
    dtype    band     none              R=0               R=3               R=T-2             R=T-1             R=T+70
    fp32     4e-5     2.06e-06 (T=300)  2.01e-06 (T=255)  3.29e-06 (T=300)  1.86e-06 (T=257)  2.41e-06 (T=255)  1.82e-06 (T=63)
    bf16     3e-2     4.01e-03 (T=160)  3.93e-03 (T=191)  3.53e-03 (T=255)  3.67e-03 (T=255)  3.76e-03 (T=256)  3.70e-03 (T=256)
    fp16     4e-3     4.58e-04 (T=300)  4.75e-04 (T=257)  4.41e-04 (T=160)  4.44e-04 (T=160)  5.13e-04 (T=129)  4.63e-04 (T=257)
    fp32x3   1e-4     5.17e-05 (T=257)  7.46e-05 (T=127)  5.46e-05 (T=160)  6.92e-05 (T=256)  5.50e-05 (T=128)  5.97e-05 (T=256)
fp32x3 sits closest to its band: 7.5e-5 of 1e-4, in utterance 0 (the two loud keys).  That is the mode's operand error, not a wrong
row: attention_ref.restate(..., x3_operands=True), the same three-term products on hi + lo bf16 splits of q, k and v on the CPU,
gives 7.48e-5 at the same case (T = 127, R = 0) and the kernel 7.46e-5.  No band was moved.
The 24 tests take 4 s together (the float64 references are computed once per case and operand rounding and shared).
"""

import pytest

import attention_ref as A
from test_ops_gpu import _dev, _ptr, _torch
from test_row_edges_gpu import assert_guards, guarded

pytestmark = pytest.mark.gpu

B, H = A.B, A.H
D = 64 * H


def _run(lib, dtype, c, dq, dvalid, dtable, dgate, what):
    """one launch into a guarded buffer -> (the (B*T, D) device view, its values as float numpy)"""
    from s3prl_amd import _lib

    torch = _torch()
    buf, out = guarded(B * c.T, D, dq.dtype)
    _lib.check(lib.s3enc_op_attention(_lib.DTYPES[dtype], _ptr(dq), _ptr(out), _ptr(dvalid), B, c.T, H, _ptr(dtable),
                                      0 if c.R is None else c.R, _ptr(dgate), None), what)
    torch.cuda.synchronize()
    assert_guards(buf, B * c.T, D, what)
    return out, out.float().cpu().numpy()


@pytest.mark.parametrize("mode", A.MODES)
@pytest.mark.parametrize("dtype", A.DTYPES)
def test_attention_rows_against_float64(dtype, mode):
    torch = _torch()
    from s3prl_amd import _lib

    lib = _lib.load()
    band = A.row_band(dtype)
    worst, worst_at = 0.0, None
    for c in A.cases_of(mode):
        qkv, table, gate, valid = A.case_inputs(c)
        ref = A.case_reference(c, dtype)
        dq = _dev(A.operands(qkv, dtype)[0].copy(), dtype)  # (copies: the case's arrays are read-only)
        dvalid = torch.from_numpy(valid.copy()).cuda()
        dtable = None if table is None else _dev(table.copy())  # (kept alive across the calls)
        dgate = None if gate is None else _dev(gate.copy())
        what = f"attention {dtype} T = {c.T} {c.mode} (R = {c.R}) valid {list(c.valid)}"
        out, got = _run(lib, dtype, c, dq, dvalid, dtable, dgate, what)
        row = A.assert_rows(got, ref, band, what, T=c.T)  # (a row that is not finite fails here)
        whole = A.rel_err(got, ref)
        assert whole < A.ATT_TOL[dtype], f"{what}: whole-tensor {whole:.3e}"
        if c.R == 0:
            A.assert_rows(got, A.case_reference(c, dtype, biased=False), band, what + " against the bias-free reference", T=c.T)
        if row > worst:
            worst, worst_at = row, c
        if dtype == "fp32x3":
            continue
        try:
            _lib.check(lib.s3enc_set_tuning(b"attn_persist", 1))
            pout, _ = _run(lib, dtype, c, dq, dvalid, dtable, dgate, what + " attn_persist = 1")
        finally:
            _lib.check(lib.s3enc_set_tuning(b"attn_persist", 0))
        bits = torch.int32 if dq.dtype == torch.float32 else torch.int16
        same = out.view(bits) == pout.view(bits)
        if not bool(same.all()):
            m = int((~same).any(dim=1).nonzero()[0])
            raise AssertionError(f"{what}: the persistent form differs from the one-shot grid in {int((~same).any(dim=1).sum())} rows, "
                                 f"first {A.row_name(m, B * c.T, c.T)}")
    print(f"attention rows {dtype} {mode}: worst row {worst:.2e} at T = {worst_at.T} valid {list(worst_at.valid)} (band {band:.1e})")
