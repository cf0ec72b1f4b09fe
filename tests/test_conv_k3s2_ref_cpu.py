"""Pins the yardstick of tests/test_conv_k3s2_gpu.py (tests/conv_k3s2_ref.py) against torch.nn.functional.conv1d in float64, then
shows (a) that on the sweep's draw the two-output form restated in float32 stays below OP_TOL / 8 per row — the inputs are fair
and the form alone sits far inside the bound —, (b) that the per-row score names the row of each fault the sweep exists for, and
(c) that a NaN row counts as failed."""

import math

import numpy as np
import pytest
import torch

import conv_k3s2_ref as R

WIDTHS = [32, 96, 128, 160, 512]
LENGTHS = [1, 2, 3, 63, 64, 65, 127, 128, 129, 130, 257]


def _torch_conv(x, w, bias, act, dtype, k=3):
    y = torch.nn.functional.conv1d(torch.from_numpy(x).to(dtype).transpose(1, 2), torch.from_numpy(w).to(dtype),
                                   None if bias is None else torch.from_numpy(bias).to(dtype), stride=2).transpose(1, 2)
    assert w.shape[2] == k
    return (0.5 * y * (1.0 + torch.erf(y / math.sqrt(2.0)))) if act else y


@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("M", [1, 2, 64, 129])
def test_conv_ref_is_torch_conv1d_at_stride_2(M, act):
    rng = np.random.default_rng(10 * M + act)
    x, w, bias = R.draw(rng, 3, 2 * M + 1, 96)
    ref = R.conv_ref(x, w, bias, M, act)
    want = _torch_conv(x, w, bias, act, torch.float64).numpy()
    assert ref.dtype == np.float64 and ref.shape == want.shape == (3, M, 96)
    assert np.abs(ref - want).max() < 1e-12 * (1.0 + np.abs(want).max())
    assert np.abs(R.conv_ref(x, w, None, M, act) - _torch_conv(x, w, None, act, torch.float64).numpy()).max() < 1e-10
    # a frame behind 2M changes nothing, and conv5-6's k = 2 is the same sum without its last tap
    longer = np.concatenate([x, np.full((3, 1, 96), np.nan, dtype=np.float32)], axis=1)
    assert np.array_equal(R.conv_ref(longer, w, bias, M, act), ref)
    w2 = np.ascontiguousarray(w[:, :, :2])
    want2 = _torch_conv(x[:, :2 * M], w2, bias, act, torch.float64, k=2).numpy()
    assert np.abs(R.conv_ref(x, w2, bias, M, act, k=2) - want2).max() < 1e-12 * (1.0 + np.abs(want2).max())
    assert np.sqrt((ref ** 2).sum(-1)).min() > 1.0  # the draw keeps every row far from the per-row floor


@pytest.mark.parametrize("C", WIDTHS)
def test_the_two_output_form_in_float32_sits_far_inside_the_bound(C):
    """(a) worst row below OP_TOL / 8 and no element near the cap, at every length of the list and both activations; torch's own
    fp32 conv1d on the same rows is printed beside it."""
    worst = worst_t = worst_el = 0.0
    for M in LENGTHS:
        for act in (0, 1):
            x, w, bias = R.draw(np.random.default_rng(1000 * C + 2 * M + act), 3, R.frames_for(M), C)
            ref = R.conv_ref(x, w, bias, M, act)
            got = R.two_output_f32(x, w, bias, M, act)
            assert got.shape == ref.shape and got.dtype == np.float32
            whole, row, at, off = R.row_scores(got, ref)
            theirs = R.row_scores(_torch_conv(x[:, :2 * M + 1], w, bias, act, torch.float32).numpy(), ref)
            el = float((np.abs(got - ref) / (1.0 + np.abs(ref))).max())
            worst, worst_t, worst_el = max(worst, row), max(worst_t, theirs[1]), max(worst_el, el)
            assert row < R.OP_TOL / 8 and off == 0, (C, M, act, whole, row, at, off)
    print(f"two-output fp32 C={C}: worst row {worst:.2e} (torch fp32 conv1d {worst_t:.2e}), worst element {worst_el:.2e} (1 + |ref|)")


def _faults(x, w, bias, M, act):
    """three results that are right but for one fault each -> {name: (result, (b, row) of the fault)}"""
    C = w.shape[0]
    good = R.two_output_f32(x, w, bias, M, act)
    out = {}
    # the last row of an odd M computed with frame 2M + 1 instead of 2M (a clamp one frame late)
    late = x[:, :2 * M + 2].copy()
    late[:, 2 * M] = late[:, 2 * M + 1]
    bad = good.copy()
    bad[0, M - 1] = R.two_output_f32(late, w, bias, M, act)[0, M - 1]
    out["clamp one frame late"] = (bad, (0, M - 1))
    # one 16-channel K chunk of the odd tap dropped on one row
    cut = x.copy()
    cut[2, 2 * 130 + 1, C - 16:] = 0.0
    bad = good.copy()
    bad[2, 130] = R.two_output_f32(cut, w, bias, M, act)[2, 130]
    out["K chunk dropped"] = (bad, (2, 130))
    # rows 2u and 2u + 1 of one pair swapped
    bad = good.copy()
    bad[0, [126, 127]] = good[0, [127, 126]]
    out["pair swapped"] = (bad, (0, 126))
    return good, out


def test_the_row_score_names_each_fault_at_its_row():
    """(b) at M = 257, C = 512, every fault in a quiet utterance beside the loud one.  Each fault is one wrong row among 771, and the
    per-row score names it.  The whole-tensor score is printed beside it: it moves by the row's error over the norm of all rows
    (about 1 / 480 of it on this draw).  Measured: clamp one frame late 1.5e-3, K chunk dropped 1.5e-4, pair swapped 3.8e-3 — a row
    that is wrong by a tenth or more of itself still moves the whole-tensor score past 2e-5, but only says "somewhere"; a row wrong
    by less than about 1e-2 of itself passes a whole-tensor bound of 2e-5 outright.  That is the fourth case: one frame of one
    row rounded to bf16 (whole 2.1e-6, the row 9.6e-4), the size of a wrong accumulation format rather than of a wrong address."""
    M, C, act = 257, 512, 1
    x, w, bias = R.draw(np.random.default_rng(5), 3, R.frames_for(M), C)
    ref = R.conv_ref(x, w, bias, M, act)
    good, faults = _faults(x, w, bias, M, act)
    assert R.row_scores(good, ref)[1] < R.OP_TOL / 8
    for name, (bad, (b, t)) in faults.items():
        whole, row, at, off = R.row_scores(bad, ref)
        print(f"{name}: whole {whole:.2e}, worst row {row:.2e} at {divmod(at, M)}, elements off {off}")
        assert row > 100 * R.OP_TOL and off > 0, (name, row, off)
        assert divmod(at, M) in ((b, t), (b, t + 1)) if name == "pair swapped" else divmod(at, M) == (b, t), (name, divmod(at, M))
    # the subtle one: frame 4u + 1 of one row rounded to bf16 (2^-9 relative on a third of the row's sum)
    rough = x.copy()
    v = rough[0, 2 * 200 + 1].view(np.uint32)
    rough[0, 2 * 200 + 1] = ((v + 0x8000) & 0xFFFF0000).astype(np.uint32).view(np.float32)
    bad = good.copy()
    bad[0, 200] = R.two_output_f32(rough, w, bias, M, act)[0, 200]
    whole, row, at, off = R.row_scores(bad, ref)
    print(f"one frame in bf16: whole {whole:.2e}, worst row {row:.2e} at {divmod(at, M)}, elements off {off}")
    assert whole < R.OP_TOL, whole                      # the whole-tensor rule lets it through
    assert row > 10 * R.OP_TOL and divmod(at, M) == (0, 200)  # the per-row rule names it


def test_a_nan_row_counts_as_failed():
    """(c)"""
    M, C = 5, 32
    x, w, bias = R.draw(np.random.default_rng(6), 3, R.frames_for(M), C)
    ref = R.conv_ref(x, w, bias, M, 1)
    got = R.two_output_f32(x, w, bias, M, 1)
    got[2, 3, 7] = np.nan
    whole, row, at, off = R.row_scores(got, ref)
    assert row == float("inf") and divmod(at, M) == (2, 3) and off == 1 and not whole <= R.OP_TOL
