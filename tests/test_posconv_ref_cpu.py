"""Pins the yardstick of tests/test_posconv_edges_gpu.py (tests/posconv_ref.py) against torch.nn.functional.conv1d in float64: the
SamePad trim at an odd and an even K (nothing trimmed / the last frame dropped), the group order, the erf-GELU, and the shift
helper — the frames of an utterance embedded in zero rows see the same windows as the utterance alone.  The last test feeds the
scores a fault of the kind they exist for."""

import math

import numpy as np
import pytest
import torch

from posconv_ref import TAIL, UTT, conv_branch_ref, draw, embed, frame_scores


def _torch_branch(x, w, bias, G):
    K = w.shape[2]
    y = torch.nn.functional.conv1d(torch.from_numpy(x).double().transpose(1, 2), torch.from_numpy(w).double(),
                                   torch.from_numpy(bias).double(), padding=K // 2, groups=G)
    if K % 2 == 0:
        y = y[:, :, :-1]  # SamePad
    y = y.transpose(1, 2)
    return (0.5 * y * (1.0 + torch.erf(y / math.sqrt(2.0)))).numpy()


@pytest.mark.parametrize("K", [1, 15, 16, 128])
@pytest.mark.parametrize("T", [1, 17, 130])
def test_conv_branch_ref_is_torch_conv1d_with_samepad(K, T):
    rng = np.random.default_rng(100 * K + T)
    B, D, G = 2, 96, 3
    x, w, bias = draw(rng, B, T, D, G, K)
    ref = conv_branch_ref(x, w, bias, G)
    want = _torch_branch(x, w, bias, G)
    assert ref.dtype == np.float64 and ref.shape == (B, T, D)
    assert np.abs(ref - want).max() < 1e-12 * (1.0 + np.abs(want).max())
    assert np.sqrt((ref ** 2).sum(-1)).min() > 1.0  # the draw keeps every frame far from the per-frame floor


@pytest.mark.parametrize("K", [15, 16])
@pytest.mark.parametrize("s", [0, 1, 17, 129])
def test_embedded_utterance_sees_the_same_windows(K, s):
    rng = np.random.default_rng(7 + K)
    B, D, G = 2, 64, 2
    u, w, bias = draw(rng, B, UTT, D, G, K)
    e = embed(u, s)
    assert e.shape == (B, s + UTT + TAIL, D) and np.array_equal(e[:, s:s + UTT], u)
    assert not e[:, :s].any() and not e[:, s + UTT:].any()
    alone = _torch_branch(u, w, bias, G)
    inside = conv_branch_ref(e, w, bias, G)[:, s:s + UTT]
    assert np.abs(inside - alone).max() < 1e-12 * (1.0 + np.abs(alone).max())


def test_frame_scores_name_a_tap_dropped_on_three_frames():
    """The last tap dropped on the last three frames of a 256-frame tile in one of four batches: the whole-tensor error stays under the
    bf16 bound that test_posconv used to apply (1.2e-2), the per-frame score, the element count and the (batch, group) score do
    not, and the worst frame is one of the three.  The clean result rounded to fp32 passes everything."""
    tol = 2e-5
    B, T, D, G, K = 4, 385, 256, 8, 16
    x, w, bias = draw(np.random.default_rng(11), B, T, D, G, K)
    ref = conv_branch_ref(x, w, bias, G)
    w_drop = w.copy()
    w_drop[:, :, K - 1] = 0.0
    bad = ref.copy()
    bad[1, 253:256] = conv_branch_ref(x, w_drop, bias, G)[1, 253:256]
    tref = torch.from_numpy(ref)
    whole, fmax, farg, nbad, bmax, barg = frame_scores(torch.from_numpy(bad.astype(np.float32)), tref, tol, G).tolist()
    assert 1e-3 < whole < 1.2e-2
    assert fmax > 0.05 and divmod(int(farg), T)[0] == 1 and 253 <= divmod(int(farg), T)[1] < 256
    assert nbad > 100 and bmax > 2 * tol and int(barg) // G == 1
    whole, fmax, farg, nbad, bmax, barg = frame_scores(torch.from_numpy(ref.astype(np.float32)), tref, tol, G).tolist()
    assert whole < 1e-7 and fmax < 1e-7 and nbad == 0 and bmax < 1e-7
    nan = ref.astype(np.float32)
    nan[0, 7, 3] = np.nan
    whole, fmax, farg, nbad, bmax, barg = frame_scores(torch.from_numpy(nan), tref, tol, G).tolist()
    assert fmax == float("inf") and int(farg) == 7 and nbad == 1 and not whole <= tol
