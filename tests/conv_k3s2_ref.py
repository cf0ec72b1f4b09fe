"""float64 yardstick of the k = 3, stride-2 conv sweep (tests/test_conv_k3s2_gpu.py): the operand draw, the float64 reference
act(Conv1d(C, C, 3, stride = 2)(x) + bias) on channel-last rows, and a float32 numpy restatement of the two-output form that
convf22.hip computes (P, y[2u], y[2u + 1] as in the kernel's header comment).  tests/test_conv_k3s2_ref_cpu.py pins the
reference against torch.nn.functional.conv1d in float64, shows that the restatement sits far inside the op bound on this draw,
and feeds the per-row scores the faults they exist for (no GPU needed).

The loudness is per utterance, never per frame: the two-output form subtracts neighbouring frames, and a loud frame next to a
quiet one would measure the conditioning of that subtraction, not the kernel."""

import numpy as np

from oracle import encoder_oracle as O

OP_TOL = 2e-5   # the project's op bound
LOUD = 30.0     # utterance 1 against the others


def frames_for(M):
    """frames of an utterance whose M outputs read up to frame 2M, and one more that nothing may read"""
    return 2 * M + 2


def draw(rng, B, L, C):
    """x (B, L, C) ~ N(0, 1) with utterance 1 LOUD times louder, w (C, C, 3) ~ N(0, 1) / sqrt(3C), bias (C) ~ 0.5 N(0, 1)"""
    x = rng.standard_normal((B, L, C)).astype(np.float32)
    if B > 1:
        x[1] *= LOUD
    w = (rng.standard_normal((C, C, 3)) / np.sqrt(3 * C)).astype(np.float32)
    bias = (0.5 * rng.standard_normal(C)).astype(np.float32)
    return x, w, bias


def conv_ref(x, w, bias, M, act, k=3):
    """(B, M, C) float64: y[b][t] = act(sum_j W[:, :, j] x[b][2t + j] + bias), act 0 none / 1 erf-GELU; bias may be None.
    k = 2 is conv5-6's shape (w (C, C, 2))."""
    x = np.asarray(x, dtype=np.float64)
    w = np.asarray(w, dtype=np.float64)
    assert w.shape[2] == k and x.shape[1] >= 2 * (M - 1) + k, (w.shape, x.shape, M)
    y = np.zeros((x.shape[0], M, w.shape[0]))
    for j in range(k):
        y += x[:, j:j + 2 * M:2][:, :M] @ w[:, :, j].T
    if bias is not None:
        y += np.asarray(bias, dtype=np.float64)
    return O.gelu(y) if act else y


def two_output_f32(x, w, bias, M, act):
    """The two-output form in float32 (products and sums in float32, the association of convf22.hip), frames past 2M clamped to
    it as the kernel clamps them; the GELU is taken in float64 on the float32 sum and rounded once.  (B, M, C) float32."""
    x = np.asarray(x, dtype=np.float32)
    w0, w1, w2 = (np.ascontiguousarray(w[:, :, j].T, dtype=np.float32) for j in range(3))
    wp = (w0 + w2).astype(np.float32)
    U = (M + 1) // 2
    f = lambda d: x[:, np.minimum(4 * np.arange(U) + d, 2 * M)]  # noqa: E731
    x0, x1, x2, x3, x4 = (f(d) for d in range(5))
    P = x2 @ wp
    ye = ((x1 @ w1) + ((x0 - x2) @ w0)) + P
    yo = ((x3 @ w1) + ((x4 - x2) @ w2)) + P
    y = np.empty((x.shape[0], 2 * U, w.shape[0]), dtype=np.float32)
    y[:, 0::2], y[:, 1::2] = ye, yo
    y = y[:, :M]
    if bias is not None:
        y = y + np.asarray(bias, dtype=np.float32)
    assert y.dtype == np.float32
    return O.gelu(y.astype(np.float64)).astype(np.float32) if act else y


def row_scores(got, ref, tol=OP_TOL):
    """posconv_ref.frame_scores on numpy or torch operands: (whole, worst row, its flat index b * M + t, elements off)"""
    import torch

    import posconv_ref as PR

    g = got if isinstance(got, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(got))
    r = ref if isinstance(ref, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(ref))
    s = PR.frame_scores(g, r.to(g.device), tol).tolist()
    return s[0], s[1], int(s[2]), int(s[3])
