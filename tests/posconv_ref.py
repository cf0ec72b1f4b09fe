"""float64 yardstick of the positional-conv edge sweep (tests/test_posconv_edges_gpu.py): the conv branch
GELU(SamePad(Conv1d(D, D, K, padding=K // 2, groups=G)(x)) + bias) on operands the caller has already rounded to what the kernel
sees, the operand draw, the shift helper of the "a frame's bits do not depend on where it sits" check, and the per-frame scores.
tests/test_posconv_ref_cpu.py pins the first two against torch.nn.functional.conv1d in float64 and shows that the scores name a
tap dropped on three frames which the whole-tensor score lets through (no GPU needed)."""

import numpy as np

from oracle import encoder_oracle as O

UTT = 70    # frames of the utterance that the shift check embeds
TAIL = 16   # zero rows behind it
FLOOR = 1e-3  # under the per-frame / per-block norm of the reference


def draw(rng, B, T, D, G, K):
    """x ~ N(0, 1), w ~ 3 N(0, 1) / sqrt(Dg K), bias ~ N(0, 1): the conv output has a standard deviation of about 3, so GELU is used on
    both sides of its bend and every frame's norm over D stays far from the floor of the per-frame score."""
    Dg = D // G
    x = rng.standard_normal((B, T, D)).astype(np.float32)
    w = (3.0 * rng.standard_normal((D, Dg, K)) / np.sqrt(Dg * K)).astype(np.float32)
    bias = rng.standard_normal(D).astype(np.float32)
    return x, w, bias


def conv_branch_ref(x, w, bias, G):
    """(B, T, D) float64: GELU of the grouped SamePad conv of x (B, T, D) with w (D, D / G, K) and bias (D,)."""
    y = O.grouped_conv_same(np.asarray(x, dtype=np.float64), np.asarray(w, dtype=np.float64), np.asarray(bias, dtype=np.float64), G)
    assert y.shape == tuple(x.shape), (y.shape, x.shape)
    return O.gelu(y)


def embed(u, s, tail=TAIL):
    """The utterance u (B, n, D) behind s zero rows and in front of `tail` zero rows: (B, s + n + tail, D)."""
    B, n, D = u.shape
    out = np.zeros((B, s + n + tail, D), dtype=u.dtype)
    out[:, s:s + n] = u
    return out


def frame_scores(branch, ref, tol, G=None):
    """Scores of a conv branch (B, T, D) against ref (float64, same shape), torch tensors on one device; returns six float64 values
    on that device: whole-tensor relative error, the worst per-frame relative error (over D for each (b, t), the frame's reference
    norm floored at FLOOR) and its flat index b * T + t, the count of elements off by more than 50 * tol * (1 + |ref|) (NaN counts),
    and — with G — the worst relative error of a (batch, group) block over its T x Dg elements and its flat index b * G + g."""
    import torch

    B, T, D = ref.shape
    inf = float("inf")
    d = branch.double() - ref
    whole = d.norm() / ref.norm().clamp_min(1e-30)
    fr = torch.nan_to_num(d.norm(dim=2) / ref.norm(dim=2).clamp_min(FLOOR), nan=inf).reshape(-1)
    fmax, farg = fr.max(dim=0)
    nbad = (~(d.abs() <= 50.0 * tol * (1.0 + ref.abs()))).sum().double()
    if G:
        num = d.view(B, T, G, D // G).pow(2).sum(dim=(1, 3)).sqrt()
        den = ref.view(B, T, G, D // G).pow(2).sum(dim=(1, 3)).sqrt().clamp_min(FLOOR)
        bmax, barg = torch.nan_to_num(num / den, nan=inf).reshape(-1).max(dim=0)
    else:
        bmax, barg = torch.zeros_like(whole), torch.zeros_like(farg)
    return torch.stack([whole, fmax, farg.double(), nbad, bmax, barg.double()])
