"""float64 numpy restatement of the wav2vec 2.0 Conformer encoder (TEST HELPER, not product code).

Restates ConformerEncoder.extract_features / ConformerEncoderLayer.forward and their modules
(s3prl/upstream/wav2vec2/wav2vec2_model.py:25-71 rotary, 165-252 rel_pos attention, 313-438 conv module / FFN,
440-578 layer, 1525-1588 RelPositionalEncoding, 3132-3211 encoder) on top of the front end of ``oracle.encoder_oracle``
(conv feature extractor, LayerNorm, post_extract_proj).  ``tests/test_conformer_cpu.py`` pins it against the fixtures the
reference itself produced (``tests/golden/make_golden_conformer.py``); the GPU op tests use its pieces as their float64 truth.
"""

from __future__ import annotations

import math
from typing import Dict, List, Optional, Sequence

import numpy as np

from oracle import encoder_oracle as O

EPS = 1e-5


def swish(x):
    return x / (1.0 + np.exp(-x))


def ffn(W, p, x):
    h = O.layer_norm(x, W[f"{p}.layer_norm.weight"], W[f"{p}.layer_norm.bias"])
    return swish(h @ W[f"{p}.w_1.weight"].T + W[f"{p}.w_1.bias"]) @ W[f"{p}.w_2.weight"].T + W[f"{p}.w_2.bias"]


def glu_dw_bn_swish(x2d: np.ndarray, dw: np.ndarray, bn: Dict[str, np.ndarray]) -> np.ndarray:
    """(B, T, 2D) pointwise_conv1 output -> swish(BN(DW(GLU(.)))) (B, T, D): depthwise Conv1d with zero padding (K-1)/2 over
    the batch-padded time axis, BatchNorm1d in eval (eps 1e-5).  dw: (D, K)."""
    B, T, D2 = x2d.shape
    D = D2 // 2
    K = dw.shape[-1]
    pad = (K - 1) // 2
    g = x2d[..., :D] * (1.0 / (1.0 + np.exp(-x2d[..., D:])))
    gp = np.zeros((B, T + 2 * pad, D), dtype=x2d.dtype)
    gp[:, pad:pad + T] = g
    y = np.zeros((B, T, D), dtype=x2d.dtype)
    for k in range(K):
        y += gp[:, k:k + T] * dw[:, k]
    y = (y - bn["running_mean"]) / np.sqrt(bn["running_var"] + EPS) * bn["weight"] + bn["bias"]
    return swish(y)


def conv_module(W, p, x):
    h = O.layer_norm(x, W[f"{p}.layer_norm.weight"], W[f"{p}.layer_norm.bias"])
    h = h @ W[f"{p}.pointwise_conv1.weight"][:, :, 0].T
    bn = {n: W[f"{p}.batch_norm.{n}"] for n in ("weight", "bias", "running_mean", "running_var")}
    h = glu_dw_bn_swish(h, W[f"{p}.depthwise_conv.weight"][:, 0, :], bn)
    return h @ W[f"{p}.pointwise_conv2.weight"][:, :, 0].T


def rope_tables(T: int, dh: int = 64):
    """cos, sin (T, dh) of RotaryPositionalEmbedding (fp32 formula, as the reference evaluates it)."""
    inv = (1.0 / (10000 ** (np.arange(0, dh, 2, dtype=np.float32) / dh))).astype(np.float32)
    f = np.outer(np.arange(T, dtype=np.float32), inv).astype(np.float32)
    emb = np.concatenate([f, f], axis=-1)
    return np.cos(emb.astype(np.float64)), np.sin(emb.astype(np.float64))


def rotate(x: np.ndarray, cos: np.ndarray, sin: np.ndarray) -> np.ndarray:
    """x (B, T, D) -> x * cos + rotate_half(x) * sin per 64-wide head chunk."""
    B, T, D = x.shape
    h = x.reshape(B, T, D // 64, 64)
    rh = np.concatenate([-h[..., 32:], h[..., :32]], axis=-1)
    return (h * cos[None, :, None, :] + rh * sin[None, :, None, :]).reshape(B, T, D)


def rel_pe(T: int, D: int) -> np.ndarray:
    """(2T-1, D) table of RelPositionalEncoding: row r holds relative position (T-1) - r."""
    pos = np.arange(T - 1, -T, -1, dtype=np.float32)[:, None]
    div = np.exp(np.arange(0, D, 2, dtype=np.float32) * np.float32(-(math.log(10000.0) / D))).astype(np.float32)
    a = (np.abs(pos) * div).astype(np.float32) * np.sign(pos + 0.5).astype(np.float32)
    pe = np.zeros((2 * T - 1, D), dtype=np.float64)
    pe[:, 0::2] = np.sin(a.astype(np.float64))
    pe[:, 1::2] = np.cos(a.astype(np.float64))
    return pe


def softmax_masked(s: np.ndarray, valid: Sequence[int]) -> np.ndarray:
    """s: (B, H, T, T) scores; keys >= valid[b] masked."""
    s = s.copy()
    for b, v in enumerate(valid):
        s[b, :, :, v:] = -np.inf
    s = s - s.max(-1, keepdims=True)
    e = np.exp(s)
    return e / e.sum(-1, keepdims=True)


def relpos_scores(q: np.ndarray, k: np.ndarray, P: np.ndarray, qadd: np.ndarray) -> np.ndarray:
    """score(i, j) = q_i . k_j + (q_i + qadd_h) . P_h[(j - i) + T - 1]: q, k (B, H, T, 64), P (2T-1, H, 64), qadd (H, 64)."""
    T = q.shape[2]
    ac = q @ k.transpose(0, 1, 3, 2)
    bd_full = np.einsum("bhtd,rhd->bhtr", q + qadd[None, :, None, :], P)  # (B, H, T, 2T-1)
    idx = np.arange(T)[None, :] - np.arange(T)[:, None] + T - 1           # [i, j] -> (j - i) + T - 1
    bd = np.take_along_axis(bd_full, np.broadcast_to(idx, bd_full.shape[:2] + idx.shape), axis=-1)
    return ac + bd


def attention(cfg, W, p, x: np.ndarray, valid) -> np.ndarray:
    B, T, D = x.shape
    H = cfg.encoder_attention_heads
    a = f"{p}.self_attn"
    if cfg.pos_enc_type == "rope":
        cos, sin = rope_tables(T)
        xr = rotate(x, cos, sin)
        q = xr @ W[f"{a}.linear_q.weight"].T + W[f"{a}.linear_q.bias"]
        k = xr @ W[f"{a}.linear_k.weight"].T + W[f"{a}.linear_k.bias"]
    else:
        q = x @ W[f"{a}.linear_q.weight"].T + W[f"{a}.linear_q.bias"]
        k = x @ W[f"{a}.linear_k.weight"].T + W[f"{a}.linear_k.bias"]
    v = x @ W[f"{a}.linear_v.weight"].T + W[f"{a}.linear_v.bias"]
    sh = lambda t: t.reshape(B, T, H, 64).transpose(0, 2, 1, 3)  # noqa: E731
    q, k, v = sh(q), sh(k), sh(v)
    if cfg.pos_enc_type == "rope":
        s = (q @ k.transpose(0, 1, 3, 2)) / 8.0
    else:
        P = (rel_pe(T, D) @ W[f"{a}.linear_pos.weight"].T).reshape(2 * T - 1, H, 64)
        u, vb = W[f"{a}.pos_bias_u"], W[f"{a}.pos_bias_v"]
        s = relpos_scores((q + u[None, :, None, :]) / 8.0, k, P, (vb - u) / 8.0)
    o = softmax_masked(s, valid) @ v
    o = o.transpose(0, 2, 1, 3).reshape(B, T, D)
    return o @ W[f"{a}.linear_out.weight"].T + W[f"{a}.linear_out.bias"]


def conformer_layer(cfg, W, l: int, x: np.ndarray, valid) -> np.ndarray:
    p = f"encoder.layers.{l}"
    x = x + 0.5 * ffn(W, f"{p}.ffn1", x)
    x = x + attention(cfg, W, p, O.layer_norm(x, W[f"{p}.self_attn_layer_norm.weight"], W[f"{p}.self_attn_layer_norm.bias"]),
                      valid)
    x = x + conv_module(W, f"{p}.conv_module", x)
    x = x + 0.5 * ffn(W, f"{p}.ffn2", x)
    return O.layer_norm(x, W[f"{p}.final_layer_norm.weight"], W[f"{p}.final_layer_norm.bias"])


def forward(cfg, weights: Dict[str, np.ndarray], wavs: List[np.ndarray], n_max: Optional[int] = None) -> List[np.ndarray]:
    """hidden_states of the wav2vec2 expert on a Conformer: [input of layer 0 .. input of layer NL-1, encoder output]."""
    dt = np.float64
    W = {k: v.astype(dt) for k, v in weights.items()}
    lens = [len(w) for w in wavs]
    n_max = n_max or max(lens)
    B = len(wavs)
    padded = np.zeros((B, n_max), dtype=dt)
    for b, w in enumerate(wavs):
        w = w.astype(dt)
        padded[b, :lens[b]] = O.wav_normalize(w) if cfg.normalize else w
    x = O.feature_extractor(cfg, W, padded)
    valid = [cfg.valid_frames(n, n_max) for n in lens]
    x = O.layer_norm(x, W["layer_norm.weight"], W["layer_norm.bias"])
    x = x @ W["post_extract_proj.weight"].T + W["post_extract_proj.bias"]
    for b in range(B):
        x[b, valid[b]:] = 0
    if not cfg.layer_norm_first:
        x = O.layer_norm(x, W["encoder.layer_norm.weight"], W["encoder.layer_norm.bias"])
    hidden = []
    for l in range(cfg.encoder_layers):
        hidden.append(x)
        x = conformer_layer(cfg, W, l, x, valid)
    if cfg.layer_norm_first:
        x = O.layer_norm(x, W["encoder.layer_norm.weight"], W["encoder.layer_norm.bias"])
    hidden.append(x)
    return hidden
