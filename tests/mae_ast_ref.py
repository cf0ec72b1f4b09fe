"""float64 restatement of the MAE-AST upstream behind its front end (s3prl/upstream/mae_ast/{expert,mae_ast}.py): the eval
BatchNorm2d(1, affine=False) times 0.5, nn.Unfold into kt x kc patches, post_extract_proj, the checkpoint's own sinusoidal rows on
the live tokens, the Transformer encoder with key padding, and the expert's reshape.  The front end itself is
``oracle/fbank_oracle.py::kaldi_fbank(num_mel_bins=128)``.  Written from the reference's source, never from the HIP path; the
fixtures under tests/golden/mae_ast/ are REAL runs of the reference model and this file is checked against them
(tests/test_mae_ast_cpu.py)."""

from __future__ import annotations

import math

import numpy as np

from oracle.fbank_oracle import kaldi_fbank

LN_EPS = 1e-5

_erf = np.vectorize(math.erf, otypes=[np.float64])


def features(wavs, feature_dtype=np.float64):
    """expert.py:68-80: per utterance fbank at 128 bins, zero-padded to the longest (pad_sequence): (B, Fmax, 128), frame counts.
    ``feature_dtype=np.float32`` rounds the features once to float32, as the fixtures' generator hands them to the reference."""
    feats = [kaldi_fbank(np.asarray(w, np.float64), num_mel_bins=128).astype(feature_dtype).astype(np.float64) for w in wavs]
    F = [len(f) for f in feats]
    x = np.zeros((len(feats), max(F), 128))
    for b, f in enumerate(feats):
        x[b, :len(f)] = f
    return x, F


def key_counts(F, kt, kc, Ttok):
    """forward_padding_mask (mae_ast.py:305-325) as the number of leading un-masked tokens per utterance.  The fast exit (nothing
    padded in the last frame column) and an index at or beyond Ttok both mask nothing."""
    V = 128 // kc
    return [min(((f - 1) // kt + 1) * V, Ttok) for f in F]


def layer_norm(x, g, b):
    mu = x.mean(-1, keepdims=True)
    var = ((x - mu) ** 2).mean(-1, keepdims=True)
    return (x - mu) / np.sqrt(var + LN_EPS) * g + b


def gelu(x):
    return 0.5 * x * (1.0 + _erf(x / math.sqrt(2.0)))


def _w(weights, name):
    return np.asarray(weights[name], np.float64)


def attention(x, weights, p, H, kv):
    """fairseq MultiheadAttention, self-attention with a key padding mask: x (T, D), keys at or past kv masked with -inf."""
    T, D = x.shape
    hd = D // H
    q = (x @ _w(weights, p + ".q_proj.weight").T + _w(weights, p + ".q_proj.bias")) * hd ** -0.5
    k = x @ _w(weights, p + ".k_proj.weight").T + _w(weights, p + ".k_proj.bias")
    v = x @ _w(weights, p + ".v_proj.weight").T + _w(weights, p + ".v_proj.bias")
    out = np.empty((T, D))
    for h in range(H):
        s = q[:, h * hd:(h + 1) * hd] @ k[:kv, h * hd:(h + 1) * hd].T
        s = np.exp(s - s.max(-1, keepdims=True))
        out[:, h * hd:(h + 1) * hd] = (s / s.sum(-1, keepdims=True)) @ v[:kv, h * hd:(h + 1) * hd]
    return out @ _w(weights, p + ".out_proj.weight").T + _w(weights, p + ".out_proj.bias")


def encoder_layer(x, weights, p, H, kv, pre_ln):
    """TransformerSentenceEncoderLayer (mae_ast.py:745-799)."""
    ln1 = lambda t: layer_norm(t, _w(weights, p + ".self_attn_layer_norm.weight"), _w(weights, p + ".self_attn_layer_norm.bias"))
    ln2 = lambda t: layer_norm(t, _w(weights, p + ".final_layer_norm.weight"), _w(weights, p + ".final_layer_norm.bias"))
    ffn = lambda t: gelu(t @ _w(weights, p + ".fc1.weight").T + _w(weights, p + ".fc1.bias")) @ _w(weights, p + ".fc2.weight").T + \
        _w(weights, p + ".fc2.bias")
    if pre_ln:
        x = x + attention(ln1(x), weights, p + ".self_attn", H, kv)
        return x + ffn(ln2(x))
    x = ln1(x + attention(x, weights, p + ".self_attn", H, kv))
    return ln2(x + ffn(x))


def embed(cfg, weights, x, F):
    """(B, Fmax, 128) features -> (B, Ttok, D) tokens with their position rows, and the key counts."""
    kt, kc, D = cfg.ma_kt, cfg.ma_kc, cfg.encoder_embed_dim
    B, Fmax, _ = x.shape
    V, Tt = 128 // kc, Fmax // kt
    Ttok = Tt * V
    mean, var = float(_w(weights, "batch_norm.running_mean").reshape(-1)[0]), float(_w(weights, "batch_norm.running_var").reshape(-1)[0])
    x = (x - mean) / math.sqrt(var + cfg.ma_bn_eps) * 0.5
    # nn.Unfold, kernel = stride = (kt, kc): token t * V + v, content in (time, channel) row-major order
    patches = x[:, :Tt * kt].reshape(B, Tt, kt, V, kc).transpose(0, 1, 3, 2, 4).reshape(B, Ttok, kt * kc)
    tok = patches @ _w(weights, "post_extract_proj.weight").T + _w(weights, "post_extract_proj.bias")
    pe = _w(weights, "enc_sine_pos_embed.pe").reshape(-1, D)[:Ttok]
    kv = key_counts(F, kt, kc, Ttok)
    for b in range(B):
        tok[b, :kv[b]] += pe[:kv[b]]  # SinusoidalPositionalEncoding zeroes the rows of padded tokens
    return tok, kv


def forward(cfg, weights, wavs, feature_dtype=np.float64):
    """{"states": the encoder_layers layer outputs as (B, Tt, V * D), "kv": key counts, "frames": F_b, "tokens": (B, Ttok, D)}."""
    x, F = features(wavs, feature_dtype)
    tok, kv = embed(cfg, weights, x, F)
    B, Ttok, D = tok.shape
    V = 128 // cfg.ma_kc
    H, pre_ln = cfg.encoder_attention_heads, cfg.layer_norm_first
    states = [np.empty((B, Ttok // V, V * D)) for _ in range(cfg.encoder_layers)]
    for b in range(B):
        h = tok[b]
        if not pre_ln:
            h = layer_norm(h, _w(weights, "encoder.layer_norm.weight"), _w(weights, "encoder.layer_norm.bias"))
        for l in range(cfg.encoder_layers):
            h = encoder_layer(h, weights, f"encoder.layers.{l}", H, kv[b], pre_ln)
            states[l][b] = h.reshape(Ttok // V, V * D)
    return dict(states=states, kv=kv, frames=F, tokens=tok)
