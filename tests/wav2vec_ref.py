"""Float64 restatement of the wav2vec / vq-wav2vec forward (upstream/wav2vec/wav2vec_model.py:59-286,565-700; the gumbel
quantizer in eval, wav2vec2_model.py:1722-1782; wav2vec/expert.py:15-62), numpy only.  Pinned to the reference's own outputs by
tests/test_wav2vec_cpu.py (the fixtures under tests/golden/wav2vec/); the GPU tests use it where no fixture exists."""

import numpy as np


def conv1d(x, w, stride, bias=None):
    """x (B, L, Cin) channel-last, w (Cout, Cin, k) -> (B, (L - k) // stride + 1, Cout)"""
    B, L, Cin = x.shape
    Cout, _, k = w.shape
    Lo = (L - k) // stride + 1
    idx = np.arange(Lo)[:, None] * stride + np.arange(k)[None, :]
    win = x[:, idx, :].reshape(B * Lo, k * Cin)  # rows (k, Cin)
    y = (win @ w.transpose(2, 1, 0).reshape(k * Cin, Cout)).reshape(B, Lo, Cout)
    return y if bias is None else y + bias


def group_norm1(x, gamma=None, beta=None, eps=1e-5):
    """Fp32GroupNorm(1, C): one mean / biased variance per utterance over all L x C values"""
    mu = x.mean(axis=(1, 2), keepdims=True)
    var = x.var(axis=(1, 2), keepdims=True)
    y = (x - mu) / np.sqrt(var + eps)
    if gamma is not None:
        y = y * gamma + beta
    return y


def gn1_apply(x, gamma=None, beta=None, res=None, scale=1.0, log=False):
    """the row pass of the HIP path: GroupNorm(1, C) -> ReLU -> [(y + res) * scale] -> [log(|y| + 1)]"""
    y = np.maximum(group_norm1(x, gamma, beta), 0.0)
    if res is not None:
        y = (y + res) * scale
    if log:
        y = np.log(np.abs(y) + 1.0)
    return y


def pad_left(x, n, zero):
    if n == 0:
        return x
    head = np.zeros_like(x[:, :1]) if zero else x[:, :1]
    return np.concatenate([np.repeat(head, n, axis=1), x], axis=1)


def top2_margin(scores):
    """per decision: (best - second best) of `scores` (..., V), largest = chosen; a single variable is no decision: inf"""
    if scores.shape[-1] < 2:
        return np.full(scores.shape[:-1], np.inf)
    s = np.sort(scores, axis=-1)
    return s[..., -1] - s[..., -2]


def forward(cfg, weights, wavs, dtype=np.float64, n_max=None):
    """Returns dict(hidden_states=[z, agg layer outputs...], codewords, codeids, margin): margin = the smallest relative top-2
    margin of the quantizer's decisions (gumbel: relative to the largest |logit|; k-means: relative to the distance)."""
    W = {k: np.asarray(v, dtype=dtype) for k, v in weights.items()}
    n_max = n_max or max(len(w) for w in wavs)
    x = np.zeros((len(wavs), n_max, 1), dtype=dtype)
    for b, w in enumerate(wavs):
        x[b, : len(w), 0] = w
    affine = not cfg.non_affine_group_norm
    for i, (_, k, s) in enumerate(cfg.conv_layers):
        p = f"feature_extractor.conv_layers.{i}"
        x = conv1d(x, W[f"{p}.0.weight"], s)
        x = np.maximum(group_norm1(x, W.get(f"{p}.2.weight") if affine else None, W.get(f"{p}.2.bias") if affine else None), 0.0)
    if cfg.log_compression:
        x = np.log(np.abs(x) + 1.0)
    out = dict(hidden_states=[x], codewords=None, codeids=None, margin=None)
    B, T, C = x.shape
    if cfg.vq_type != "none":
        G, V = cfg.vq_groups, cfg.vq_vars
        Dv = C // G
        if cfg.vq_type == "gumbel":
            h = x.reshape(B * T, C)
            for i in range(cfg.vq_depth - 1):
                h = np.maximum(h @ W[f"vector_quantizer.weight_proj.{i}.0.weight"].T + W[f"vector_quantizer.weight_proj.{i}.0.bias"], 0.0)
            last = f"vector_quantizer.weight_proj.{cfg.vq_depth - 1}" if cfg.vq_depth > 1 else "vector_quantizer.weight_proj"
            logits = (h @ W[last + ".weight"].T + W[last + ".bias"]).reshape(B, T, G, V)
            ids = logits.argmax(-1)
            out["margin"] = float((top2_margin(logits) / np.abs(logits).max()).min())
            table = W["vector_quantizer.vars"].reshape(-1, V, Dv)  # (Gt, V, Dv)
        else:
            wp = W["vector_quantizer.projection.0.weight"][:, :, 0]  # (C, Dv): Conv1d(C, C, 1, groups = G)
            ze = np.concatenate([x[..., g * Dv:(g + 1) * Dv] @ wp[g * Dv:(g + 1) * Dv].T for g in range(G)], axis=-1)
            zg = ze.reshape(B, T, G, Dv)
            mu = zg.mean(axis=(1, 3), keepdims=True)
            var = zg.var(axis=(1, 3), keepdims=True)
            zn = ((zg - mu) / np.sqrt(var + 1e-5)).reshape(B, T, C) * W["vector_quantizer.projection.1.weight"] + \
                W["vector_quantizer.projection.1.bias"]
            emb = W["vector_quantizer.embedding"]  # (V, Gt, Dv)
            if cfg.combine_groups:
                emb = np.repeat(emb, G, axis=1)
            d = np.sqrt(((zn.reshape(B, T, G, 1, Dv) - emb.transpose(1, 0, 2)[None, None]) ** 2).sum(-1))  # (B, T, G, V)
            ids = d.argmin(-1)
            out["margin"] = float((top2_margin(-d) / d.min(-1)).min())
            table = emb.transpose(1, 0, 2) if not cfg.combine_groups else W["vector_quantizer.embedding"].transpose(1, 0, 2)
        Gt = table.shape[0]
        cw = np.stack([table[g % Gt][ids[..., g]] for g in range(G)], axis=2).reshape(B, T, C)
        out["codewords"], out["codeids"] = cw, ids.astype(np.int64)
        x = cw
    scale = np.sqrt(cfg.residual_scale)
    for j, (_, k, _) in enumerate(cfg.agg_layers):
        p = f"feature_aggregator.conv_layers.{j}"
        y = conv1d(pad_left(x, k - 1, cfg.agg_zero_pad), W[f"{p}.1.weight"], 1, None if cfg.no_conv_bias else W[f"{p}.1.bias"])
        y = np.maximum(group_norm1(y, W.get(f"{p}.3.weight") if affine else None, W.get(f"{p}.3.bias") if affine else None), 0.0)
        x = (y + x) * scale if cfg.skip_connections_agg else y
        out["hidden_states"].append(x)
    return out
