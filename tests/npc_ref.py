"""float64 numpy restatement of NPC (upstream/npc/npc.py:21-248, audio.py:53-115, expert.py:18-53), written from the model's
definition: APC's kaldi log-mel front end (``apc_ref``: hamming window, CMVN over time, ``pad_sequence``) and a stack of stride-1
convolutions run over ALL ``T`` rows of the padded batch — no length masking anywhere, so the rows behind an utterance's own
frames are not zeros from the first block on.  The yardstick of the NPC tests on both sides: the reference-generated fixtures pin
the model part on the CPU (fed THIS front end's features, rounded to fp32); the GPU op, the family and the fuzz cases are compared
with it."""

import numpy as np

import apc_ref

features = apc_ref.features  # (cfg, wavs, dtype) -> (B, T, feat_dim), frame counts: NPC's front end is APC's


def conv1d(x, w, b, live=None):
    """nn.Conv1d(C, N, k, padding=(k - 1) / 2) on channel-last rows: x (B, T, C), w (N, C, k) -> (B, T, N).  ``live``: the taps
    that are multiplied (default: all) — a masked tap contributes nothing, whatever its weight."""
    B, T, C = x.shape
    k = w.shape[2]
    P = (k - 1) // 2
    xp = np.zeros((B, T + 2 * P, C), dtype=x.dtype)
    xp[:, P:P + T] = x
    y = np.zeros((B, T, w.shape[0]), dtype=x.dtype) + b
    for j in (range(k) if live is None else live):
        y += xp[:, j:j + T] @ w[:, :, j].T
    return y


def live_taps(k, mask):
    """MaskConvBlock (npc.py:36-41): taps [head, head + mask) are zeroed, head = (k - mask) // 2."""
    head = (k - mask) // 2
    return [j for j in range(k) if not head <= j < head + mask]


def batch_norm(y, g, b, mean, var, eps=1e-5):
    """nn.BatchNorm1d in eval mode: the running statistics."""
    return (y - mean) / np.sqrt(var + y.dtype.type(eps)) * g + b


def state_names(cfg):
    """The reference's hooks in the order they fire (expert.py:28-41); the None entries of masked_convs never do."""
    names = []
    for i in range(cfg.npc_blocks):
        names.append(f"self.model.blocks[{i}]")
        if cfg.npc_has_mask(i):
            names.append(f"self.model.masked_convs[{i}]")
    return names + ["self.model"]


def model(cfg, weights, feats, dtype=np.float64):
    """NPC.forward (npc.py:216-248) behind the front end, and what the expert's hooks keep of it.  Returns hidden_states (hook
    order), kinds ("block" | "masked" | "sum" per state) and the masked convolutions' pre-activations."""
    g = lambda n: np.asarray(weights[n], dtype=dtype)  # noqa: E731
    act = (lambda v: np.maximum(v, 0)) if cfg.npc_activate == "relu" else np.tanh
    x = np.asarray(feats, dtype=dtype)
    hs, kinds, pre, feat = [], [], [], None
    for i in range(cfg.npc_blocks):
        p = f"blocks.{i}."
        y = conv1d(x, g(p + "conv.weight"), g(p + "conv.bias"))
        if cfg.npc_batch_norm:
            y = batch_norm(y, *(g(p + "bn1." + n) for n in ("weight", "bias", "running_mean", "running_var")))
        y = conv1d(act(y), g(p + "linear.weight"), g(p + "linear.bias"))
        if cfg.npc_batch_norm:
            y = batch_norm(y, *(g(p + "bn2." + n) for n in ("weight", "bias", "running_mean", "running_var")))
        if cfg.npc_residual and i > 0:
            y = y + x
        x = act(y).astype(dtype)
        hs.append(x)
        kinds.append("block")
        if not cfg.npc_has_mask(i):
            continue
        p = f"masked_convs.{i}.conv."
        z = conv1d(x, g(p + "weight"), g(p + "bias"), live_taps(cfg.npc_kernel_size, cfg.npc_mask(i)))
        pre.append(z)
        m = np.tanh(z).astype(dtype)
        hs.append(m)
        kinds.append("masked")
        feat = m if feat is None else feat + m
    hs.append(feat)
    kinds.append("sum")
    return dict(hidden_states=hs, kinds=kinds, masked_pre=pre)


def forward(cfg, weights, wavs):
    feats, lens = features(cfg, wavs)
    out = model(cfg, weights, feats)
    out["features"], out["lengths"] = feats, lens
    return out


def forward_fp32(cfg, weights, wavs):
    """The same model with every operation in fp32, from the waveforms: the CPU proxy of a GPU evaluation's error."""
    feats, _ = features(cfg, wavs, dtype=np.float32)
    return model(cfg, weights, feats, dtype=np.float32)["hidden_states"]
