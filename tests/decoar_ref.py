"""float64 numpy restatement of DeCoAR / DeCoAR-layers (upstream/decoar/{decoar,audio,expert}.py, upstream/decoar_layers/), written
from the model's definition and evaluated PER UTTERANCE: the kaldi log-mel front end (hamming window, no deltas, CMVN over time),
every ``decoar_subsample``-th frame, the projection, a forward and a backward stack of unidirectional LSTM layers on the
utterance's own frames — the backward stack with the flips written out as the reference does them (``flipBatch`` before the stack
and after it) — and the two outputs side by side.  The yardstick of the DeCoAR tests on both sides: the reference-generated
fixtures pin the model part on the CPU (the reference's own front end needs torchaudio, so the fixtures are fed THIS front end's
features, rounded to fp32); the GPU op, the family and the fuzz cases are compared with it."""

import numpy as np

import apc_ref
import cpc_ref

STACKS = ("forward_lstm", "backward_lstm")


def frontend(cfg, wav, dtype=np.float64):
    """FeatureExtractor.forward (decoar/audio.py:69-83) on one waveform, then every subsample-th frame: (frames, feat_dim)."""
    y = apc_ref.kaldi_fbank(wav, cfg.decoar_feat_dim, cfg.decoar_frame_length, cfg.decoar_frame_shift, "hamming", dtype=dtype)
    return apc_ref.cmvn(y)[::cfg.decoar_subsample] if y.shape[0] > 0 else y


def features(cfg, wavs, dtype=np.float64):
    """pad_sequence of the per-utterance features (decoar/expert.py:59-62): (B, T, feat_dim) and the frame counts."""
    feats = [frontend(cfg, w, dtype) for w in wavs]
    lens = [f.shape[0] for f in feats]
    out = np.zeros((len(feats), max(lens), cfg.decoar_feat_dim), dtype=dtype)
    for b, f in enumerate(feats):
        out[b, :f.shape[0]] = f
    return out, lens


def flip(x):
    """flipBatch (decoar/decoar.py:41-46) on one utterance's own rows"""
    return x[::-1].copy()


def lstm_stack(x, weights, stack, layers):
    """``layers`` nn.LSTM layers (batch_first, zero initial state) on one utterance (n, H): every layer's output and the gate
    pre-activations of its live rows."""
    outs, gates = [], []
    for l in range(layers):
        g = lambda n: np.asarray(weights[f"{stack}.{n}_l{l}"], dtype=np.float64)  # noqa: E731
        y, a = cpc_ref.rnn_layer(x[None], g("weight_ih"), g("weight_hh"), g("bias_ih"), g("bias_hh"), "LSTM")
        outs.append(y[0])
        gates.append(a.reshape(-1))
        x = y[0]
    return outs, gates


def model(cfg, weights, feats, lens):
    """Decoar.forward behind the front end (decoar/decoar.py:48-83; decoar_layers/decoar.py:50-97 for one state per layer): the
    states the expert returns, each (B, T, 2 H) with zeros behind every utterance's frames, and the standard deviation of the gate
    pre-activations per layer and direction."""
    feats = np.asarray(feats, dtype=np.float64)
    B, T, _ = feats.shape
    H, NL = cfg.decoar_hidden, cfg.decoar_layers
    wp, bp = (np.asarray(weights[f"post_extract_proj.{n}"], dtype=np.float64) for n in ("weight", "bias"))
    full = [np.zeros((B, T, 2 * H)) for _ in range(NL)]
    gates = [[[] for _ in range(2)] for _ in range(NL)]
    for b, n in enumerate(lens):
        x = feats[b, :n] @ wp.T + bp
        fwd, gf = lstm_stack(x, weights, STACKS[0], NL)
        bwd, gb = lstm_stack(flip(x), weights, STACKS[1], NL)
        for l in range(NL):
            full[l][b, :n, :H] = fwd[l]
            full[l][b, :n, H:] = flip(bwd[l])
            gates[l][0].append(gf[l])
            gates[l][1].append(gb[l])
    std = [float(np.concatenate(gates[l][d]).std()) for l in range(NL) for d in range(2)]
    return dict(hidden_states=full if cfg.decoar_per_layer else [full[-1]], gate_std=std)


def forward(cfg, weights, wavs):
    feats, lens = features(cfg, wavs)
    out = model(cfg, weights, feats, lens)
    out["features"], out["lengths"] = feats, lens
    return out


# ---- the same model with every operation rounded to fp32: the CPU proxy of a GPU evaluation's error (make_golden_decoar.py) -----
def forward_fp32(cfg, weights, wavs):
    f32 = np.float32
    feats, lens = features(cfg, wavs, dtype=f32)
    sig = lambda v: f32(1) / (f32(1) + np.exp(-v))  # noqa: E731
    B, T, _ = feats.shape
    H, NL = cfg.decoar_hidden, cfg.decoar_layers
    wp, bp = (np.asarray(weights[f"post_extract_proj.{n}"], dtype=f32) for n in ("weight", "bias"))
    full = [np.zeros((B, T, 2 * H), dtype=f32) for _ in range(NL)]
    for b, n in enumerate(lens):
        x0 = feats[b, :n] @ wp.T + bp
        for d, stack in enumerate(STACKS):
            x = flip(x0) if d else x0
            for l in range(NL):
                g = lambda k: np.asarray(weights[f"{stack}.{k}_l{l}"], dtype=f32)  # noqa: E731
                w_hh = g("weight_hh")
                pre = x @ g("weight_ih").T + (g("bias_ih") + g("bias_hh"))
                h, c, y = np.zeros(H, dtype=f32), np.zeros(H, dtype=f32), np.zeros((n, H), dtype=f32)
                for t in range(n):
                    a = pre[t] + w_hh @ h
                    c = (sig(a[H:2 * H]) * c + sig(a[:H]) * np.tanh(a[2 * H:3 * H])).astype(f32)
                    h = (sig(a[3 * H:]) * np.tanh(c)).astype(f32)
                    y[t] = h
                full[l][b, :n, d * H:(d + 1) * H] = flip(y) if d else y
                x = y
    return full if cfg.decoar_per_layer else [full[-1]]
