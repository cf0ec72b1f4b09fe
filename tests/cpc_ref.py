"""float64 numpy restatement of modified CPC (conv stack with symmetric zero padding, per-frame channel norm with the unbiased
variance, ReLU, multi-layer LSTM / GRU in torch's gate order), written from the model's definition: the yardstick of the CPC
tests on both sides (the reference-generated fixtures pin it on the CPU; the GPU ops and the fuzz cases are compared with it)."""

import numpy as np


def sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def conv1d(x, w, b, stride, pad):
    """x: (B, L, Cin) channel-last; w: (Cout, Cin, k); zero padding of ``pad`` frames on both sides -> (B, Lout, Cout)."""
    B, L, Cin = x.shape
    Cout, _, k = w.shape
    xp = np.zeros((B, L + 2 * pad, Cin))
    xp[:, pad:pad + L] = x
    Lout = (L + 2 * pad - k) // stride + 1
    idx = np.arange(Lout)[:, None] * stride + np.arange(k)[None, :]
    win = xp[:, idx, :].reshape(B * Lout, k * Cin)                     # [tap][channel]
    wm = np.transpose(w, (0, 2, 1)).reshape(Cout, k * Cin)
    return (win @ wm.T + b).reshape(B, Lout, Cout)


def channelnorm_relu(x, gamma=None, beta=None, eps=1e-5):
    """Per frame over the last axis: (x - mean) / sqrt(var + eps) * gamma + beta with the UNBIASED variance, then ReLU."""
    mean = x.mean(-1, keepdims=True)
    var = x.var(-1, keepdims=True, ddof=1)
    y = (x - mean) / np.sqrt(var + eps)
    if gamma is not None:
        y = y * gamma
    if beta is not None:
        y = y + beta
    return np.maximum(y, 0.0)


def lstm_from_pre(pre, w_hh):
    """pre: (B, T, 4H) = x W_ih^T + b_ih + b_hh, gates i, f, g, o; zero initial state -> (B, T, H)."""
    B, T, H4 = pre.shape
    H = H4 // 4
    h, c = np.zeros((B, H)), np.zeros((B, H))
    out = np.empty((B, T, H))
    for t in range(T):
        a = pre[:, t] + h @ w_hh.T
        i, f, g, o = sigmoid(a[:, :H]), sigmoid(a[:, H:2 * H]), np.tanh(a[:, 2 * H:3 * H]), sigmoid(a[:, 3 * H:])
        c = f * c + i * g
        h = o * np.tanh(c)
        out[:, t] = h
    return out


def gru_from_pre(pre, w_hh, b_hn):
    """pre: (B, T, 3H) = x W_ih^T + b_ih (+ b_hh for the r and z parts only), gates r, z, n; b_hn stays inside r * (W_hn h + b_hn)."""
    B, T, H3 = pre.shape
    H = H3 // 3
    h = np.zeros((B, H))
    out = np.empty((B, T, H))
    for t in range(T):
        a = h @ w_hh.T
        r = sigmoid(pre[:, t, :H] + a[:, :H])
        z = sigmoid(pre[:, t, H:2 * H] + a[:, H:2 * H])
        n = np.tanh(pre[:, t, 2 * H:] + r * (a[:, 2 * H:] + b_hn))
        h = (1.0 - z) * n + z * h
        out[:, t] = h
    return out


def rnn_pre(x, w_ih, b_ih, b_hh, cell):
    """The input projection with the biases that may be folded into it (LSTM: all of b_hh; GRU: its r and z parts)."""
    pre = x @ w_ih.T + b_ih
    H = w_ih.shape[0] // (4 if cell == "LSTM" else 3)
    fold = b_hh.copy()
    if cell == "GRU":
        fold[2 * H:] = 0.0
    return pre + fold


def rnn_layer(x, w_ih, w_hh, b_ih, b_hh, cell):
    """One layer of nn.LSTM / nn.GRU on (B, T, I); returns (output, the gate pre-activations of every step)."""
    pre = rnn_pre(x, w_ih, b_ih, b_hh, cell)
    H = w_hh.shape[1]
    out = lstm_from_pre(pre, w_hh) if cell == "LSTM" else gru_from_pre(pre, w_hh, b_hh[2 * H:])
    hprev = np.concatenate([np.zeros_like(out[:, :1]), out[:, :-1]], axis=1)
    gates = pre + hprev @ w_hh.T
    if cell == "GRU":  # the n gate's argument depends on r; its linear parts are what is reported
        gates[..., 2 * H:] += b_hh[2 * H:]
    return out, gates


def encoder(cfg, weights, wavs):
    """The conv stack on the zero-padded batch: (B, T, C)."""
    W = {k: np.asarray(v, dtype=np.float64) for k, v in weights.items() if k.startswith("gEncoder.")}
    n_max = max(len(w) for w in wavs)
    x = np.zeros((len(wavs), n_max, 1))
    for b, w in enumerate(wavs):
        x[b, :len(w), 0] = w
    for i, ((_, k, s), p) in enumerate(zip(cfg.conv_layers, cfg.conv_pads)):
        x = conv1d(x, W[f"gEncoder.conv{i}.weight"], W[f"gEncoder.conv{i}.bias"], s, p)
        x = channelnorm_relu(x, W[f"gEncoder.batchNorm{i}.weight"].reshape(-1), W[f"gEncoder.batchNorm{i}.bias"].reshape(-1))
    return x


def forward(cfg, weights, wavs):
    """hidden_states = [encoder output (B, T, C), recurrent output (B, T, H)]; gate_std: per recurrent layer the standard
    deviation of the gate pre-activations."""
    enc = encoder(cfg, weights, wavs)
    x, stds = enc, []
    for l in range(cfg.ar_layers):
        g = lambda n: np.asarray(weights[f"gAR.baseNet.{n}_l{l}"], dtype=np.float64)  # noqa: E731
        x, gates = rnn_layer(x, g("weight_ih"), g("weight_hh"), g("bias_ih"), g("bias_hh"), cfg.ar_mode)
        stds.append(float(gates.std()))
    return dict(hidden_states=[enc, x], gate_std=stds)
