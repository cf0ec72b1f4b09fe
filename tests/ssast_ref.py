"""float64 restatement of the SSAST upstream (s3prl/upstream/ssast/{expert,ast_models,audio}.py) in the project's own words: the
fixed windows, the per-window hanning kaldi log-mel with its affine normalisation and zero rows, the Conv2d patch embedding in the
reference's f-major token order behind cls and dist, the position rows cut or interpolated from the pretraining grid, timm 0.4.5's
pre-LN blocks (one fused attn.qkv, LayerNorm eps 1e-6, erf-GELU), the states and the expert's cut.  Written from the reference's
source, never from the HIP path.  Neither timm nor torchaudio is installed here, so no run of the reference's expert stands behind
it: tests/test_ssast_cpu.py pins its pieces against torch (nn.Conv2d, nn.TransformerEncoderLayer, F.interpolate) and the front end
against oracle/fbank_oracle.py with the window swapped.  ``weights`` is the released file's ``module.v.*`` layout."""

from __future__ import annotations

import math

import numpy as np

from oracle.fbank_oracle import EPS32, mel_banks

LN_EPS = 1e-6
NORM_ADD = float(np.float32(4.2677393))
NORM_DIV = float(np.float32(4.5689974 * 2))

_erf = np.vectorize(math.erf, otypes=[np.float64])


def _w(weights, name):
    w = weights[name]
    return w.detach().cpu().double().numpy() if hasattr(w, "detach") else np.asarray(w, np.float64)


# ---- windows (expert.py:85-107) -----------------------------------------------------------------------------------------------------
def windows(cfg, wavs):
    """(B, nseg, W) zero-padded windows starting at s * W, nseg = ceil(max_len / W)."""
    W = cfg.ss_window_samples
    nseg = -(-max(len(w) for w in wavs) // W)
    out = np.zeros((len(wavs), nseg * W))
    for b, w in enumerate(wavs):
        out[b, :len(w)] = np.asarray(w, np.float64)
    return out.reshape(len(wavs), nseg, W)


# ---- front end (audio.py:88-116) ----------------------------------------------------------------------------------------------------
def hanning(n):
    return 0.5 - 0.5 * np.cos(2.0 * math.pi * np.arange(n) / (n - 1))


def fbank_hanning(x):
    """kaldi.fbank(htk_compat=True, use_energy=False, window_type="hanning", num_mel_bins=128, dither=0, frame_shift=10): 25 ms
    frames, snip_edges, DC removal, pre-emphasis 0.97 with the first sample replicated, a 512-point DFT, log(max(e, FLT_EPSILON))."""
    x = np.asarray(x, np.float64)
    m = 0 if len(x) < 400 else 1 + (len(x) - 400) // 160
    if m == 0:
        return np.zeros((0, 128))
    fr = np.stack([x[160 * t:160 * t + 400] for t in range(m)])
    fr = fr - fr.mean(1, keepdims=True)
    fr = fr - 0.97 * np.concatenate([fr[:, :1], fr[:, :-1]], 1)
    spec = np.fft.rfft(fr * hanning(400), n=512, axis=1)
    return np.log(np.maximum((spec.real ** 2 + spec.imag ** 2) @ mel_banks(128, 512, 16000.0).T, EPS32))


def window_image(cfg, x):
    """One window's (target_length, 128) image: normalised log-mel rows, exact zeros behind them."""
    y = (fbank_hanning(x) + NORM_ADD) / NORM_DIV
    TL = cfg.ss_target_length
    img = np.zeros((TL, 128))
    img[:min(len(y), TL)] = y[:TL]
    return img


# ---- position rows (ast_models.py:303-351) ------------------------------------------------------------------------------------------
def bilinear(x, Ho, Wo):
    """F.interpolate(mode="bilinear", align_corners=False) of (C, H, W): per output pixel the source coordinate (i + 0.5) in / out
    - 0.5, clamped below at 0; the two nearest source pixels, the upper one clamped to the last."""
    C, H, W = x.shape
    out = np.empty((C, Ho, Wo))
    for i in range(Ho):
        si = max((i + 0.5) * H / Ho - 0.5, 0.0)
        i0 = min(int(math.floor(si)), H - 1)
        i1 = min(i0 + 1, H - 1)
        li = si - i0
        for j in range(Wo):
            sj = max((j + 0.5) * W / Wo - 0.5, 0.0)
            j0 = min(int(math.floor(sj)), W - 1)
            j1 = min(j0 + 1, W - 1)
            lj = sj - j0
            out[:, i, j] = (1 - li) * ((1 - lj) * x[:, i0, j0] + lj * x[:, i0, j1]) + li * ((1 - lj) * x[:, i1, j0] + lj * x[:, i1, j1])
    return out


def position_rows(cfg, weights):
    """(2 + f_dim * t_dim, D): the two prefix rows as stored, then the patch rows in the reference's f-major order."""
    pf, pt = cfg.ss_pretrain_grid
    f_dim, t_dim = cfg.ss_f_dim, cfg.ss_t_dim
    key = (id(weights["module.v.pos_embed"]), pf, pt, f_dim, t_dim)
    if key in _POS_CACHE:  # (the entry keeps the tensor alive, so its id stays its own)
        return _POS_CACHE[key][1]
    _POS_CACHE[key] = (weights["module.v.pos_embed"], _position_rows(_w(weights, "module.v.pos_embed")[0], pf, pt, f_dim, t_dim))
    return _POS_CACHE[key][1]


_POS_CACHE = {}


def _position_rows(pe, pf, pt, f_dim, t_dim):
    D = pe.shape[1]
    g = pe[2:].T.reshape(D, pf, pt)
    if t_dim < pt:
        lo = int(pt / 2) - int(t_dim / 2)
        g = g[:, :, lo:lo + t_dim]
    else:
        g = bilinear(g, 8, t_dim)
    if f_dim < pf:
        raise ValueError("f_dim < p_f_dim: the reference slices with t_dim here; unreachable for both experts and refused")
    g = bilinear(g, f_dim, t_dim)
    return np.concatenate([pe[:2], g.reshape(D, f_dim * t_dim).T])


# ---- embedding (ast_models.py:367-378) ----------------------------------------------------------------------------------------------
def patches(cfg, img):
    """(f_dim, t_dim, fshape, tshape): the Conv2d's receptive fields on the (128, target_length) transpose of the image."""
    fs, ts, fst, tst = cfg.ss_fshape, cfg.ss_tshape, cfg.ss_fstride, cfg.ss_tstride
    x = img.T
    return np.stack([np.stack([x[fi * fst:fi * fst + fs, ti * tst:ti * tst + ts] for ti in range(cfg.ss_t_dim)]) for fi in range(cfg.ss_f_dim)])


def embed(cfg, weights, img, time_major=False):
    """(2 + f_dim * t_dim, D) tokens of one window: cls, dist, then the patch tokens f-major (the reference's flatten(2) of the conv
    output); ``time_major`` = the handle's order, token 2 + ti * f_dim + fi, with the position rows permuted alike."""
    Wc = _w(weights, "module.v.patch_embed.proj.weight").sum(1)
    D = Wc.shape[0]
    p = patches(cfg, img)
    tok = np.einsum("ftab,nab->ftn", p, Wc) + _w(weights, "module.v.patch_embed.proj.bias")
    pos = position_rows(cfg, weights)
    tok = tok + pos[2:].reshape(cfg.ss_f_dim, cfg.ss_t_dim, D)
    if time_major:
        tok = tok.transpose(1, 0, 2)
    pre = np.stack([_w(weights, "module.v.cls_token").reshape(D), _w(weights, "module.v.dist_token").reshape(D)]) + pos[:2]
    return np.concatenate([pre, tok.reshape(-1, D)])


# ---- blocks (timm 0.4.5 vision_transformer.Block) -----------------------------------------------------------------------------------
def layer_norm(x, g, b, eps=LN_EPS):
    mu = x.mean(-1, keepdims=True)
    var = ((x - mu) ** 2).mean(-1, keepdims=True)
    return (x - mu) / np.sqrt(var + eps) * g + b


def gelu(x):
    return 0.5 * x * (1.0 + _erf(x / math.sqrt(2.0)))


def block(x, weights, p, H, eps=LN_EPS):
    """x + proj(attn(norm1(x))), then + fc2(gelu(fc1(norm2(.)))); attn.qkv rows q | k | v, heads as head_dim-wide chunks, no mask."""
    T, D = x.shape
    hd = D // H
    y = layer_norm(x, _w(weights, p + ".norm1.weight"), _w(weights, p + ".norm1.bias"), eps)
    qkv = y @ _w(weights, p + ".attn.qkv.weight").T + _w(weights, p + ".attn.qkv.bias")
    q, k, v = qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:]
    ctx = np.empty((T, D))
    for h in range(H):
        s = (q[:, h * hd:(h + 1) * hd] @ k[:, h * hd:(h + 1) * hd].T) * hd ** -0.5
        s = np.exp(s - s.max(-1, keepdims=True))
        ctx[:, h * hd:(h + 1) * hd] = (s / s.sum(-1, keepdims=True)) @ v[:, h * hd:(h + 1) * hd]
    x = x + ctx @ _w(weights, p + ".attn.proj.weight").T + _w(weights, p + ".attn.proj.bias")
    y = layer_norm(x, _w(weights, p + ".norm2.weight"), _w(weights, p + ".norm2.bias"), eps)
    y = gelu(y @ _w(weights, p + ".mlp.fc1.weight").T + _w(weights, p + ".mlp.fc1.bias"))
    return x + y @ _w(weights, p + ".mlp.fc2.weight").T + _w(weights, p + ".mlp.fc2.bias")


# ---- states and cut (ast_models.py:385-393, expert.py:113-133) ----------------------------------------------------------------------
def num_steps(cfg, max_len):
    """T_out = min(nseg * t_dim, len(range(0, max_len, 160 * tstride)))."""
    return min(-(-max_len // cfg.ss_window_samples) * cfg.ss_t_dim, len(range(0, max_len, 160 * cfg.ss_tstride)))


def forward(cfg, weights, wavs, time_major=False, eps=None):
    """{"states": depth arrays (B, T_out, f_dim * D), "images": (B, nseg, target_length, 128), "tokens": (B, nseg, 2 + f t, D)}.
    ``time_major``: run the blocks on the handle's token order (the states must not move)."""
    eps = cfg.ss_ln_eps if eps is None else eps
    win = windows(cfg, wavs)
    B, nseg, _ = win.shape
    f_dim, t_dim, D, H = cfg.ss_f_dim, cfg.ss_t_dim, cfg.encoder_embed_dim, cfg.encoder_attention_heads
    T_out = num_steps(cfg, max(len(w) for w in wavs))
    imgs = np.stack([np.stack([window_image(cfg, win[b, s]) for s in range(nseg)]) for b in range(B)])
    toks = np.empty((B, nseg, 2 + f_dim * t_dim, D))
    states = [np.empty((B, nseg * t_dim, f_dim * D)) for _ in range(cfg.encoder_layers)]
    cache = {}
    for b in range(B):
        for s in range(nseg):
            key = imgs[b, s].tobytes()  # silent windows repeat: encode each distinct image once
            if key not in cache:
                x = x0 = embed(cfg, weights, imgs[b, s], time_major)
                outs = []
                for l in range(cfg.encoder_layers):
                    x = block(x, weights, f"module.v.blocks.{l}", H, eps)
                    p = x[2:].reshape((t_dim, f_dim, D) if time_major else (f_dim, t_dim, D))
                    outs.append((p if time_major else p.transpose(1, 0, 2)).reshape(t_dim, f_dim * D))
                cache[key] = (x0, outs)
            toks[b, s], outs = cache[key]
            for l, o in enumerate(outs):
                states[l][b, s * t_dim:(s + 1) * t_dim] = o
    return dict(states=[h[:, :T_out] for h in states], images=imgs, tokens=toks)
