"""Readers for the three converted-checkpoint formats the reference experts load:

* HuBERT   ``{"task_cfg", "model_cfg", "model_weight", "dictionaries_symbols"}``  (hubert/convert.py:37-56)
* wav2vec2 ``{"task_cfg", "model_cfg", "model_weight"}``                          (wav2vec2/convert.py:26-39)
* WavLM / UniSpeech-SAT ``{"cfg", "model"}``                      (wavlm/expert.py:37-40, unispeech_sat/expert.py:36-39)
* DistilHuBERT ``{"Config": {"distiller": {...}}, "Distiller": state_dict}``      (distiller/builder.py:41-58,119-122)
* multires-HuBERT: the HuBERT layout with ``MultiresHubertConfig`` in ``model_cfg``  (multires_hubert/convert.py:21-62)
* LightHuBERT ``{"cfg": {"model": {...}}, "model": supernet state_dict}``         (lighthubert/expert.py:17-47): cut to its subnet here
* DeCoAR 2.0 ``{"model": state_dict}``, no configuration: the widths come from the tensors' shapes  (decoar2/expert.py:20-26)

plus the fairseq layout ``{"cfg": {"task", "model"}, "model"}`` that ``hubert_custom(fairseq=True)`` /
``wav2vec2_custom(fairseq=True)`` convert first (hubert/convert.py:22-40, wav2vec2/convert.py:14-24).

Only the hot-path tensors are kept (``mask_emb``, ``label_embs_concat``, ``final_proj``, ``quantizer.*``,
``project_q`` … are unused at inference).  Also writes the same formats from synthetic weights.
"""

from __future__ import annotations

from typing import Dict, Tuple

import numpy as np

from .config import EncoderConfig, LIGHTHUBERT_SUPERNET, config_from_decoar2, config_from_lighthubert, byol_a_config, byol_s_config, config_from_mae_ast, decoar_config, vggish_config, config_from_apc, config_from_npc, config_from_cpc, config_from_mockingjay, config_from_dicts, config_from_distiller, config_from_multires, config_from_wav2vec
from .synth import lighthubert_supernet_config, param_shapes

_REQUIRED = {
    "hubert": ["task_cfg", "model_cfg", "model_weight", "dictionaries_symbols"],
    "wav2vec2": ["task_cfg", "model_cfg", "model_weight"],
    "wavlm": ["cfg", "model"],
    "distiller": ["Config", "Distiller"],
    "multires_hubert": ["task_cfg", "model_cfg", "model_weight", "dictionaries_symbols"],
    "wav2vec": ["task_cfg", "model_cfg", "model_weight"],  # wav2vec/convert.py:24-37
}


def _plain(d):
    """dataclass / namespace / omegaconf-ish → plain dict."""
    if isinstance(d, dict):
        return d
    import dataclasses

    if dataclasses.is_dataclass(d):
        return dataclasses.asdict(d)
    return dict(vars(d))


def load_cpc_checkpoint(ckpt: str) -> Tuple[EncoderConfig, Dict[str, np.ndarray]]:
    """``{"config": dict, "weights": state_dict}`` (upstream/cpc/expert.py:29-36): the checkpoint's ``config`` overrides the defaults
    of ``cpc_default_config.py``.  The reference loads the weights with ``strict=False`` — a missing tensor silently keeps its random
    initialisation, which nobody can reproduce — so every tensor the forward reads is required here."""
    import torch

    state = torch.load(ckpt, map_location="cpu", weights_only=False)
    for key in ("config", "weights"):
        if key not in state:
            raise ValueError(f"{ckpt} is not a valid checkpoint since the required key: {key} is missing")
    config = state["config"]
    cfg = config_from_cpc(config if isinstance(config, dict) else _plain(config))
    return cfg, _hot_path_weights(ckpt, cfg, state["weights"])


def load_apc_checkpoint(ckpt: str) -> Tuple[EncoderConfig, Dict[str, np.ndarray]]:
    """``{"config": {"data": {"audio": ...}, "model": {"paras": ...}}, "model": state_dict}`` (upstream/apc/expert.py:22-27).
    Every GRU tensor is required; ``postnet.*`` and VQ-APC's ``vq_layers.*`` feed only the prediction the upstream discards and are
    left in the file."""
    import torch

    state = torch.load(ckpt, map_location="cpu", weights_only=False)
    for key in ("config", "model"):
        if key not in state:
            raise ValueError(f"{ckpt} is not a valid checkpoint since the required key: {key} is missing")
    cfg = config_from_apc(state["config"])
    return cfg, _hot_path_weights(ckpt, cfg, state["model"])


def load_npc_checkpoint(ckpt: str) -> Tuple[EncoderConfig, Dict[str, np.ndarray]]:
    """``{"config": {"data": {"audio": ...}, "model": {"paras": ...}}, "model": state_dict}`` (upstream/npc/expert.py:22-26).  Every
    convolution and BatchNorm tensor is required; ``postnet.*`` and ``vq_layers.*`` feed only the prediction the upstream discards
    and are left in the file.  ``masked_convs.N.conv_mask`` is a registered buffer, not a parameter: a file that carries it must
    carry the mask this configuration computes (a wrong one is refused by name; the HIP path never reads masked taps, so a mask it
    did not apply would be a silent difference); ``bnN.num_batches_tracked`` is training state."""
    import torch

    state = torch.load(ckpt, map_location="cpu", weights_only=False)
    for key in ("config", "model"):
        if key not in state:
            raise ValueError(f"{ckpt} is not a valid checkpoint since the required key: {key} is missing")
    cfg = config_from_npc(state["config"])
    sd = state["model"]
    weights = _hot_path_weights(ckpt, cfg, sd)
    H, k = cfg.conv_dim, cfg.npc_kernel_size
    for i in range(cfg.npc_blocks):
        name = f"masked_convs.{i}.conv_mask"
        if not cfg.npc_has_mask(i) or name not in sd:
            continue
        m = sd[name]
        m = m.detach().cpu().float().numpy() if hasattr(m, "detach") else np.asarray(m, dtype=np.float32)
        head = (k - cfg.npc_mask(i)) // 2
        want = np.ones((H, H, k), dtype=np.float32)
        want[:, :, head:head + cfg.npc_mask(i)] = 0
        if m.shape != want.shape or not np.array_equal(m, want):
            raise ValueError(f"{ckpt}: {name} is not the mask of kernel_size {k} / mask_size {cfg.npc_mask_size} (block {i}: taps "
                             f"[{head}, {head + cfg.npc_mask(i)}) zeroed)")
    return cfg, weights


def vggish_geometry(cfg: EncoderConfig) -> Dict:
    """What a VGGish state dict does not show: the front end and the quantiser's range (``vggish_params.py`` in the reference)."""
    return dict(example_frames=cfg.vg_example_frames, num_mel_bins=cfg.vg_num_mel_bins, window=cfg.conv_layers[0][1],
                shift=cfg.conv_layers[0][2], mel_min_hz=cfg.vg_mel_min_hz, mel_max_hz=cfg.vg_mel_max_hz,
                log_offset=cfg.vg_log_offset, quant_min=cfg.vg_quant_min, quant_max=cfg.vg_quant_max)


def load_vggish_checkpoint(ckpt, postprocess: bool = True) -> Tuple[EncoderConfig, Dict[str, np.ndarray]]:
    """``{"vggish": state_dict, "pca": {"pca_eigen_vectors", "pca_means"}}`` (upstream/vggish/hubconf.py:22-31, vggish.py:136-156) —
    a dict, as the reference's expert takes it, or the path of a file holding one.  The files carry no configuration: the layer
    list is read off the tensors themselves (``features.K.weight`` in ``nn.Sequential`` order, a gap of 3 between two conv indices
    is a pool; a pool behind the last conv is taken when the flattened width of ``embeddings.0.weight`` asks for it), the front
    end is ``vggish_params.py``'s unless the dict carries this package's ``config`` entry (``vggish_geometry``).  ``pca_means`` may be ``(D,)`` or ``(D, 1)``; without ``postprocess`` the ``pca`` entry is not
    read."""
    if not isinstance(ckpt, dict):
        import torch

        ckpt = torch.load(ckpt, map_location="cpu", weights_only=False)
    if "vggish" not in ckpt:
        raise ValueError("a VGGish checkpoint is a dict with the key 'vggish' (and 'pca' with postprocess): 'vggish' is missing")
    sd = ckpt["vggish"]
    idx = sorted(int(k.split(".")[1]) for k in sd if k.startswith("features.") and k.endswith(".weight"))
    if not idx or idx[0] != 0:
        raise ValueError("VGGish checkpoint: no features.0.weight")
    layers = []
    for j, k in enumerate(idx):
        gap = (idx[j + 1] - k) if j + 1 < len(idx) else 2
        if gap not in (2, 3):
            raise ValueError(f"VGGish checkpoint: features.{k} is followed by features.{k + gap}: not a conv + ReLU (+ pool) stack")
        layers.append((int(sd[f"features.{k}.weight"].shape[0]), gap == 3))
    for name in ("embeddings.0.weight", "embeddings.2.weight", "embeddings.4.weight"):
        if name not in sd:
            raise ValueError(f"VGGish checkpoint: missing parameter {name}")
    fc = tuple(int(sd[f"embeddings.{i}.weight"].shape[0]) for i in (0, 2, 4))
    flat, (ch, _) = int(sd["embeddings.0.weight"].shape[1]), layers[-1]
    geometry = dict(ckpt.get("config") or {})
    frames, bands = int(geometry.get("example_frames", 96)), int(geometry.get("num_mel_bins", 64))
    pools = sum(p for _, p in layers)
    if flat * (4 ** (pools + 1)) == frames * bands * ch:
        layers[-1] = (ch, True)
    cfg = vggish_config(layers=layers, fc=fc, postprocess=postprocess, **geometry)
    what = "the VGGish checkpoint"
    merged = dict(sd)
    if postprocess:
        if "pca" not in ckpt:
            raise ValueError("a VGGish checkpoint needs the key 'pca' with postprocess=True")
        for name in ("pca_eigen_vectors", "pca_means"):
            if name not in ckpt["pca"]:
                raise ValueError(f"{what}: missing parameter pca.{name}")
            merged[name] = ckpt["pca"][name]
        m = merged["pca_means"]
        m = m.detach().cpu().float().numpy() if hasattr(m, "detach") else np.asarray(m, dtype=np.float32)
        if m.shape not in ((fc[2],), (fc[2], 1)):
            raise ValueError(f"{what}: parameter pca_means has shape {tuple(m.shape)}, expected ({fc[2]},) or ({fc[2]}, 1)")
        merged["pca_means"] = m.reshape(fc[2])
    return cfg, _hot_path_weights(what, cfg, merged)


def byol_a_state_dict(state) -> Dict:
    """``NetworkCommonMixIn.load_weight`` (upstream/byol_a/byol_a.py:58-80): a plain state dict, or one under ``"state_dict"``;
    every key is cut at its first ``fc.`` / ``features.`` component (whatever prefix a training wrapper put in front of it), keys
    without one are dropped."""
    import re

    if "state_dict" in state:
        state = state["state_dict"]
    out = {}
    for k in state:
        m = re.search(r"(^fc\.|\.fc\.|^features\.|\.features\.)", k)
        if m is None:
            continue
        new_k = k[m.start():]
        out[new_k[1:] if new_k[0] == "." else new_k] = state[k]
    return out


def load_byol_a_checkpoint(ckpt, feature_d: int = None, window_secs: float = 1.0, stride_secs: float = 1.0
                           ) -> Tuple[EncoderConfig, Dict[str, np.ndarray]]:
    """An ``AudioNTT2020`` weight file (upstream/byol_a/hubconf.py:18-42) or the dict it holds.  The file carries no configuration:
    ``feature_d`` is read off ``fc.0.weight`` and, when the caller names one (the hub entries do), checked against it.  The
    BatchNorm2d layers bring ``running_mean`` / ``running_var`` (eps 1e-5, the module's default); ``num_batches_tracked`` is
    training state and is ignored.  The reference loads strictly: every tensor is required."""
    what = ckpt if isinstance(ckpt, str) else "the BYOL-A checkpoint"
    if not isinstance(ckpt, dict):
        import torch

        ckpt = torch.load(ckpt, map_location="cpu", weights_only=False)
    sd = byol_a_state_dict(ckpt)
    if "fc.0.weight" not in sd:
        raise ValueError(f"{what}: missing parameter fc.0.weight")
    d = int(sd["fc.0.weight"].shape[0])
    if feature_d is not None and int(feature_d) != d:
        raise ValueError(f"{what}: feature_d {int(feature_d)} was asked for, but fc.0.weight has {d} rows")
    cfg = byol_a_config(feature_d=d, window_secs=window_secs, stride_secs=stride_secs)
    return cfg, _hot_path_weights(what, cfg, sd)


# what an MAE-AST state dict holds and the forward never reads (mae_ast.py:202-281): the decoder, the reconstruction / classification
# heads, the mask embeddings, the LayerNorm(feature_dim) and the decoder's position table; num_batches_tracked is training state
MAE_AST_UNUSED = ("decoder.", "final_proj_", "encoder_mask_emb", "decoder_mask_emb", "layer_norm.", "dec_sine_pos_embed.pe",
                  "batch_norm.num_batches_tracked")


def mae_ast_hot_path(what: str, cfg: EncoderConfig, sd) -> Dict[str, np.ndarray]:
    """The tensors an MAE-AST handle reads, out of a strict state dict (or of an already cut one): every hot-path parameter is
    required, ``enc_sine_pos_embed.pe`` — ``(1, max_token_length, D)`` in the file — is cut to its leading ``cfg.ma_pos_rows`` rows
    (the file's table is the operand: it is not recomputed), the keys of ``MAE_AST_UNUSED`` are ignored and any other key fails."""
    shapes = param_shapes(cfg)
    for k in sd:
        if k not in shapes and not k.startswith(MAE_AST_UNUSED):
            raise ValueError(f"{what}: unexpected parameter {k} (not a tensor of MAE_AST with this configuration)")
    sd = dict(sd)
    if "enc_sine_pos_embed.pe" in sd:
        pe = sd["enc_sine_pos_embed.pe"]
        pe = pe.detach().cpu().float().numpy() if hasattr(pe, "detach") else np.asarray(pe, dtype=np.float32)
        D = cfg.encoder_embed_dim
        if pe.ndim == 3:
            if pe.shape != (1, cfg.ma_max_token_length, D):
                raise ValueError(f"{what}: parameter enc_sine_pos_embed.pe has shape {tuple(pe.shape)}, expected "
                                 f"{(1, cfg.ma_max_token_length, D)}")
            pe = pe[0, :cfg.ma_pos_rows]
        sd["enc_sine_pos_embed.pe"] = np.ascontiguousarray(pe)
    return _hot_path_weights(what, cfg, sd)


def load_mae_ast_checkpoint(ckpt) -> Tuple[EncoderConfig, Dict[str, np.ndarray]]:
    """``{"cfg": {"model": MAE_AST_Config, "task": {feature_dim, sample_rate, ...}}, "model": state_dict}`` (mae_ast/expert.py:28-45)
    — the path of a file holding one, or the dict.  The reference loads with ``strict=True``; here every tensor the forward reads is
    required, the ones it never reads are ignored by name (``MAE_AST_UNUSED``) and anything else fails."""
    what = ckpt if isinstance(ckpt, str) else "the MAE-AST checkpoint"
    if not isinstance(ckpt, dict):
        import torch

        ckpt = torch.load(ckpt, map_location="cpu", weights_only=False)
    if "cfg" not in ckpt or "model" not in ckpt:
        raise ValueError(f"{what} is not a valid checkpoint since the required key: {'cfg' if 'cfg' not in ckpt else 'model'} is missing")
    c = _plain(ckpt["cfg"])
    for key in ("model", "task"):
        if key not in c:
            raise ValueError(f"{what}: cfg has no {key!r} block")
    cfg = config_from_mae_ast(_plain(c["model"]), _plain(c["task"]))
    return cfg, mae_ast_hot_path(what, cfg, ckpt["model"])


def mae_ast_cfg_blocks(cfg: EncoderConfig) -> Dict:
    """``checkpoint["cfg"]`` of a ``family="mae_ast"`` configuration: every field of ``MAE_AST_Config`` (the reference builds a
    ``SimpleNamespace`` from the dict, so a missing one is an AttributeError) and the task fields the model and the expert read."""
    model = dict(ast_kernel_size_chan=cfg.ma_kc, ast_kernel_size_time=cfg.ma_kt, ast_kernel_stride_chan=cfg.ma_stride_c,
                 ast_kernel_stride_time=cfg.ma_stride_t, encoder_layers=cfg.encoder_layers, encoder_embed_dim=cfg.encoder_embed_dim,
                 encoder_ffn_embed_dim=cfg.encoder_ffn_embed_dim, encoder_attention_heads=cfg.encoder_attention_heads,
                 activation_fn=cfg.ma_activation, layer_norm_first=cfg.layer_norm_first, feature_grad_mult=1.0,
                 use_post_enc_proj=False, decoder_embed_dim=cfg.encoder_embed_dim, decoder_layers=cfg.ma_decoder_layers,
                 decoder_layerdrop=0.0, dropout=0.1, attention_dropout=0.1, activation_dropout=0.0, encoder_layerdrop=0.0,
                 dropout_input=0.0, random_mask_prob=0.75, mask_length=10, mask_selection="static", mask_other=0,
                 no_mask_overlap=False, mask_min_space=0, conv_pos=128, conv_pos_groups=16, checkpoint_activations=False,
                 max_token_length=cfg.ma_max_token_length, enc_sine_pos=cfg.ma_enc_sine_pos, enc_conv_pos=cfg.ma_enc_conv_pos,
                 dec_sine_pos=cfg.ma_dec_sine_pos, dec_conv_pos=False)
    task = dict(feature_dim=cfg.ma_feature_dim, sample_rate=cfg.ma_sample_rate, feature_rate=100, feature_type="fbank",
                mask_type="random_mask" if cfg.ma_kc == 128 else "chunk_patch")
    return dict(model=model, task=task)


# what an SSAST file holds and the upstream never reads (ast_models.py:96-208, 381-398): v.norm reaches no returned state, the heads and
# the pretext layers are training state
SSAST_UNUSED = ("module.v.norm.", "module.v.head.", "module.v.head_dist.", "module.cpredlayer.", "module.gpredlayer.", "module.mask_embed")


def ssast_bilinear(x: np.ndarray, Ho: int, Wo: int) -> np.ndarray:
    """``F.interpolate(x, size=(Ho, Wo), mode="bilinear")`` (align_corners=False) of a (C, H, W) array, in float64: source coordinate
    (i + 0.5) * in / out - 0.5 clamped at 0, the two neighbours with the upper one clamped to the last index."""
    x = np.asarray(x, np.float64)
    _, H, W = x.shape

    def axis(n_in, n_out):
        src = np.maximum((np.arange(n_out) + 0.5) * (n_in / n_out) - 0.5, 0.0)
        i0 = np.minimum(np.floor(src).astype(np.int64), n_in - 1)
        i1 = np.minimum(i0 + 1, n_in - 1)
        return i0, i1, src - i0

    h0, h1, lh = axis(H, Ho)
    w0, w1, lw = axis(W, Wo)
    top = x[:, h0][:, :, w0] * (1.0 - lw) + x[:, h0][:, :, w1] * lw
    bot = x[:, h1][:, :, w0] * (1.0 - lw) + x[:, h1][:, :, w1] * lw
    return top * (1.0 - lh)[None, :, None] + bot * lh[None, :, None]


def ssast_position_rows(pos_patch: np.ndarray, p_f_dim: int, p_t_dim: int, f_dim: int, t_dim: int) -> np.ndarray:
    """The patch tokens' position rows for an (f_dim, t_dim) grid out of the pretraining table (p_f_dim * p_t_dim, D), by the
    reference's rule (ast_models.py:303-342): time — a centre cut when t_dim < p_t_dim, else a bilinear interpolation to (8, t_dim);
    frequency — a bilinear interpolation to (f_dim, t_dim).  The reference's other frequency branch (f_dim < p_f_dim) slices with
    ``+ t_dim`` and is refused.  Returns (f_dim * t_dim, D) float64 in the reference's f-major token order."""
    pos_patch = np.asarray(pos_patch, np.float64)
    P, D = pos_patch.shape
    if P != p_f_dim * p_t_dim:
        raise ValueError(f"ssast position table has {P} patch rows, the pretraining grid is {p_f_dim} x {p_t_dim}")
    if f_dim < p_f_dim:
        raise ValueError(f"ssast f_dim {f_dim} < p_f_dim {p_f_dim}: the reference's frequency cut of the position rows slices with "
                         "t_dim (ast_models.py:325-334) and is reached by neither released model; it is not built")
    g = pos_patch.T.reshape(D, p_f_dim, p_t_dim)
    if t_dim < p_t_dim:
        lo = int(p_t_dim / 2) - int(t_dim / 2)
        g = g[:, :, lo:lo + t_dim]
    else:
        g = ssast_bilinear(g, 8, t_dim)
    g = ssast_bilinear(g, f_dim, t_dim)
    return g.reshape(D, f_dim * t_dim).T


def ssast_hot_path(what: str, cfg: EncoderConfig, sd) -> Dict[str, np.ndarray]:
    """The tensors an SSAST handle reads (include/s3enc.h: s3enc_ssast_config), out of the released ``module.v.*`` state dict — or an
    already prepared set, which passes through.  ``patch.weight``: the conv weight summed over its input channel (ast_models.py:297-299)
    and permuted to [n][t][f]; ``prefix``: cls_token + pos_embed[0], dist_token + pos_embed[1]; ``pos``: the patch tokens' rows by
    ``ssast_position_rows``, permuted to the handle's time-major token order (row ti * f_dim + fi); the blocks as stored.  The keys
    of ``SSAST_UNUSED`` are ignored, any other unknown key fails."""
    if "patch.weight" in sd:
        return {k: (v.detach().cpu().float().numpy() if hasattr(v, "detach") else np.asarray(v, np.float32)) for k, v in sd.items()}
    arr = lambda w: w.detach().cpu().double().numpy() if hasattr(w, "detach") else np.asarray(w, dtype=np.float64)
    D, F = cfg.encoder_embed_dim, cfg.encoder_ffn_embed_dim
    need = {"module.v.cls_token": (1, 1, D), "module.v.dist_token": (1, 1, D), "module.v.patch_embed.proj.bias": (D,)}
    for l in range(cfg.encoder_layers):
        for name, shape in (("norm1", (D,)), ("attn.qkv", (3 * D, D)), ("attn.proj", (D, D)), ("norm2", (D,)), ("mlp.fc1", (F, D)),
                            ("mlp.fc2", (D, F))):
            need[f"module.v.blocks.{l}.{name}.weight"], need[f"module.v.blocks.{l}.{name}.bias"] = shape, shape[:1]
    free = ("module.v.pos_embed", "module.v.patch_embed.proj.weight", "module.p_input_fdim", "module.p_input_tdim")
    for k in sd:
        if k not in need and k not in free and not k.startswith(SSAST_UNUSED):
            raise ValueError(f"{what}: unexpected parameter {k} (not a tensor of an SSAST model with this configuration)")
    for k in list(need) + list(free):
        if k not in sd:
            raise ValueError(f"{what}: missing parameter {k}")
    for k, shape in need.items():
        if tuple(np.shape(sd[k])) != tuple(shape):
            raise ValueError(f"{what}: parameter {k} has shape {tuple(np.shape(sd[k]))}, expected {tuple(shape)}")
    p_fdim, p_tdim = int(arr(sd["module.p_input_fdim"]).reshape(-1)[0]), int(arr(sd["module.p_input_tdim"]).reshape(-1)[0])
    if (p_fdim, p_tdim) != (cfg.ss_p_input_fdim, cfg.ss_p_input_tdim):
        raise ValueError(f"{what}: pretraining input size {(p_fdim, p_tdim)}, the configuration says "
                         f"{(cfg.ss_p_input_fdim, cfg.ss_p_input_tdim)}")
    cw = arr(sd["module.v.patch_embed.proj.weight"])
    if cw.ndim != 4 or cw.shape[0] != D or cw.shape[2:] != (cfg.ss_fshape, cfg.ss_tshape):
        raise ValueError(f"{what}: parameter module.v.patch_embed.proj.weight has shape {tuple(cw.shape)}, expected "
                         f"{(D, 1, cfg.ss_fshape, cfg.ss_tshape)}")
    pf, pt = cfg.ss_pretrain_grid
    pe = arr(sd["module.v.pos_embed"])
    if pe.shape != (1, pf * pt + 2, D):
        raise ValueError(f"{what}: parameter module.v.pos_embed has shape {tuple(pe.shape)}, expected {(1, pf * pt + 2, D)}")
    f_dim, t_dim = cfg.ss_f_dim, cfg.ss_t_dim
    rows = ssast_position_rows(pe[0, 2:], pf, pt, f_dim, t_dim)  # f-major: row fi * t_dim + ti
    out = {
        "patch.weight": cw.sum(1).transpose(0, 2, 1).reshape(D, cfg.ss_tshape * cfg.ss_fshape),  # [n][f][t] -> [n][t][f]
        "patch.bias": arr(sd["module.v.patch_embed.proj.bias"]),
        "prefix": np.stack([arr(sd["module.v.cls_token"]).reshape(D) + pe[0, 0], arr(sd["module.v.dist_token"]).reshape(D) + pe[0, 1]]),
        "pos": rows.reshape(f_dim, t_dim, D).transpose(1, 0, 2).reshape(t_dim * f_dim, D),
    }
    for k in need:
        if k.startswith("module.v.blocks."):
            out[k[len("module.v."):]] = arr(sd[k])
    return {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in out.items()}


def load_ssast_checkpoint(ckpt, model_size: str = "base_p", window_secs: float = 1.0) -> Tuple[EncoderConfig, Dict[str, np.ndarray]]:
    """An SSAST pretraining file (ast_models.py:217-251: ``torch.load`` of a PLAIN state dict with ``module.`` keys) or the dict it
    holds.  The file carries no configuration beyond its shapes and the two ``p_input_*`` scalars: ``model_size`` is the reference's
    "<size>_<p|f>" and ``window_secs`` its constructor argument.  Returns the configuration and the RELEASED-layout tensors the
    forward needs (``ssast_hot_path`` prepares them for the handle)."""
    from .config import SSAST_SIZES, ssast_config

    what = ckpt if isinstance(ckpt, str) else "the SSAST checkpoint"
    if not isinstance(ckpt, dict):
        import torch

        ckpt = torch.load(ckpt, map_location="cpu", weights_only=False)
    size, _, mtype = str(model_size).partition("_")
    if size not in SSAST_SIZES or mtype not in ("p", "f"):
        raise ValueError(f"ssast model_size must be '<tiny|small|base>_<p|f>', got {model_size!r}")
    for k in ("module.v.pos_embed", "module.p_input_fdim", "module.p_input_tdim"):
        if k not in ckpt:
            raise ValueError(f"{what} is not a valid checkpoint since the required key: {k} is missing (the reference asks for a "
                             "model saved from a torch.nn.DataParallel object)")
    num = lambda w: int(w.reshape(-1)[0]) if hasattr(w, "reshape") else int(w)
    D = int(np.shape(ckpt["module.v.pos_embed"])[2])
    layers = 1 + max(int(k.split(".")[3]) for k in ckpt if k.startswith("module.v.blocks."))
    ffn = int(np.shape(ckpt["module.v.blocks.0.mlp.fc1.weight"])[0])
    if D != SSAST_SIZES[size][0]:
        raise ValueError(f"{what}: the file is {D} wide, model size {size!r} is {SSAST_SIZES[size][0]} wide")
    cfg = ssast_config(model_type=mtype, model_size=size, window_secs=window_secs, layers=layers, ffn=ffn,
                       p_input_fdim=num(ckpt["module.p_input_fdim"]), p_input_tdim=num(ckpt["module.p_input_tdim"]))
    keep = {k: v for k, v in ckpt.items() if not k.startswith(SSAST_UNUSED)}
    ssast_hot_path(what, cfg, keep)  # every check of the file happens at load time
    return cfg, {k: (v.detach().cpu().float().numpy() if hasattr(v, "detach") else np.asarray(v, np.float32)) for k, v in keep.items()}


def load_byol_s_checkpoint(ckpt, model_name: str = None, window_secs: float = 1, hop_secs: float = 0.05, blocks=None
                           ) -> Tuple[EncoderConfig, Dict[str, np.ndarray]]:
    """A BYOL-S weight file (upstream/byol_s/serab_byols/serab.py:74-103: ``model.load_state_dict(torch.load(path))``, a PLAIN
    state dict, loaded strictly) or the dict it holds.  The file carries no configuration.  ``model_name`` is the reference's:
    "default" (``features.*`` / ``fc.*``), "resnetish34" (``conv1`` / ``bn1`` / ``layerL.B.*``), "cvt" and "clstm" (refused by name);
    without one it is read off the keys.  The ResNet's block counts are read off the ``layerL.B`` keys (``blocks`` checks them);
    ``num_batches_tracked`` is training state and is ignored."""
    import re

    what = ckpt if isinstance(ckpt, str) else "the BYOL-S checkpoint"
    if not isinstance(ckpt, dict):
        import torch

        ckpt = torch.load(ckpt, map_location="cpu", weights_only=False)
    if model_name is None:
        model_name = "default" if "fc.0.weight" in ckpt else "resnetish"  # (any block counts)
    if model_name in ("cvt", "clstm"):
        raise ValueError(f"byol_s network {model_name} is not built (default and resnetish are)")
    if model_name == "default":
        cfg = byol_s_config("default", window_secs=window_secs, hop_secs=hop_secs)
        return cfg, _hot_path_weights(what, cfg, ckpt)
    if not model_name.startswith("resnetish"):
        raise ValueError(f"unknown byol_s model_name {model_name!r}")
    if any(re.match(r"layer\d+\.\d+\.(conv3|bn3)\.", k) for k in ckpt):
        raise ValueError(f"{what}: byol_s Bottleneck blocks (resnetish50) are not built: BasicBlock layers only")
    found = [1 + max([int(m.group(1)) for m in (re.match(rf"layer{L}\.(\d+)\.conv1\.weight$", k) for k in ckpt) if m], default=-1)
             for L in (1, 2, 3, 4)]
    if min(found) < 1:
        raise ValueError(f"{what}: missing parameter layer{1 + found.index(min(found))}.0.conv1.weight")
    want = {"resnetish34": (3, 4, 6, 3), "resnetish18": (2, 2, 2, 2), "resnetish10": (1, 1, 1, 1)}.get(model_name) if blocks is None else tuple(blocks)
    if want is not None and tuple(found) != tuple(want):
        raise ValueError(f"{what}: {model_name} has {tuple(want)} blocks, but the checkpoint's layers hold {tuple(found)}")
    cfg = byol_s_config("resnetish", blocks=found, window_secs=window_secs, hop_secs=hop_secs)
    return cfg, _hot_path_weights(what, cfg, ckpt)


def load_decoar_checkpoint(ckpt: str) -> Tuple[EncoderConfig, Dict[str, np.ndarray]]:
    """``{"model": state_dict}`` (upstream/decoar/expert.py:30-36; decoar_layers/expert.py:30-47 reads the same file and renames
    ``{forward,backward}_lstm.X_lN`` to its per-layer modules).  The file carries no configuration — the reference's ``Decoar()``
    hard-codes 80 / 1024 / 4 — so the widths and the depth are read off the tensors.  The reference loads with ``strict=False``: a
    missing tensor would silently keep its random initialisation, so every tensor the forward reads is required here."""
    import re

    import torch

    state = torch.load(ckpt, map_location="cpu", weights_only=False)
    if "model" not in state:
        raise ValueError(f"{ckpt} is not a valid checkpoint since the required key: model is missing")
    sd = state["model"]
    if "post_extract_proj.weight" not in sd:
        raise ValueError(f"{ckpt}: missing parameter post_extract_proj.weight")
    hidden, feat_dim = (int(v) for v in sd["post_extract_proj.weight"].shape)
    layers = {int(m.group(1)) for m in (re.fullmatch(r"forward_lstm\.weight_hh_l(\d+)", k) for k in sd) if m}
    if not layers or layers != set(range(len(layers))):
        raise ValueError(f"{ckpt}: missing parameter forward_lstm.weight_hh_l{min(set(range(len(layers) + 1)) - layers)}")
    cfg = decoar_config(hidden, len(layers), False, feat_dim)
    return cfg, _hot_path_weights(ckpt, cfg, sd)


def load_decoar2_checkpoint(ckpt: str) -> Tuple[EncoderConfig, Dict[str, np.ndarray]]:
    """``{"model": state_dict}`` (upstream/decoar2/expert.py:20-26).  The file carries no configuration — the reference's
    ``Decoar2()`` hard-codes 80 / 768 / 12 / 3072 — so the widths, the depth and the positional conv's kernel and groups are read off
    the tensors; heads are D / 64.  The reference loads with ``strict=False``: the tensors of the pre-training model that the encoder
    does not own are ignored here too, but a missing tensor that it does own would silently keep its random initialisation there, so
    every tensor the forward reads is required here, by name."""
    import torch

    state = torch.load(ckpt, map_location="cpu", weights_only=False)
    if "model" not in state:
        raise ValueError(f"{ckpt} is not a valid checkpoint since the required key: model is missing")
    sd = state["model"]
    try:
        cfg = config_from_decoar2(sd)
    except ValueError as err:
        raise ValueError(f"{ckpt}: {err}") from None
    return cfg, _hot_path_weights(ckpt, cfg, sd)


def mockingjay_state_dict(sd) -> Dict:
    """The legacy LayerNorm names of a ``Transformer`` state_dict, renamed as ``TransformerBuilder.load_model`` does
    (mockingjay/builder.py:136-150): ``gamma`` -> ``weight``, ``beta`` -> ``bias``."""
    out = {}
    for key, value in sd.items():
        if "gamma" in key:
            key = key.replace("gamma", "weight")
        if "beta" in key:
            key = key.replace("beta", "bias")
        out[key] = value
    return out


def load_mockingjay_checkpoint(ckpt: str) -> Tuple[EncoderConfig, Dict[str, np.ndarray]]:
    """``{"Transformer": state_dict, "Upstream_Config" (legacy: "Config"): {transformer, task, audio}, ...}``
    (mockingjay/builder.py:59-76).  ``SpecHead`` (the pre-training head) is left in the file; a config without an ``audio`` block
    is refused, as the reference's expert refuses it."""
    import sys
    import types

    import torch

    # old checkpoints pickle a scheduler of the reference's `optimizers` module (builder.py:53-56): a placeholder module lets the
    # unpickler resolve the name; the object is never used
    had = sys.modules.get("optimizers")
    if had is None:
        stub = types.ModuleType("optimizers")
        stub.__getattr__ = lambda name: type(name, (), {"__setstate__": lambda self, st: None})  # type: ignore[assignment]
        sys.modules["optimizers"] = stub
    try:
        state = torch.load(ckpt, map_location="cpu", weights_only=False)
    finally:
        if had is None:
            sys.modules.pop("optimizers", None)
    if "Transformer" not in state:
        raise ValueError(f"{ckpt} is not a valid checkpoint since the required key: Transformer is missing")
    if "transformer" in state.get("Config", {}):
        config = state["Config"]  # legacy: 'Config' is the upstream config
    elif "transformer" in state.get("Upstream_Config", {}):
        config = state["Upstream_Config"]
    else:
        raise NotImplementedError(f"{ckpt}: neither 'Config' nor 'Upstream_Config' holds a 'transformer' block")
    cfg = config_from_mockingjay(config)
    return cfg, _hot_path_weights(ckpt, cfg, mockingjay_state_dict(state["Transformer"]))


def mockingjay_upstream_config(cfg: EncoderConfig) -> Dict:
    """The ``Upstream_Config`` dict of a ``family="mockingjay"`` configuration, in the schema of pretrain/tera/config_model.yaml."""
    t = dict(input_dim=-1, hidden_size=cfg.encoder_embed_dim, num_hidden_layers=cfg.encoder_layers,
             num_attention_heads=cfg.encoder_attention_heads, intermediate_size=cfg.encoder_ffn_embed_dim,
             hidden_act=cfg.mj_hidden_act, hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1, initializer_range=0.02,
             layer_norm_eps=cfg.mj_layer_norm_eps, share_layer=cfg.mj_share_layer, pre_layer_norm=cfg.mj_pre_layer_norm)
    if cfg.mj_frontend == "kaldi":
        audio = dict(kaldi=dict(feat_type="fbank", fbank=dict(num_mel_bins=cfg.mj_kaldi_mel_bins, frame_length=cfg.mj_kaldi_frame_length,
                                                              frame_shift=cfg.mj_kaldi_frame_shift, use_log_fbank=True)),
                     delta=dict(order=cfg.mj_delta_order, win_length=cfg.mj_delta_win), cmvn=dict(use_cmvn=cfg.mj_cmvn))
    else:
        feat = dict(feat_type="mel", channel=0, log=True, delta=0, cmvn=cfg.mj_cmvn)
        audio = dict(target_level=cfg.mj_target_level, win_ms=25, hop_ms=10, n_freq=201, n_mels=cfg.mj_input_dim, n_mfcc=13,
                     input=dict(feat), target=dict(feat, channel=1))
    return dict(transformer=t, task=dict(sequence_length=cfg.mj_sequence_length), audio=audio)


def _split_rows(full: int, block: int, take: int, total: int) -> np.ndarray:
    """Indices an ``SLinear`` with splits keeps along its split axis (lighthubert/modules/scaling_linear.py:71-121): the axis of
    ``full`` entries is ``full // block`` equal blocks; a subnet of ``total`` entries takes the leading ``take`` of every block
    (the last block what is left of ``total``).  The whole axis when nothing is cut."""
    if total == full:
        return np.arange(full)
    idx, i = [], 0
    while len(idx) < total:
        n = min(take, total - i * take)
        idx.extend(range(i * block, i * block + n))
        i += 1
    assert i * block <= full
    return np.asarray(idx)


def lighthubert_slice(cfg: EncoderConfig, sd, what: str = "the LightHuBERT weights") -> Dict[str, np.ndarray]:
    """The supernet state dict cut to the subnet ``cfg`` describes — the tensors the handle reads, under HuBERT's names.

    ``SLayerNorm`` / ``SLinear`` / q, k, v, out_proj keep leading rows and columns; fc1 keeps the leading ``embed`` rows of each of its
    four 768-row blocks and fc2 the same columns (their ``out_splits`` / ``in_splits``); the positional ``SConv1d`` keeps
    ``weight[:embed, :embed // groups, :]`` with ``groups`` unchanged — new group g owns supernet filters [g dg, (g + 1) dg) and reads
    the first dg input columns of each — AFTER ``weight_norm`` has been resolved on the unsliced tensor (``weight_v`` (768, 48, K),
    ``weight_g`` (1, 1, K): the per-tap norm runs over all 768 x 48 entries), so the fold happens here, in float64, and the result
    travels as ``encoder.pos_conv.0.weight``.  ``mask_emb``, ``layer_pred_heads.*`` and label tensors are never read."""
    S = LIGHTHUBERT_SUPERNET
    E, F, C = cfg.encoder_embed_dim, cfg.encoder_ffn_embed_dim, cfg.conv_dim
    SE, SF = S["embed_dim"], S["ffn_embed"]

    def get(name, shape):
        if name not in sd:
            raise ValueError(f"{what}: missing parameter {name}")
        w = sd[name]
        w = w.detach().cpu().float().numpy() if hasattr(w, "detach") else np.asarray(w, dtype=np.float32)
        if tuple(w.shape) != tuple(shape):
            raise ValueError(f"{what}: parameter {name} has shape {tuple(w.shape)}, expected {tuple(shape)}")
        return w

    out: Dict[str, np.ndarray] = {}
    for name, shape in param_shapes(lighthubert_supernet_config(cfg)).items():  # the extractor is not cut
        if name.startswith(("feature_extractor.", "layer_norm.")):
            out[name] = get(name, shape)
    out["post_extract_proj.weight"] = get("post_extract_proj.weight", (SE, C))[:E]
    out["post_extract_proj.bias"] = get("post_extract_proj.bias", (SE,))[:E]
    K, G = cfg.conv_pos, cfg.conv_pos_groups
    v = get("encoder.pos_conv.0.weight_v", (SE, SE // G, K)).astype(np.float64)
    g = get("encoder.pos_conv.0.weight_g", (1, 1, K)).astype(np.float64)
    w = v * (g / np.sqrt((v * v).sum(axis=(0, 1), keepdims=True)))
    out["encoder.pos_conv.0.weight"] = w[:E, :E // G, :].astype(np.float32)
    out["encoder.pos_conv.0.bias"] = get("encoder.pos_conv.0.bias", (SE,))[:E]
    for leaf in ("weight", "bias"):
        out[f"encoder.layer_norm.{leaf}"] = get(f"encoder.layer_norm.{leaf}", (SE,))[:E]
    ffn = _split_rows(SF, SE, E, F)
    for l in range(cfg.encoder_layers):
        p = f"encoder.layers.{l}"
        for n in ("q_proj", "k_proj", "v_proj", "out_proj"):
            out[f"{p}.self_attn.{n}.weight"] = get(f"{p}.self_attn.{n}.weight", (SE, SE))[:E, :E]
            out[f"{p}.self_attn.{n}.bias"] = get(f"{p}.self_attn.{n}.bias", (SE,))[:E]
        for n in ("self_attn_layer_norm", "final_layer_norm"):
            for leaf in ("weight", "bias"):
                out[f"{p}.{n}.{leaf}"] = get(f"{p}.{n}.{leaf}", (SE,))[:E]
        out[f"{p}.fc1.weight"] = get(f"{p}.fc1.weight", (SF, SE))[ffn][:, :E]
        out[f"{p}.fc1.bias"] = get(f"{p}.fc1.bias", (SF,))[ffn]
        out[f"{p}.fc2.weight"] = get(f"{p}.fc2.weight", (SE, SF))[:E][:, ffn]
        out[f"{p}.fc2.bias"] = get(f"{p}.fc2.bias", (SE,))[:E]
    return {k: np.ascontiguousarray(a, dtype=np.float32) for k, a in out.items()}


def lighthubert_model_cfg(cfg: EncoderConfig) -> Dict:
    """``checkpoint["cfg"]["model"]`` for a LightHuBERT configuration, as the released files spell it."""
    d = dict(_name=cfg.lh_model, extractor_mode=cfg.extractor_mode, conv_bias=cfg.conv_bias, encoder_layers=12, encoder_embed_dim=768,
             encoder_ffn_embed_dim=3072, encoder_attention_heads=12, layer_norm_first=cfg.layer_norm_first, conv_pos=cfg.conv_pos,
             conv_pos_groups=cfg.conv_pos_groups, activation_fn="gelu", layer_type="transformer", pos_conv_depth=cfg.pos_conv_depth,
             conv_feature_layers=str([tuple(t) for t in cfg.conv_layers]))
    if cfg.lh_model == "hubert_pruner":
        d["pruner_supernet"] = f"lighthubert_{cfg.lh_supernet}.yaml"
    else:
        d["supernet_type"] = cfg.lh_supernet
    return d


def load_lighthubert_checkpoint(ckpt: str) -> Tuple[EncoderConfig, Dict[str, np.ndarray]]:
    """``{"cfg": {"model": {...}}, "model": state_dict}`` (upstream/lighthubert/expert.py:17-47): the subnet is resolved as the
    expert does and only the sliced tensors are returned (what reaches the device)."""
    import torch

    state = torch.load(ckpt, map_location="cpu", weights_only=False)
    for key in ("cfg", "model"):
        if key not in state:
            raise ValueError(f"{ckpt} is not a valid checkpoint since the required key: {key} is missing")
    model_cfg = _plain(_plain(state["cfg"])["model"])
    cfg = config_from_lighthubert(model_cfg)
    return cfg, lighthubert_slice(cfg, state["model"], ckpt)


def _hot_path_weights(ckpt: str, cfg: EncoderConfig, sd) -> Dict[str, np.ndarray]:
    weights = {}
    for name, shape in param_shapes(cfg).items():
        if name not in sd:
            raise ValueError(f"{ckpt}: missing parameter {name}")
        w = sd[name]
        w = w.detach().cpu().float().numpy() if hasattr(w, "detach") else np.asarray(w, dtype=np.float32)
        if tuple(w.shape) != tuple(shape):
            raise ValueError(f"{ckpt}: parameter {name} has shape {tuple(w.shape)}, expected {tuple(shape)}")
        weights[name] = np.ascontiguousarray(w)
    return weights


def load_checkpoint(ckpt: str, family: str) -> Tuple[EncoderConfig, Dict[str, np.ndarray]]:
    import torch

    if family == "cpc":
        return load_cpc_checkpoint(ckpt)
    if family == "apc":
        return load_apc_checkpoint(ckpt)
    if family == "mockingjay":
        return load_mockingjay_checkpoint(ckpt)
    if family == "decoar":
        return load_decoar_checkpoint(ckpt)
    if family == "npc":
        return load_npc_checkpoint(ckpt)
    if family == "vggish":
        return load_vggish_checkpoint(ckpt)
    if family == "byol_a":
        return load_byol_a_checkpoint(ckpt)
    if family == "byol_s":
        return load_byol_s_checkpoint(ckpt)
    if family == "mae_ast":
        return load_mae_ast_checkpoint(ckpt)
    if family == "lighthubert":
        return load_lighthubert_checkpoint(ckpt)
    if family == "decoar2":
        return load_decoar2_checkpoint(ckpt)
    if family == "ssast":
        return load_ssast_checkpoint(ckpt)

    state = torch.load(ckpt, map_location="cpu", weights_only=False)
    if family == "wav2vec" and "model_cfg" not in state and "model" in state and ("cfg" in state or "args" in state):
        # the original fairseq layout ({"cfg": {"task", "model"}, "model"}; before fairseq 0.10.2 {"args": Namespace, "model"}),
        # what wav2vec/convert.py:11-17 turns into the converted format
        cfg_ = state.get("cfg")
        if cfg_ is None:
            state = {"task_cfg": {}, "model_cfg": _plain(state["args"]), "model_weight": state["model"]}
        else:
            cfg_ = _plain(cfg_)
            state = {"task_cfg": _plain(cfg_.get("task") or {}), "model_cfg": _plain(cfg_["model"]), "model_weight": state["model"]}
    for key in _REQUIRED[family]:
        if key not in state:
            # same message shape as hubert/convert.py:46-49
            raise ValueError(f"{ckpt} is not a valid checkpoint since the required key: {key} is missing")
    if family == "wavlm":
        cfg = config_from_dicts("wavlm", _plain(state["cfg"]))
        sd = state["model"]
    elif family == "distiller":
        cfg = config_from_distiller(_plain(_plain(state["Config"])["distiller"]))
        sd = state["Distiller"]
    elif family == "multires_hubert":
        cfg = config_from_multires(_plain(state["model_cfg"]), _plain(state["task_cfg"]))
        sd = state["model_weight"]
    elif family == "wav2vec":  # (wav2vec_predictions.* / project_features.* are training-only: param_shapes does not name them)
        cfg = config_from_wav2vec(_plain(state["model_cfg"]), _plain(state["task_cfg"]))
        sd = state["model_weight"]
    else:
        cfg = config_from_dicts(family, _plain(state["model_cfg"]), _plain(state["task_cfg"]))
        sd = state["model_weight"]
    weights = {}
    for name, shape in param_shapes(cfg).items():
        if name not in sd:
            raise ValueError(f"{ckpt}: missing parameter {name}")
        w = sd[name]
        w = w.detach().cpu().float().numpy() if hasattr(w, "detach") else np.asarray(w, dtype=np.float32)
        if tuple(w.shape) != tuple(shape):
            raise ValueError(f"{ckpt}: parameter {name} has shape {tuple(w.shape)}, expected {tuple(shape)}")
        weights[name] = np.ascontiguousarray(w)
    return cfg, weights


def save_checkpoint(path: str, cfg: EncoderConfig, weights: Dict[str, np.ndarray]) -> None:
    """Write ``weights`` in the reference's converted format for ``cfg.family`` (what ``*_local(ckpt=...)`` reads)."""
    import torch

    sd = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in weights.items()}
    if cfg.family == "mockingjay":  # upstream/mockingjay/builder.py:59-76
        # new-style files keep the runner's config under "Config" and the reference's builder reads that key first
        torch.save({"Transformer": sd, "Upstream_Config": mockingjay_upstream_config(cfg), "Config": {"runner": {}}}, path)
        return
    if cfg.family in ("decoar", "decoar2"):  # upstream/decoar/expert.py:30-36, upstream/decoar2/expert.py:20-26
        torch.save({"model": sd}, path)
        return
    if cfg.family == "mae_ast":  # upstream/mae_ast/expert.py:28-38
        if "batch_norm.num_batches_tracked" in sd:
            sd["batch_norm.num_batches_tracked"] = sd["batch_norm.num_batches_tracked"].to(torch.int64).reshape(())
        torch.save({"cfg": mae_ast_cfg_blocks(cfg), "model": sd}, path)
        return
    if cfg.family == "ssast":  # upstream/ssast/ast_models.py:217-227: a plain state dict, the two input sizes as scalar tensors
        for k in ("module.p_input_fdim", "module.p_input_tdim"):
            if k in sd:
                sd[k] = sd[k].to(torch.int64).reshape(())
        torch.save(sd, path)
        return
    if cfg.family == "lighthubert":  # upstream/lighthubert/expert.py:17-21: the SUPERNET state dict beside cfg.model
        torch.save({"cfg": {"model": lighthubert_model_cfg(cfg)}, "model": sd}, path)
        return
    if cfg.family in ("byol_a", "byol_s"):  # upstream/byol_a/byol_a.py:58-80, byol_s/serab_byols/serab.py:100-102: a plain state dict
        torch.save(sd, path)
        return
    if cfg.family == "vggish":  # upstream/vggish/hubconf.py:22-31: the two state dicts in one file
        # "config" is this package's addition (the reference reads "vggish" and "pca" only): a shape other than the released one
        pca = {k: sd.pop(k) for k in ("pca_eigen_vectors", "pca_means") if k in sd}
        torch.save({"vggish": sd, "pca": pca, "config": vggish_geometry(cfg)}, path)
        return
    if cfg.family == "npc":  # upstream/npc/expert.py:22-26
        audio = dict(feat_type=cfg.apc_feat_type, feat_dim=cfg.apc_feat_dim, frame_length=cfg.apc_frame_length,
                     frame_shift=cfg.apc_frame_shift, decode_wav=False, cmvn=cfg.apc_cmvn)
        paras = dict(kernel_size=cfg.npc_kernel_size, mask_size=cfg.npc_mask_size, n_blocks=cfg.npc_blocks, hidden_size=cfg.conv_dim,
                     dropout=0.0, residual=cfg.npc_residual, batch_norm=cfg.npc_batch_norm, activate=cfg.npc_activate,
                     disable_cross_layer=cfg.npc_disable_cross_layer)
        if cfg.npc_vq is not None:
            paras["vq"] = dict(cfg.npc_vq)
        if cfg.npc_dim_bottleneck is not None:
            paras["dim_bottleneck"] = cfg.npc_dim_bottleneck
        torch.save({"config": {"data": {"audio": audio}, "model": {"paras": paras}}, "model": sd}, path)
        return
    if cfg.family == "apc":  # upstream/apc/expert.py:22-27
        audio = dict(feat_type=cfg.apc_feat_type, feat_dim=cfg.apc_feat_dim, frame_length=cfg.apc_frame_length,
                     frame_shift=cfg.apc_frame_shift, decode_wav=False, cmvn=cfg.apc_cmvn)
        paras = dict(hidden_size=cfg.conv_dim, num_layers=cfg.apc_layers, dropout=0.0, residual=cfg.apc_residual)
        if cfg.apc_vq is not None:
            paras["vq"] = dict(cfg.apc_vq)
        torch.save({"config": {"data": {"audio": audio}, "model": {"paras": paras}}, "model": sd}, path)
        return
    if cfg.family == "cpc":  # upstream/cpc/expert.py:29-36
        config = dict(hiddenEncoder=cfg.conv_dim, hiddenGar=cfg.ar_hidden, arMode=cfg.ar_mode, nLevelsGRU=cfg.ar_layers,
                      normMode=cfg.norm_mode, encoder_type="cpc", cpc_mode="reverse" if cfg.cpc_reverse else None,
                      samplingType="sequential" if cfg.cpc_keep_hidden else "samespeaker")
        torch.save({"config": config, "weights": sd}, path)
        return
    if cfg.family == "wav2vec":
        w2v = dict(conv_feature_layers=str([tuple(t) for t in cfg.conv_layers]),
                   conv_aggregator_layers=str([tuple(t) for t in cfg.agg_layers]), aggregator=cfg.aggregator,
                   activation=cfg.activation, log_compression=cfg.log_compression, skip_connections_feat=cfg.skip_connections_feat,
                   skip_connections_agg=cfg.skip_connections_agg, residual_scale=cfg.residual_scale,
                   non_affine_group_norm=cfg.non_affine_group_norm, no_conv_bias=cfg.no_conv_bias, agg_zero_pad=cfg.agg_zero_pad,
                   vq_type=cfg.vq_type, vq_vars=cfg.vq_vars, vq_groups=cfg.vq_groups, vq_dim=cfg.vq_dim, vq_depth=cfg.vq_depth,
                   combine_groups=cfg.combine_groups, infonce=False)
        torch.save({"task_cfg": {"normalize": False}, "model_cfg": w2v, "model_weight": sd}, path)
        return
    model_cfg = dict(
        extractor_mode=cfg.extractor_mode, conv_bias=cfg.conv_bias, encoder_layers=cfg.encoder_layers,
        encoder_embed_dim=cfg.encoder_embed_dim, encoder_ffn_embed_dim=cfg.encoder_ffn_embed_dim,
        encoder_attention_heads=cfg.encoder_attention_heads, layer_norm_first=cfg.layer_norm_first,
        conv_pos=cfg.conv_pos, conv_pos_groups=cfg.conv_pos_groups, activation_fn="gelu", pos_conv_depth=cfg.pos_conv_depth,
        conv_feature_layers=str([tuple(t) for t in cfg.conv_layers]),
    )
    if cfg.layer_type == "conformer":
        model_cfg.update(layer_type="conformer", pos_enc_type=cfg.pos_enc_type, attn_type=cfg.attn_type,
                         depthwise_conv_kernel_size=cfg.depthwise_conv_kernel_size)
    if cfg.family == "distiller":
        d = dict(extractor_mode=cfg.extractor_mode, extractor_conv_feature_layers=model_cfg["conv_feature_layers"],
                 conv_pos=cfg.conv_pos, conv_pos_groups=cfg.conv_pos_groups, encoder_layers=cfg.encoder_layers,
                 encoder_embed_dim=cfg.encoder_embed_dim, encoder_ffn_embed_dim=cfg.encoder_ffn_embed_dim,
                 encoder_attention_heads=cfg.encoder_attention_heads, layer_norm_first=cfg.layer_norm_first,
                 final_dim=cfg.encoder_embed_dim, n_tasks=cfg.pred_heads, task_emb_type="expand-last",
                 out_layer_type="expand-last")
        torch.save({"Config": {"distiller": d}, "Distiller": sd}, path)
    elif cfg.family == "multires_hubert":
        R = len(cfg.rate_pairs) + 1
        bl = cfg.block_layers
        model_cfg.update(label_rate_ratios=list(cfg.label_rate_ratios), encoder_layers=bl[0],
                         override_encoder_layers=str(bl[:R] + [bl[2 * R - 2 - i] for i in range(R - 1)]),
                         conv_adapator_kernal=cfg.conv_adapter_kernel, use_plain_updownsample=cfg.use_plain_updownsample)
        model_cfg.pop("pos_conv_depth")
        torch.save({"task_cfg": {"normalize": cfg.normalize, "label_rate": 50.0}, "model_cfg": model_cfg,
                    "model_weight": sd, "dictionaries_symbols": [["a"] * 8] * R}, path)
    elif cfg.family == "wavlm":
        model_cfg.update(normalize=cfg.normalize, relative_position_embedding=cfg.relative_position_embedding,
                         num_buckets=cfg.num_buckets, max_distance=cfg.max_distance, gru_rel_pos=cfg.gru_rel_pos)
        torch.save({"cfg": model_cfg, "model": sd}, path)
    elif cfg.family == "hubert":
        torch.save({"task_cfg": {"normalize": cfg.normalize, "label_rate": 50.0}, "model_cfg": model_cfg,
                    "model_weight": sd, "dictionaries_symbols": [["a"] * 8]}, path)
    else:
        torch.save({"task_cfg": {"normalize": cfg.normalize}, "model_cfg": model_cfg, "model_weight": sd}, path)


def convert_fairseq_checkpoint(path: str, family: str, refresh: bool = False) -> str:
    """``<stem>.converted.pt`` next to a fairseq checkpoint, in the reference's converted format — what
    ``load_and_convert_fairseq_ckpt`` writes (hubert/convert.py:22-40, wav2vec2/convert.py:14-24), without importing
    the ``fairseq`` package: the file is unpickled with torch and ``cfg`` may be a dict or an OmegaConf container
    (unpickling the latter needs ``omegaconf`` to be importable; if it is not, the error says so)."""
    import os

    import torch

    src = os.path.abspath(path)
    name = os.path.splitext(os.path.basename(src))[0] + ".converted.pt"
    out_dir = os.path.dirname(src)
    if not os.access(out_dir, os.W_OK):  # read-only checkpoint store: convert into a per-user cache instead
        import hashlib

        out_dir = os.path.join(os.environ.get("S3PRL_AMD_CACHE", os.path.join(os.path.expanduser("~"), ".cache", "s3prl_amd")),
                               hashlib.sha1(src.encode()).hexdigest()[:12])
        os.makedirs(out_dir, exist_ok=True)
    out = os.path.join(out_dir, name)

    def fresh():  # converted file present and not older than its source (refresh re-converts once, not once per rank)
        return os.path.isfile(out) and os.path.getmtime(out) >= os.path.getmtime(src)

    if fresh() and not refresh:
        return out
    # one converter at a time (every rank of a data-parallel job calls this at once): exclusive lock on a side file, then
    # re-check — the ranks that waited find the finished file (the reference serialises the same step with FileLock,
    # hubert/hubconf.py:46-56) — and the result appears atomically (temp file + os.replace), never half-written
    import fcntl
    import time

    t_call = time.time()
    with open(out + ".lock", "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        try:
            if fresh() and (not refresh or os.path.getmtime(out) >= t_call - 1.0):
                return out
            try:
                state = torch.load(src, map_location="cpu", weights_only=False)
            except ModuleNotFoundError as e:  # pragma: no cover - depends on the pickled classes
                raise RuntimeError(f"{path}: unpickling this fairseq checkpoint needs the module {e.name!r}; convert it "
                                   f"with s3prl's upstream/{family}/convert.py where fairseq is installed") from e
            if "cfg" not in state or "model" not in state:
                raise ValueError(f"{path} is not a fairseq checkpoint (needs 'cfg' and 'model')")
            cfg = state["cfg"]
            if not isinstance(cfg, dict):
                from omegaconf import OmegaConf  # only reachable when omegaconf unpickled the object above

                cfg = OmegaConf.to_container(cfg)
            conv = {"task_cfg": _plain(cfg["task"]), "model_cfg": _plain(cfg["model"]), "model_weight": state["model"]}
            if family == "hubert":
                dicts = (state.get("task_state") or {}).get("dictionaries") or []
                conv["dictionaries_symbols"] = [list(getattr(d, "symbols", d)) for d in dicts]
            tmp = f"{out}.tmp.{os.getpid()}"
            try:
                torch.save(conv, tmp)
                os.replace(tmp, out)
            finally:
                if os.path.exists(tmp):
                    os.remove(tmp)
        finally:
            fcntl.flock(lock, fcntl.LOCK_UN)
    return out
