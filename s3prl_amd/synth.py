"""Deterministic synthetic checkpoints and waveforms.

There is no network for real checkpoints, so benchmarks, tests and the golden
fixtures all use weights drawn from a seeded numpy generator, named exactly like the reference
``state_dict`` entries on the hot path, so that the very same tensors can be loaded
into the reference classes (``tests/golden/make_golden.py``) and into the HIP encoder.

The scales are chosen so activations stay O(1) through 12-24 layers and so that every bias /
affine parameter is exercised (none is left at its 0/1 default).
"""

from __future__ import annotations

from typing import Dict, List

import numpy as np

from .config import EncoderConfig


def param_shapes(cfg: EncoderConfig) -> Dict[str, tuple]:
    """Hot-path parameter names → shapes (reference naming)."""
    if cfg.family == "wav2vec":
        return _wav2vec_shapes(cfg)
    if cfg.family == "cpc":
        return _cpc_shapes(cfg)
    if cfg.family == "apc":
        return _apc_shapes(cfg)
    if cfg.family == "mockingjay":
        return _mockingjay_shapes(cfg)
    if cfg.family == "decoar":
        return _decoar_shapes(cfg)
    if cfg.family == "npc":
        return _npc_shapes(cfg)
    if cfg.family == "vggish":
        return _vggish_shapes(cfg)
    if cfg.family == "byol_a":
        return _byol_a_shapes(cfg)
    if cfg.family == "byol_s":
        return _byol_s_shapes(cfg)
    if cfg.family == "mae_ast":
        return _mae_ast_shapes(cfg)
    if cfg.family == "lighthubert":
        return _lighthubert_shapes(cfg)
    if cfg.family == "ssast":
        return _ssast_shapes(cfg)
    s: Dict[str, tuple] = {}
    cin = 1
    d2 = cfg.family == "decoar2"  # its "conv stack" is the kaldi front end's geometry: no weights, no feature LayerNorm
    for i, (dim, k, _) in enumerate([] if d2 else cfg.conv_layers):
        p = f"feature_extractor.conv_layers.{i}"
        s[f"{p}.0.weight"] = (dim, cin, k)
        if cfg.conv_bias:
            s[f"{p}.0.bias"] = (dim,)
        if cfg.extractor_mode == "layer_norm":
            s[f"{p}.2.1.weight"] = (dim,)
            s[f"{p}.2.1.bias"] = (dim,)
        elif i == 0:
            s[f"{p}.2.weight"] = (dim,)
            s[f"{p}.2.bias"] = (dim,)
        cin = dim
    C, D, F, H = cfg.conv_dim, cfg.encoder_embed_dim, cfg.encoder_ffn_embed_dim, cfg.encoder_attention_heads
    if cfg.feature_layer_norm and not d2:
        s["layer_norm.weight"] = (C,)
        s["layer_norm.bias"] = (C,)
    s["post_extract_proj.weight"] = (D, C)
    s["post_extract_proj.bias"] = (D,)
    if cfg.family == "multires_hubert":
        return _multires_shapes(cfg, s)
    if cfg.pos_conv_depth > 1:  # data2vec: plain convs, no weight_norm (wav2vec2_model.py:3001-3007)
        for i in range(cfg.pos_conv_depth):
            s[f"encoder.pos_conv.{i}.0.weight"] = (D, D // cfg.conv_pos_groups, cfg.pos_conv_kernel)
            s[f"encoder.pos_conv.{i}.0.bias"] = (D,)
    else:
        s["encoder.pos_conv.0.bias"] = (D,)
        s["encoder.pos_conv.0.weight_g"] = (1, 1, cfg.conv_pos)
        s["encoder.pos_conv.0.weight_v"] = (D, D // cfg.conv_pos_groups, cfg.conv_pos)
    s["encoder.layer_norm.weight"] = (D,)
    s["encoder.layer_norm.bias"] = (D,)
    if cfg.layer_type == "conformer":  # (the pos_conv above is in every checkpoint, ConformerEncoder never calls it)
        for l in range(cfg.encoder_layers):
            _conformer_shapes(s, f"encoder.layers.{l}", cfg)
        return s
    for l in range(cfg.encoder_layers):
        p = f"encoder.layers.{l}"
        _layer_shapes(s, p, D, F)
        if cfg.family == "wavlm":
            if cfg.relative_position_embedding and l == 0:
                s[f"{p}.self_attn.relative_attention_bias.weight"] = (cfg.num_buckets, H)
            if cfg.gru_rel_pos:
                s[f"{p}.self_attn.grep_linear.weight"] = (8, cfg.head_dim)
                s[f"{p}.self_attn.grep_linear.bias"] = (8,)
                s[f"{p}.self_attn.grep_a"] = (1, H, 1, 1)
    if cfg.pred_heads:  # distiller/model.py:155-161: Linear(D, D*N) -> GELU -> SplitLinear(D, N, D)
        N = cfg.pred_heads
        s["output_layer.0.weight"] = (D * N, D)
        s["output_layer.0.bias"] = (D * N,)
        s["output_layer.2.weight"] = (N, D, D)
        s["output_layer.2.bias"] = (1, 1, N, D)
    return s


def lighthubert_supernet_config(cfg: EncoderConfig) -> EncoderConfig:
    """The HuBERT-base shaped network a LightHuBERT checkpoint stores: 768 wide whatever subnet ``cfg`` runs (the reference
    hard-codes it), with ``cfg``'s extractor."""
    return EncoderConfig(family="hubert", conv_layers=cfg.conv_layers, extractor_mode=cfg.extractor_mode, conv_bias=cfg.conv_bias,
                         conv_pos=cfg.conv_pos, conv_pos_groups=cfg.conv_pos_groups, normalize=True)


def _lighthubert_shapes(cfg: EncoderConfig) -> Dict[str, tuple]:
    """The SUPERNET state dict of a LightHuBERT checkpoint (``s3prl_amd.ckpt.lighthubert_slice`` cuts it to ``cfg``'s subnet), with
    the two tensors the forward never reads, so that a written file is one the reference's ``load_state_dict`` takes."""
    s = param_shapes(lighthubert_supernet_config(cfg))
    s["mask_emb"] = (768,)
    s["layer_pred_heads.11.weight"] = (768, 768)
    return s


def _layer_shapes(s: Dict[str, tuple], p: str, D: int, F: int) -> None:
    for n in ("q_proj", "k_proj", "v_proj", "out_proj"):
        s[f"{p}.self_attn.{n}.weight"] = (D, D)
        s[f"{p}.self_attn.{n}.bias"] = (D,)
    s[f"{p}.self_attn_layer_norm.weight"] = (D,)
    s[f"{p}.self_attn_layer_norm.bias"] = (D,)
    s[f"{p}.fc1.weight"] = (F, D)
    s[f"{p}.fc1.bias"] = (F,)
    s[f"{p}.fc2.weight"] = (D, F)
    s[f"{p}.fc2.bias"] = (D,)
    s[f"{p}.final_layer_norm.weight"] = (D,)
    s[f"{p}.final_layer_norm.bias"] = (D,)


def _conformer_shapes(s: Dict[str, tuple], p: str, cfg: EncoderConfig) -> None:
    """ConformerWav2Vec2EncoderLayer (wav2vec2_model.py:440-578) parameters, reference state_dict names."""
    D, F, H, K = cfg.encoder_embed_dim, cfg.encoder_ffn_embed_dim, cfg.encoder_attention_heads, cfg.depthwise_conv_kernel_size
    for f in ("ffn1", "ffn2"):
        s[f"{p}.{f}.layer_norm.weight"] = (D,)
        s[f"{p}.{f}.layer_norm.bias"] = (D,)
        s[f"{p}.{f}.w_1.weight"] = (F, D)
        s[f"{p}.{f}.w_1.bias"] = (F,)
        s[f"{p}.{f}.w_2.weight"] = (D, F)
        s[f"{p}.{f}.w_2.bias"] = (D,)
    s[f"{p}.self_attn_layer_norm.weight"] = (D,)
    s[f"{p}.self_attn_layer_norm.bias"] = (D,)
    for n in ("linear_q", "linear_k", "linear_v", "linear_out"):
        s[f"{p}.self_attn.{n}.weight"] = (D, D)
        s[f"{p}.self_attn.{n}.bias"] = (D,)
    if cfg.pos_enc_type == "rel_pos":
        s[f"{p}.self_attn.linear_pos.weight"] = (D, D)
        s[f"{p}.self_attn.pos_bias_u"] = (H, D // H)
        s[f"{p}.self_attn.pos_bias_v"] = (H, D // H)
    s[f"{p}.conv_module.layer_norm.weight"] = (D,)
    s[f"{p}.conv_module.layer_norm.bias"] = (D,)
    s[f"{p}.conv_module.pointwise_conv1.weight"] = (2 * D, D, 1)
    s[f"{p}.conv_module.depthwise_conv.weight"] = (D, 1, K)
    for n in ("weight", "bias", "running_mean", "running_var"):
        s[f"{p}.conv_module.batch_norm.{n}"] = (D,)
    s[f"{p}.conv_module.pointwise_conv2.weight"] = (D, D, 1)
    s[f"{p}.final_layer_norm.weight"] = (D,)
    s[f"{p}.final_layer_norm.bias"] = (D,)


def _wav2vec_shapes(cfg: EncoderConfig) -> Dict[str, tuple]:
    """Wav2VecModel (upstream/wav2vec/wav2vec_model.py:565-700) parameters the forward reads, reference state_dict names;
    ``wav2vec_predictions.*`` / ``project_features.*`` are training-only."""
    s: Dict[str, tuple] = {}
    affine = not cfg.non_affine_group_norm
    cin = 1
    for i, (dim, k, _) in enumerate(cfg.conv_layers):
        p = f"feature_extractor.conv_layers.{i}"
        s[f"{p}.0.weight"] = (dim, cin, k)
        if affine:
            s[f"{p}.2.weight"] = (dim,)
            s[f"{p}.2.bias"] = (dim,)
        cin = dim
    C = cfg.conv_dim
    if cfg.vq_type != "none":
        G, V = cfg.vq_groups, cfg.vq_vars
        Gt, Dv = (1 if cfg.combine_groups else G), C // G
        if cfg.vq_type == "gumbel":
            s["vector_quantizer.vars"] = (1, Gt * V, Dv)
            if cfg.vq_depth > 1:
                for i in range(cfg.vq_depth - 1):
                    s[f"vector_quantizer.weight_proj.{i}.0.weight"] = (2 * C, C if i == 0 else 2 * C)
                    s[f"vector_quantizer.weight_proj.{i}.0.bias"] = (2 * C,)
                s[f"vector_quantizer.weight_proj.{cfg.vq_depth - 1}.weight"] = (G * V, 2 * C)
                s[f"vector_quantizer.weight_proj.{cfg.vq_depth - 1}.bias"] = (G * V,)
            else:
                s["vector_quantizer.weight_proj.weight"] = (G * V, C)
                s["vector_quantizer.weight_proj.bias"] = (G * V,)
        else:
            s["vector_quantizer.embedding"] = (V, Gt, Dv)
            s["vector_quantizer.projection.0.weight"] = (C, Dv, 1)
            s["vector_quantizer.projection.1.weight"] = (C,)
            s["vector_quantizer.projection.1.bias"] = (C,)
    for j, (dim, k, _) in enumerate(cfg.agg_layers):
        p = f"feature_aggregator.conv_layers.{j}"
        s[f"{p}.1.weight"] = (dim, C, k)
        if not cfg.no_conv_bias:
            s[f"{p}.1.bias"] = (dim,)
        if affine:
            s[f"{p}.3.weight"] = (dim,)
            s[f"{p}.3.bias"] = (dim,)
    return s


def _cpc_shapes(cfg: EncoderConfig) -> Dict[str, tuple]:
    """CPCModel (upstream/cpc/model.py:62-104,146-191) parameters, reference state_dict names."""
    s: Dict[str, tuple] = {}
    cin = 1
    for i, (dim, k, _) in enumerate(cfg.conv_layers):
        s[f"gEncoder.conv{i}.weight"] = (dim, cin, k)
        s[f"gEncoder.conv{i}.bias"] = (dim,)
        s[f"gEncoder.batchNorm{i}.weight"] = (1, dim, 1)
        s[f"gEncoder.batchNorm{i}.bias"] = (1, dim, 1)
        cin = dim
    G, H = (4 if cfg.ar_mode == "LSTM" else 3), cfg.ar_hidden
    for l in range(cfg.ar_layers):
        s[f"gAR.baseNet.weight_ih_l{l}"] = (G * H, cfg.conv_dim if l == 0 else H)
        s[f"gAR.baseNet.weight_hh_l{l}"] = (G * H, H)
        s[f"gAR.baseNet.bias_ih_l{l}"] = (G * H,)
        s[f"gAR.baseNet.bias_hh_l{l}"] = (G * H,)
    return s


def _apc_shapes(cfg: EncoderConfig) -> Dict[str, tuple]:
    """APC (upstream/apc/apc.py:41-48): the GRU layers, reference state_dict names.  ``postnet.*`` and VQ-APC's ``vq_layers.*``
    feed only the discarded prediction and are not hot-path parameters."""
    s: Dict[str, tuple] = {}
    H = cfg.conv_dim
    for l in range(cfg.apc_layers):
        s[f"rnn_layers.{l}.weight_ih_l0"] = (3 * H, cfg.apc_feat_dim if l == 0 else H)
        s[f"rnn_layers.{l}.weight_hh_l0"] = (3 * H, H)
        s[f"rnn_layers.{l}.bias_ih_l0"] = (3 * H,)
        s[f"rnn_layers.{l}.bias_hh_l0"] = (3 * H,)
    return s


def _npc_shapes(cfg: EncoderConfig) -> Dict[str, tuple]:
    """NPC (upstream/npc/npc.py:131-171), reference state_dict names: the ConvBlocks (with their BatchNorm statistics) and the
    masked convolutions.  ``postnet.*``, ``vq_layers.*``, the ``conv_mask`` buffers and ``num_batches_tracked`` are not hot-path
    parameters."""
    H, k = cfg.conv_dim, cfg.npc_kernel_size
    s: Dict[str, tuple] = {}
    for i in range(cfg.npc_blocks):
        s[f"blocks.{i}.conv.weight"] = (H, cfg.apc_feat_dim if i == 0 else H, 3)
        s[f"blocks.{i}.conv.bias"] = (H,)
        s[f"blocks.{i}.linear.weight"] = (H, H, 1)
        s[f"blocks.{i}.linear.bias"] = (H,)
        if cfg.npc_batch_norm:
            for bn in ("bn1", "bn2"):
                for leaf in ("weight", "bias", "running_mean", "running_var"):
                    s[f"blocks.{i}.{bn}.{leaf}"] = (H,)
        if cfg.npc_has_mask(i):
            s[f"masked_convs.{i}.conv.weight"] = (H, H, k)
            s[f"masked_convs.{i}.conv.bias"] = (H,)
    return s


def _vggish_shapes(cfg: EncoderConfig) -> Dict[str, tuple]:
    """VGGish (upstream/vggish/vggish.py:18-41,123-133), the names of the reference's two state dicts: ``features.K`` with K the
    conv's index in its ``nn.Sequential``, ``embeddings.{0,2,4}``, and — with the post-processor — ``pca_eigen_vectors`` and
    ``pca_means`` (held here as ``(D,)``; the reference reshapes whatever it is given to ``(D, 1)``)."""
    s: Dict[str, tuple] = {}
    cin, H, W = 1, cfg.vg_example_frames, cfg.vg_num_mel_bins
    for i, (ch, pool) in enumerate(cfg.vg_layers):
        s[f"features.{cfg.vg_seq_index(i)}.weight"] = (ch, cin, 3, 3)
        s[f"features.{cfg.vg_seq_index(i)}.bias"] = (ch,)
        cin = ch
        if pool:
            H, W = H // 2, W // 2
    k = H * W * cin
    for i, f in zip((0, 2, 4), cfg.vg_fc):
        s[f"embeddings.{i}.weight"] = (f, k)
        s[f"embeddings.{i}.bias"] = (f,)
        k = f
    if cfg.vg_postprocess:
        s["pca_eigen_vectors"] = (k, k)
        s["pca_means"] = (k,)
    return s


def _byol_a_shapes(cfg: EncoderConfig) -> Dict[str, tuple]:
    """AudioNTT2020 (upstream/byol_a/byol_a.py:91-137), the reference's state_dict names after its prefix rule: three Conv2d(., 64,
    3) at ``features.{0,4,8}`` each followed by a BatchNorm2d, ``fc.0`` (d, 64 * 8) and ``fc.3`` (d, d).  ``num_batches_tracked`` is
    training state and is not listed."""
    s: Dict[str, tuple] = {}
    cin, d = 1, cfg.conv_layers[0][0]
    for k in (0, 4, 8):
        s[f"features.{k}.weight"] = (64, cin, 3, 3)
        s[f"features.{k}.bias"] = (64,)
        for leaf in ("weight", "bias", "running_mean", "running_var"):
            s[f"features.{k + 1}.{leaf}"] = (64,)
        cin = 64
    s["fc.0.weight"], s["fc.0.bias"] = (d, 512), (d,)
    s["fc.3.weight"], s["fc.3.bias"] = (d, d), (d,)
    return s


def _mae_ast_shapes(cfg: EncoderConfig, full: bool = False) -> Dict[str, tuple]:
    """MAE_AST (upstream/mae_ast/mae_ast.py:202-281), reference state_dict names.  The hot path: the patch Linear, the BatchNorm's
    running statistics, the leading ``ma_pos_rows`` rows of the encoder's sinusoidal table, ``encoder.layer_norm`` and the encoder
    layers.  ``full``: the whole strict state dict — the table as ``(1, max_token_length, D)``, the decoder and its table, the
    reconstruction / classification heads, the mask embeddings, ``LayerNorm(feature_dim)`` and ``num_batches_tracked``."""
    D, F, K = cfg.encoder_embed_dim, cfg.encoder_ffn_embed_dim, cfg.ma_kt * cfg.ma_kc
    s: Dict[str, tuple] = {"post_extract_proj.weight": (D, K), "post_extract_proj.bias": (D,)}
    if full:
        s["layer_norm.weight"], s["layer_norm.bias"] = (cfg.ma_feature_dim,), (cfg.ma_feature_dim,)
    s["batch_norm.running_mean"], s["batch_norm.running_var"] = (1,), (1,)
    if full:
        s["batch_norm.num_batches_tracked"] = ()
        s["encoder_mask_emb"] = (D,)
    s["enc_sine_pos_embed.pe"] = (1, cfg.ma_max_token_length, D) if full else (cfg.ma_pos_rows, D)
    for l in range(cfg.encoder_layers):
        _layer_shapes(s, f"encoder.layers.{l}", D, F)
    s["encoder.layer_norm.weight"], s["encoder.layer_norm.bias"] = (D,), (D,)
    if full:
        s["decoder_mask_emb"] = (D,)
        if cfg.ma_dec_sine_pos:
            s["dec_sine_pos_embed.pe"] = (1, cfg.ma_max_token_length, D)
        for l in range(cfg.ma_decoder_layers):
            _layer_shapes(s, f"decoder.layers.{l}", D, F)
        s["decoder.layer_norm.weight"], s["decoder.layer_norm.bias"] = (D,), (D,)
        for head in ("final_proj_reconstruction", "final_proj_classification"):
            s[f"{head}.weight"], s[f"{head}.bias"] = (K, D), (K,)
    return s


def _ssast_shapes(cfg: EncoderConfig) -> Dict[str, tuple]:
    """The released SSAST file's own key layout (upstream/ssast/ast_models.py:96-208: a DataParallel-wrapped pretraining ASTModel
    around timm 0.4.5's distilled DeiT): ``module.v.*`` with the position table of the PRETRAINING grid, the pretraining input size as
    two scalar parameters, and what the upstream never reads — ``v.norm``, the two classifier heads, ``cpredlayer``, ``gpredlayer``,
    ``mask_embed``."""
    D, F = cfg.encoder_embed_dim, cfg.encoder_ffn_embed_dim
    pf, pt = cfg.ss_pretrain_grid
    s: Dict[str, tuple] = {"module.p_input_fdim": (), "module.p_input_tdim": (), "module.mask_embed": (1, 1, D),
                           "module.v.cls_token": (1, 1, D), "module.v.dist_token": (1, 1, D), "module.v.pos_embed": (1, pf * pt + 2, D),
                           "module.v.patch_embed.proj.weight": (D, 1, cfg.ss_fshape, cfg.ss_tshape), "module.v.patch_embed.proj.bias": (D,)}
    for l in range(cfg.encoder_layers):
        p = f"module.v.blocks.{l}"
        for name, shape in (("norm1", (D,)), ("attn.qkv", (3 * D, D)), ("attn.proj", (D, D)), ("norm2", (D,)), ("mlp.fc1", (F, D)),
                            ("mlp.fc2", (D, F))):
            s[f"{p}.{name}.weight"], s[f"{p}.{name}.bias"] = shape, shape[:1]
    s["module.v.norm.weight"], s["module.v.norm.bias"] = (D,), (D,)
    for head in ("module.v.head", "module.v.head_dist"):
        s[f"{head}.weight"], s[f"{head}.bias"] = (1000, D), (1000,)
    for head in ("module.cpredlayer", "module.gpredlayer"):
        s[f"{head}.0.weight"], s[f"{head}.0.bias"], s[f"{head}.2.weight"], s[f"{head}.2.bias"] = (D, D), (D,), (256, D), (256,)
    return s


def mae_ast_sine_table(rows: int, D: int) -> np.ndarray:
    """``SinusoidalPositionalEncoding.pe`` (mae_ast.py:802-812) by the reference's float32 formula: ``(1, rows, D)``."""
    import math

    position = np.arange(rows, dtype=np.float32)[:, None]
    div_term = np.exp(np.arange(0, D, 2).astype(np.float32) * np.float32(-math.log(10000.0) / D)).astype(np.float32)
    pe = np.zeros((1, rows, D), dtype=np.float32)
    pe[0, :, 0::2] = np.sin(position * div_term)
    pe[0, :, 1::2] = np.cos(position * div_term)
    return pe


def _byol_s_shapes(cfg: EncoderConfig) -> Dict[str, tuple]:
    """BYOL-S's networks under the reference's plain state_dict names.  ``default``: AudioNTT2020(n_mels=64, d=2048), BYOL-A's names
    (upstream/byol_s/byol_a/models/audio_ntt.py).  ``resnetish``: ResNetish(BasicBlock, blocks) (models/resnetish.py:159-290): the
    7 x 7 stem, and per block two bias-free 3 x 3 convolutions with their BatchNorms; the first block of layers 2-4 carries the 1 x 1
    ``downsample``.  ``num_batches_tracked`` is training state and is not listed."""
    if cfg.bs_network == "default":
        return _byol_a_shapes(cfg)
    s: Dict[str, tuple] = {"conv1.weight": (64, 1, 7, 7)}

    def bn(name, c):
        for leaf in ("weight", "bias", "running_mean", "running_var"):
            s[f"{name}.{leaf}"] = (c,)

    bn("bn1", 64)
    cin = 64
    for L, n_blocks in enumerate(cfg.bs_blocks):
        planes = 64 << L
        for b in range(n_blocks):
            pre = f"layer{L + 1}.{b}"
            s[f"{pre}.conv1.weight"] = (planes, cin, 3, 3)
            bn(f"{pre}.bn1", planes)
            s[f"{pre}.conv2.weight"] = (planes, planes, 3, 3)
            bn(f"{pre}.bn2", planes)
            if b == 0 and (L > 0 or cin != planes):
                s[f"{pre}.downsample.0.weight"] = (planes, cin, 1, 1)
                bn(f"{pre}.downsample.1", planes)
            cin = planes
    return s


def _decoar_shapes(cfg: EncoderConfig) -> Dict[str, tuple]:
    """Decoar (upstream/decoar/decoar.py:21-39), the checkpoint's names: the projection and the two multi-layer nn.LSTM modules
    (decoar_layers/expert.py:35-47 renames them to its per-layer modules; both experts read this one file)."""
    H = cfg.decoar_hidden
    s: Dict[str, tuple] = {"post_extract_proj.weight": (H, cfg.decoar_feat_dim), "post_extract_proj.bias": (H,)}
    for stack in ("forward_lstm", "backward_lstm"):
        for l in range(cfg.decoar_layers):
            s[f"{stack}.weight_ih_l{l}"] = (4 * H, H)
            s[f"{stack}.weight_hh_l{l}"] = (4 * H, H)
            s[f"{stack}.bias_ih_l{l}"] = (4 * H,)
            s[f"{stack}.bias_hh_l{l}"] = (4 * H,)
    return s


def _mockingjay_shapes(cfg: EncoderConfig) -> Dict[str, tuple]:
    """TransformerModel (upstream/mockingjay/model.py:102-386), reference state_dict names of the checkpoint's ``Transformer``.
    With ``share_layer`` the ModuleList holds one module under every index: only ``encoder.layer.0`` is a hot-path parameter."""
    D, F = cfg.encoder_embed_dim, cfg.encoder_ffn_embed_dim
    s: Dict[str, tuple] = {"input_representations.spec_transform.weight": (D, cfg.mj_input_dim),
                           "input_representations.spec_transform.bias": (D,),
                           "input_representations.LayerNorm.weight": (D,), "input_representations.LayerNorm.bias": (D,)}
    for l in range(1 if cfg.mj_share_layer else cfg.encoder_layers):
        p = f"encoder.layer.{l}"
        for n in ("attention.self.query", "attention.self.key", "attention.self.value", "attention.output.dense"):
            s[f"{p}.{n}.weight"], s[f"{p}.{n}.bias"] = (D, D), (D,)
        s[f"{p}.attention.output.LayerNorm.weight"], s[f"{p}.attention.output.LayerNorm.bias"] = (D,), (D,)
        s[f"{p}.intermediate.dense.weight"], s[f"{p}.intermediate.dense.bias"] = (F, D), (F,)
        s[f"{p}.output.dense.weight"], s[f"{p}.output.dense.bias"] = (D, F), (D,)
        s[f"{p}.output.LayerNorm.weight"], s[f"{p}.output.LayerNorm.bias"] = (D,), (D,)
    return s


def _multires_shapes(cfg: EncoderConfig, s: Dict[str, tuple]) -> Dict[str, tuple]:
    """multires-HuBERT (hubert_model.py:337-530): encoders.{i} / middle_encoder / decoders.{i} TransformerEncoders (only
    encoders.0 keeps its positional conv, :399-403,434-449) and the conv adapters between them."""
    D, F, k = cfg.encoder_embed_dim, cfg.encoder_ffn_embed_dim, cfg.conv_adapter_kernel
    R = len(cfg.rate_pairs) + 1
    names = [f"encoders.{i}" for i in range(R - 1)] + ["middle_encoder"] + [f"decoders.{i}" for i in range(R - 1)]
    for bi, name in enumerate(names):
        if bi == 0:
            s[f"{name}.pos_conv.0.bias"] = (D,)
            s[f"{name}.pos_conv.0.weight_g"] = (1, 1, cfg.conv_pos)
            s[f"{name}.pos_conv.0.weight_v"] = (D, D // cfg.conv_pos_groups, cfg.conv_pos)
        s[f"{name}.layer_norm.weight"] = (D,)
        s[f"{name}.layer_norm.bias"] = (D,)
        for l in range(cfg.block_layers[bi]):
            _layer_shapes(s, f"{name}.layers.{l}", D, F)
    for i in range(R - 1):
        for mod, convs in ((f"downsample_modules.{i}", ("downsample_conv",) if cfg.use_plain_updownsample
                            else ("upsample_conv", "downsample_conv")),
                           (f"upsample_modules.{i}", ("upsample_conv",) if cfg.use_plain_updownsample
                            else ("upsample_conv", "downsample_conv"))):
            for cv in convs:
                s[f"{mod}.{cv}.0.weight"] = (D, D, k)  # Conv1d (out, in, k) / ConvTranspose1d (in, out, k)
                s[f"{mod}.{cv}.2.weight"] = (D,)       # Fp32GroupNorm(1, D)
                s[f"{mod}.{cv}.2.bias"] = (D,)
    return s


PROFILES = ("synthetic", "pretrained_like")


def synth_weights(cfg: EncoderConfig, seed: int = 0, profile: str = "synthetic") -> Dict[str, np.ndarray]:
    """Seeded fp32 weights for every hot-path parameter.

    ``profile="synthetic"``: gaussian weights scaled so activations stay O(1) (every fixture of rounds 1-3).
    ``profile="pretrained_like"``: the same draw reshaped to the statistics released wav2vec 2.0 / HuBERT / WavLM checkpoints
    show and O(1) gaussians do not (``_pretrained_like``): outlier channels in the residual stream, LayerNorm gains of 2-4
    on a few channels, heavy-tailed (Student-t) matrices, key / query biases that shift every score of a row, a near-silent
    and a near-constant conv0 channel, a wide relative-position table.  What the reference's own regression test runs on
    (test/test_upstream.py:118-136 loads released checkpoints; there is no network here)."""
    if profile not in PROFILES:
        raise ValueError(f"profile must be one of {PROFILES}, got {profile!r}")
    out = _synthetic(cfg, seed)
    if cfg.family == "lighthubert":  # the statistics profile is the supernet's: a HuBERT-base shaped network
        return _pretrained_like(lighthubert_supernet_config(cfg), out, seed) if profile == "pretrained_like" else out
    return _pretrained_like(cfg, out, seed) if profile == "pretrained_like" else out


def _pretrained_like(cfg: EncoderConfig, w: Dict[str, np.ndarray], seed: int) -> Dict[str, np.ndarray]:
    """Reshape an O(1) draw into released-checkpoint statistics.  Every choice is a function of (cfg, seed) only."""
    rng = np.random.default_rng([seed, 0x5EED])
    D, C = cfg.encoder_embed_dim, cfg.conv_dim
    hot = rng.choice(D, size=4, replace=False)      # the residual stream's outlier channels (the same in every layer)
    warm = rng.choice(D, size=8, replace=False)     # channels with large LayerNorm gains only
    pre_ln = bool(cfg.layer_norm_first)

    def student_t(shape, df=4.0):  # unit variance, tails ~ |x|^-5: a released matrix has entries at 8-15 sigma
        return rng.standard_t(df, size=shape) * np.sqrt((df - 2.0) / df)

    out = {}
    for name, v in w.items():
        v = v.astype(np.float64)
        leaf = name.rsplit(".", 1)[-1]
        is_linear = leaf == "weight" and v.ndim == 2 and "relative_attention_bias" not in name and "grep" not in name
        if is_linear:
            v = student_t(v.shape) * v.std()
            if name.endswith((".fc2.weight", ".out_proj.weight")):
                # writers of the residual stream: the outlier channels receive 30-100x the typical update (pre-LN models
                # accumulate them over 24 layers to the "massive activations" of released large checkpoints) ...
                v[hot] *= rng.uniform(30.0, 100.0, size=(len(hot), 1)) if pre_ln else rng.uniform(8.0, 20.0, size=(len(hot), 1))
            if name.endswith((".fc1.weight", "q_proj.weight", "k_proj.weight", "v_proj.weight")):
                # ... and its readers have learned small weights on them and on the high-gain channels (otherwise every
                # logit saturates and fp32 itself is 1e-3 away from an fp64 evaluation: the "ref vs fp64" column of
                # tools/parity_table.py / profiles/r04_parity.md is the check that a profile stays well-conditioned)
                v[:, hot] *= 0.05 if pre_ln else 0.1
                v[:, warm] *= 0.3
        elif "conv_layers" in name and leaf == "weight" and v.ndim == 3:
            if name.startswith("feature_extractor.conv_layers.0."):
                v[1] *= 1e-4                                       # a near-silent filter: variance far below GroupNorm's eps
                v[2] = 0.3 * np.abs(v[2]).mean() + 1e-3 * v[2]     # a near-constant one (local average): mean >> deviation
                v[3:8] *= rng.uniform(5.0, 30.0, size=(5, 1, 1))   # and a few loud ones
            else:
                v = student_t(v.shape) * v.std()
        elif leaf == "weight" and v.ndim == 1:  # LayerNorm / GroupNorm gains
            if v.shape[0] == D:
                v[warm] *= rng.uniform(2.0, 4.0, size=len(warm))
                v[hot] *= (0.1 if pre_ln else 3.0)  # pre-LN: the outlier is squashed on read; post-LN: written by the gain
            else:
                idx = rng.choice(v.shape[0], size=6, replace=False)
                v[idx] *= rng.uniform(3.0, 8.0, size=6)
        elif leaf == "bias":
            if name.endswith(("k_proj.bias", "q_proj.bias")):
                v = v * 20.0  # std 1: q . b_k shifts all scores of a query by tens (softmax-invariant, unbounded in training)
            elif name.endswith((".fc2.bias", ".out_proj.bias")):
                v[hot] += rng.choice([-1.0, 1.0], size=len(hot)) * (rng.uniform(2.0, 6.0, size=len(hot)) if pre_ln else 1.0)
            elif v.shape[0] == D and "layer_norm" in name:
                v[hot] += rng.choice([-1.0, 1.0], size=len(hot)) * rng.uniform(1.0, 3.0, size=len(hot))
        elif name.endswith("relative_attention_bias.weight"):
            v = student_t(v.shape, 3.0) * 2.0  # released tables span roughly +-10
        out[name] = np.ascontiguousarray(v, dtype=np.float32)
    return out


def outlier_channels(cfg: EncoderConfig, seed: int) -> np.ndarray:
    """The residual-stream outlier channels ``_pretrained_like`` picks for (cfg, seed) (its first draw)."""
    return np.random.default_rng([seed, 0x5EED]).choice(cfg.encoder_embed_dim, size=4, replace=False)


def scale_outlier_writers(cfg: EncoderConfig, weights: Dict[str, np.ndarray], seed: int, factor: float) -> Dict[str, np.ndarray]:
    """A copy of pretrained-like ``weights`` whose residual-stream writers (rows of fc2 / out_proj and their biases on the
    outlier channels) are ``factor`` times louder: the knob of tools/fp16_cliff.py, which looks for the activation scale at
    which each 16-bit mode leaves its tolerance or its number range."""
    hot = outlier_channels(cfg, seed)
    out = dict(weights)
    for name, v in weights.items():
        if name.endswith((".fc2.weight", ".out_proj.weight", ".fc2.bias", ".out_proj.bias")):
            v = np.array(v, dtype=np.float32, copy=True)
            v[hot] *= np.float32(factor)
            out[name] = v
    return out


VGGISH_PCA_SCALE = 0.25  # x (embedding - mean): see _synthetic
VGGISH_EMB_MEAN = 1.0


def _synthetic(cfg: EncoderConfig, seed: int = 0) -> Dict[str, np.ndarray]:
    rng = np.random.default_rng(seed)
    out: Dict[str, np.ndarray] = {}
    # MAE-AST: the FULL strict state dict, so that the file a test writes is one the reference's expert loads
    for name, shape in (_mae_ast_shapes(cfg, full=True) if cfg.family == "mae_ast" else param_shapes(cfg)).items():
        leaf = name.rsplit(".", 1)[-1]
        if name.endswith("relative_attention_bias.weight"):
            w = rng.standard_normal(shape) * 0.5
        elif name.endswith("sine_pos_embed.pe"):
            w = mae_ast_sine_table(shape[1], shape[2])
        elif cfg.family == "mae_ast" and name.startswith("batch_norm."):
            # running statistics at log-mel scale (an AudioSet-style normaliser): the fold moves the bias by s * mean * rowsum(W)
            w = {"running_mean": lambda: -4.0 + 0.3 * rng.standard_normal(shape), "running_var": lambda: 20.0 + rng.uniform(-2.0, 2.0, size=shape),
                 "num_batches_tracked": lambda: np.full(shape, 1000.0)}[leaf]()
        elif name.endswith("_mask_emb"):
            w = rng.uniform(0.0, 1.0, size=shape)
        elif name in ("module.p_input_fdim", "module.p_input_tdim"):  # the pretraining input size, saved as parameters
            w = np.full(shape, cfg.ss_p_input_fdim if name.endswith("fdim") else cfg.ss_p_input_tdim)
        elif name.startswith("module.") and name.endswith(("cls_token", "dist_token", "mask_embed", "pos_embed")):
            # at the scale of the patch tokens (the released tables are trained: nothing like their 0.02 initialisation is left)
            w = 0.3 * rng.standard_normal(shape)
        elif name == "module.v.patch_embed.proj.weight":  # (D, 1, fshape, tshape) on a normalised log-mel image of RMS about 0.5
            w = rng.standard_normal(shape) * (2.0 / np.sqrt(shape[2] * shape[3]))
        elif name.startswith("gEncoder.batchNorm"):  # ChannelNorm (1, C, 1): gains 1 + 0.1 N(0, 1), shifts 0.05 N(0, 1)
            w = (1.0 if leaf == "weight" else 0.0) + (0.1 if leaf == "weight" else 0.05) * rng.standard_normal(shape)
        elif name.startswith("gEncoder.conv") and leaf == "weight":  # (out, in, k): unit variance in front of the channel norm
            w = rng.standard_normal(shape) * np.sqrt(1.0 / (shape[1] * shape[2]))
        elif name.startswith("gAR.baseNet.weight"):
            # input weights 2.5 / sqrt(fan_in) (6 / sqrt(fan_in) in layers 1.., whose inputs are hidden states of RMS 0.2-0.5),
            # recurrent weights 1.5 / sqrt(H): the gate pre-activations have a standard deviation above 1, so sigmoid and tanh are
            # exercised outside their linear range — torch's default U(-1/sqrt(H), 1/sqrt(H)) leaves the recurrent output below
            # 0.2 in magnitude — while an fp32 evaluation stays within 1e-6 of a float64 one (stronger recurrent weights
            # amplify every rounding error from step to step: at 3 / sqrt(H) the reference itself is 1.8e-6 away)
            gain = 1.5 if "weight_hh" in name else (2.5 if name.endswith("_l0") else 6.0)
            w = rng.standard_normal(shape) * (gain / np.sqrt(shape[1]))
        elif name.startswith("gAR.baseNet.bias"):
            w = 0.1 * rng.standard_normal(shape)
        elif name.startswith("rnn_layers.") and ".weight_" in name:
            # APC's GRU layers, by the rule above: the CMVN'd log-mel input has unit variance (2.5 / sqrt(fan_in)); the layers
            # behind read hidden states (plus, with the residual, the states below them)
            gain = 1.5 if "weight_hh" in name else (2.5 if name.startswith("rnn_layers.0.") else 4.0)
            w = rng.standard_normal(shape) * (gain / np.sqrt(shape[1]))
        elif name.startswith("rnn_layers.") and ".bias_" in name:
            w = 0.1 * rng.standard_normal(shape)
        elif name.startswith(("forward_lstm.weight", "backward_lstm.weight")):
            # DeCoAR's LSTM stacks, by the rule above: layer 0 reads the projection (unit variance: 2.5 / sqrt(fan_in)), the layers
            # behind read hidden states of RMS 0.2-0.5
            gain = 1.5 if "weight_hh" in name else (2.5 if name.endswith("_l0") else 6.0)
            w = rng.standard_normal(shape) * (gain / np.sqrt(shape[1]))
        elif name.startswith(("forward_lstm.bias", "backward_lstm.bias")):
            w = 0.1 * rng.standard_normal(shape)
        elif name.startswith("blocks.") and name.endswith((".conv.weight", ".linear.weight")):
            # NPC's ConvBlocks at unit gain, 1 / sqrt(fan_in): the CMVN'd log-mel input has unit variance and BatchNorm's statistics
            # below keep it there, so ReLU zeroes 30-55 % of a block's state and tanh is used on both sides of its bend, while the
            # reference's own fp32 stays within 5e-7 of its float64 (at twice this gain the activations reach std 180, the masked
            # states saturate at 98 % and the reference is 4e-6 from its double)
            # (tanh blocks: gain 1.5, or the states shrink from block to block)
            w = rng.standard_normal(shape) * ((1.5 if cfg.npc_activate == "tanh" else 1.0) / np.sqrt(shape[1] * shape[2]))
        elif name.startswith("masked_convs.") and leaf == "weight":
            # gain 1.6 over the LIVE taps (the masked ones never reach the output; a block's state has RMS 0.4-0.8): pre-activations
            # of std 0.6-1.1 in front of tanh
            live = shape[2] - cfg.npc_mask(int(name.split(".")[1]))
            w = rng.standard_normal(shape) * (1.6 / np.sqrt(shape[1] * live))
        elif name.startswith(("blocks.", "masked_convs.")) and name.endswith(("conv.bias", "linear.bias")):
            w = 0.1 * rng.standard_normal(shape)
        elif name.startswith("blocks.") and ".bn" in name:  # non-trivial eval statistics: the BatchNorm fold is exercised
            w = {"weight": lambda: 1.0 + 0.1 * rng.standard_normal(shape), "bias": lambda: -0.1 + 0.05 * rng.standard_normal(shape),
                 "running_mean": lambda: 0.2 * rng.standard_normal(shape), "running_var": lambda: rng.uniform(0.5, 2.0, size=shape)}[leaf]()
        elif cfg.family == "byol_a" and name.split(".")[1] in ("1", "5", "9") and name.startswith("features."):
            # eval-mode BatchNorm statistics that do something: running variances well away from zero, means and shifts that move
            # a good part of the channels across the ReLU's edge
            w = {"weight": lambda: 1.0 + 0.2 * rng.standard_normal(shape), "bias": lambda: 0.2 * rng.standard_normal(shape),
                 "running_mean": lambda: 0.3 * rng.standard_normal(shape), "running_var": lambda: rng.uniform(0.5, 2.0, size=shape)}[leaf]()
        elif cfg.family == "byol_a" and leaf == "weight":
            w = rng.standard_normal(shape) * np.sqrt(2.0 / int(np.prod(shape[1:])))  # He scaling, as for VGGish
        elif cfg.family == "byol_s" and cfg.bs_network == "default" and name.split(".")[1] in ("1", "5", "9") and name.startswith("features."):
            w = {"weight": lambda: 1.0 + 0.2 * rng.standard_normal(shape), "bias": lambda: 0.2 * rng.standard_normal(shape),
                 "running_mean": lambda: 0.3 * rng.standard_normal(shape), "running_var": lambda: rng.uniform(0.5, 2.0, size=shape)}[leaf]()
        elif cfg.family == "byol_s" and len(shape) == 1 and cfg.bs_network == "resnetish":
            # eval-mode BatchNorm statistics that do something, running variances well away from zero; the BatchNorm that closes a
            # residual branch (bn2, downsample.1) at half gain, so that sixteen additions do not double the map sixteen times
            gain = 0.5 if (".bn2." in name or ".downsample.1." in name) else 1.0
            w = {"weight": lambda: gain * (1.0 + 0.2 * rng.standard_normal(shape)), "bias": lambda: 0.2 * rng.standard_normal(shape),
                 "running_mean": lambda: 0.3 * rng.standard_normal(shape), "running_var": lambda: rng.uniform(0.5, 2.0, size=shape)}[leaf]()
        elif cfg.family == "byol_s" and leaf == "weight":
            w = rng.standard_normal(shape) * np.sqrt(2.0 / int(np.prod(shape[1:])))  # He scaling through every conv and Linear
        elif cfg.family == "vggish" and leaf == "weight":
            # He scaling, sqrt(2 / fan_in), through every conv and Linear: ReLU then keeps the second moment of the log-mel input
            # (RMS 3-4 for unit-variance PCM) up to the embedding, about half of whose elements are exact zeros
            w = rng.standard_normal(shape) * np.sqrt(2.0 / int(np.prod(shape[1:])))
        elif name == "pca_eigen_vectors":
            # an orthogonal matrix times a fixed scale: every output mixes all embedding dimensions with unit-norm rows, and the
            # scale puts the output's spread (VGGISH_PCA_SCALE x the embedding's) at about a third of the quantiser's half range
            q, r = np.linalg.qr(rng.standard_normal(shape))
            w = VGGISH_PCA_SCALE * q * np.sign(np.diag(r))
        elif name == "pca_means":
            # near the embedding's mean (about VGGISH_EMB_MEAN per element under the rule above), so that the quantiser's input is
            # centred in its range
            w = VGGISH_EMB_MEAN * (1.0 + 0.1 * rng.standard_normal(shape))
        elif name in ("vector_quantizer.embedding", "vector_quantizer.vars"):
            # codebooks at the scale of what they are compared with / replace (a trained k-means embedding lives where the
            # normalised projection does: unit variance; the reference's 0.01 * randn init leaves argmin decisions at rounding level)
            w = rng.standard_normal(shape) if name.endswith("embedding") else rng.uniform(0.0, 1.0, size=shape)
        elif name.startswith("vector_quantizer.weight_proj") and leaf == "weight":
            w = rng.standard_normal(shape) * np.sqrt(2.0 / shape[-1])
        elif name == "vector_quantizer.projection.0.weight":
            w = rng.standard_normal(shape) * np.sqrt(1.0 / shape[1])
        elif name.endswith("batch_norm.running_mean"):  # non-trivial eval statistics: the BatchNorm fold is exercised
            w = 0.2 * rng.standard_normal(shape)
        elif name.endswith("batch_norm.running_var"):
            w = rng.uniform(0.5, 2.0, size=shape)
        elif name.endswith(("pos_bias_u", "pos_bias_v")):
            w = 0.3 * rng.standard_normal(shape)
        elif name.endswith("depthwise_conv.weight"):  # (D, 1, K)
            w = rng.standard_normal(shape) * np.sqrt(1.0 / shape[-1])
        elif name.endswith(("pointwise_conv1.weight", "pointwise_conv2.weight")):  # (out, in, 1)
            w = rng.standard_normal(shape) * np.sqrt(1.0 / shape[1])
        elif name.endswith("grep_a"):
            w = 1.0 + 0.3 * rng.standard_normal(shape)
        elif name.endswith("weight_g"):
            # weight_norm gain: w[:,:,k] = g[k] * v[:,:,k] / ||v[:,:,k]||  → RMS(w) = g/sqrt(numel per tap)
            d_out, d_in, _ = param_shapes(cfg)[name[:-1] + "v"]
            w = (1.0 + 0.2 * rng.standard_normal(shape)) * np.sqrt(d_out / shape[-1]) * 0.5
        elif name == "output_layer.2.weight":  # SplitLinear (N, Din, Dout)
            w = rng.standard_normal(shape) * np.sqrt(1.0 / shape[1])
        elif leaf == "weight" and len(shape) == 1:  # norm gains
            w = 1.0 + 0.1 * rng.standard_normal(shape)
        elif leaf == "bias":
            w = 0.05 * rng.standard_normal(shape)
        elif "pos_conv" in name and leaf == "weight":  # data2vec conv block (out, in/g, k)
            w = rng.standard_normal(shape) * np.sqrt(2.0 / (shape[1] * shape[2]))
        elif "sample_conv.0" in name:  # conv adapters (D, D, k): unit-variance output before the GroupNorm
            w = rng.standard_normal(shape) * np.sqrt(1.0 / (shape[1] * shape[2]))
        elif "conv_layers" in name:  # (out, in, k): keep unit variance through GELU (gain ~ sqrt(2.5))
            fan_in = shape[1] * shape[2]
            w = rng.standard_normal(shape) * np.sqrt(2.5 / fan_in)
        elif leaf == "weight_v":
            w = rng.standard_normal(shape)
        else:  # linear (out, in)
            gain = 2.0 if ".fc2." in name else 1.0
            w = rng.standard_normal(shape) * np.sqrt(gain / shape[-1])
        out[name] = np.ascontiguousarray(w, dtype=np.float32)
    return out


def synth_wavs(lengths: List[int], seed: int = 1234, dc: float = 0.0, scale: float = 1.0) -> List[np.ndarray]:
    """Seeded gaussian 'waveforms' (the reference's own convention: ``torch.randn``,
    s3prl/util/pseudo_data.py:70). numpy-generated so both sides can rebuild them offline."""
    rng = np.random.default_rng(seed)
    return [(rng.standard_normal(n) * scale + dc).astype(np.float32) for n in lengths]


def pseudo_lengths(n: int = 2, min_secs: float = 1.0, max_secs: float = 3.0, seed: int = 0,
                   sample_rate: int = 16000) -> List[int]:
    """Lengths in the style of ``get_pseudo_wavs`` (s3prl/util/pseudo_data.py:52-77): n utterances
    between min_secs and max_secs."""
    rng = np.random.default_rng(seed)
    lo, hi = int(min_secs * sample_rate), int(max_secs * sample_rate)
    return [int(rng.integers(lo, hi + 1)) for _ in range(n)]


# ------------------------------------------------------------------------------------------
# named configurations
# ------------------------------------------------------------------------------------------

def named_config(name: str) -> EncoderConfig:
    """Architectures named by BASELINE.json plus tiny variants of each for fast tests.

    Large-model hyper-parameters are not in the reference tree (they live in the released
    checkpoints); the values follow SURVEY §8c.
    """
    tiny_conv = [(64, 10, 5)] + [(64, 3, 2)] * 4 + [(64, 2, 2)] * 2
    tiny = dict(conv_layers=tiny_conv, encoder_layers=3, encoder_embed_dim=128,
                encoder_ffn_embed_dim=256, encoder_attention_heads=2, conv_pos=16, conv_pos_groups=4)
    large = dict(extractor_mode="layer_norm", encoder_layers=24, encoder_embed_dim=1024,
                 encoder_ffn_embed_dim=4096, encoder_attention_heads=16, layer_norm_first=True,
                 normalize=True)
    table = {
        "hubert_base": dict(family="hubert"),
        "wav2vec2_base": dict(family="wav2vec2"),
        "wavlm_base": dict(family="wavlm"),
        "wavlm_base_plus": dict(family="wavlm", relative_position_embedding=True, num_buckets=320,
                                max_distance=800, gru_rel_pos=True),
        "hubert_large": dict(family="hubert", conv_bias=False, **large),
        "wav2vec2_large": dict(family="wav2vec2", conv_bias=True, **large),
        "wavlm_large": dict(family="wavlm", conv_bias=False, relative_position_embedding=True,
                            num_buckets=320, max_distance=800, gru_rel_pos=True, **large),
        "distilhubert": dict(family="distiller", encoder_layers=2, feature_layer_norm=False, pred_heads=3),
        "tiny_distiller": dict(family="distiller", feature_layer_norm=False, pred_heads=3, **{**tiny, "encoder_layers": 2}),
        "tiny_wavlm_norel": dict(family="wavlm", **tiny),
        "data2vec_base": dict(family="wav2vec2", extractor_mode="layer_norm", conv_pos=95, pos_conv_depth=5, normalize=True),
        "tiny_data2vec": dict(family="wav2vec2", **{**tiny, "extractor_mode": "layer_norm", "conv_pos": 15,
                                                   "pos_conv_depth": 3, "normalize": True}),
        "tiny_hubert": dict(family="hubert", **tiny),
        # DeCoAR 2.0 (upstream/decoar2): HuBERT-base's post-LN encoder behind the kaldi front end; the released shape, which the
        # reference hard-codes (decoar2/decoar2.py:9-24), and a narrow one
        "decoar2": dict(family="decoar2", conv_layers=[(80, 400, 160)], conv_bias=False),
        "tiny_decoar2": dict(family="decoar2", conv_layers=[(80, 400, 160)], conv_bias=False, encoder_layers=2, encoder_embed_dim=128,
                             encoder_ffn_embed_dim=256, encoder_attention_heads=2, conv_pos=16, conv_pos_groups=4),
        "tiny_decoar2_d192": dict(family="decoar2", conv_layers=[(80, 400, 160)], conv_bias=False, encoder_layers=2,
                                  encoder_embed_dim=192, encoder_ffn_embed_dim=384, encoder_attention_heads=3, conv_pos=16,
                                  conv_pos_groups=4),  # group width 48, the released one
        # LightHuBERT (upstream/lighthubert): the subnets its three released checkpoints run.  The reference hard-codes the 768-wide
        # 12-layer supernet and the subnet shapes, so there is no tiny variant: synth_weights draws the supernet at its real width
        "lighthubert_base": dict(family="lighthubert", lh_model="hubert_pruner", lh_supernet="base", extractor_mode="layer_norm",
                                 normalize=True, encoder_embed_dim=640, encoder_ffn_embed_dim=2560, encoder_attention_heads=10),
        "lighthubert_small": dict(family="lighthubert", lh_model="hubert_pruner", lh_supernet="small", extractor_mode="layer_norm",
                                  normalize=True, encoder_embed_dim=384, encoder_ffn_embed_dim=1536, encoder_attention_heads=6),
        "lighthubert_stage1": dict(family="lighthubert", lh_model="student_hubert", lh_supernet="base", extractor_mode="layer_norm",
                                   normalize=True),
        # multires-HuBERT (mrhubert_mono_base: 20 ms -> 40 ms -> 20 ms, 4 layers each; the hyper-parameters are those of
        # the released checkpoint's config as far as the reference tree shows them: hubert_model.py:97-330 defaults)
        "multires_hubert_base": dict(family="multires_hubert", label_rate_ratios=[1, 2], block_layers=[4, 4, 4]),
        "tiny_multires": dict(family="multires_hubert", label_rate_ratios=[1, 2], block_layers=[2, 1, 2],
                              **{**tiny, "encoder_layers": 5}),
        "tiny_multires_large": dict(family="multires_hubert", label_rate_ratios=[1, 2], block_layers=[1, 2, 1],
                                    **{**tiny, "encoder_layers": 4, "extractor_mode": "layer_norm",
                                       "layer_norm_first": True, "normalize": True}),
        "tiny_multires3": dict(family="multires_hubert", label_rate_ratios=[1, 2, 1, 2], block_layers=[1, 1, 2, 1, 1],
                               **{**tiny, "encoder_layers": 6}),
        "tiny_multires_plain": dict(family="multires_hubert", label_rate_ratios=[1, 2], block_layers=[1, 1, 1],
                                    use_plain_updownsample=True, **{**tiny, "encoder_layers": 3}),
        "tiny_wav2vec2": dict(family="wav2vec2", **tiny),
        # wav2vec 2.0 Conformer (ConformerEncoder): rel_pos / rope, post-LN tiny and the large released shape (pre-LN,
        # layer-norm extractor; a released checkpoint's own config decides at load time)
        "tiny_conformer_relpos": dict(family="wav2vec2", layer_type="conformer", pos_enc_type="rel_pos", attn_type="espnet",
                                      **{**tiny, "extractor_mode": "layer_norm", "layer_norm_first": True, "normalize": True}),
        "tiny_conformer_rope": dict(family="wav2vec2", layer_type="conformer", pos_enc_type="rope", attn_type="espnet",
                                    **{**tiny, "extractor_mode": "layer_norm", "layer_norm_first": True, "normalize": True}),
        "tiny_conformer_rope_postln": dict(family="wav2vec2", layer_type="conformer", pos_enc_type="rope", attn_type="espnet",
                                           **tiny),
        "wav2vec2_conformer_large_relpos": dict(family="wav2vec2", conv_bias=True, layer_type="conformer", pos_enc_type="rel_pos",
                                                attn_type="espnet", **large),
        "wav2vec2_conformer_large_rope": dict(family="wav2vec2", conv_bias=True, layer_type="conformer", pos_enc_type="rope",
                                              attn_type="espnet", **large),
        "tiny_hubert_large": dict(family="hubert", **{**tiny, "extractor_mode": "layer_norm",
                                                      "layer_norm_first": True, "normalize": True,
                                                      "conv_bias": True}),
        "tiny_wav2vec2_large": dict(family="wav2vec2", **{**tiny, "extractor_mode": "layer_norm",
                                                          "layer_norm_first": True, "normalize": True,
                                                          "conv_bias": True}),
        "tiny_wavlm": dict(family="wavlm", relative_position_embedding=True, num_buckets=32,
                           max_distance=64, gru_rel_pos=True, **tiny),
        "tiny_wavlm_large": dict(family="wavlm", relative_position_embedding=True, num_buckets=32,
                                 max_distance=64, gru_rel_pos=True,
                                 **{**tiny, "extractor_mode": "layer_norm", "layer_norm_first": True,
                                    "normalize": True}),
    }
    # wav2vec / vq-wav2vec: the seven extractor layers at their real kernels and strides (receptive field 465, hop 160)
    w2v_feat = lambda C: [(C, 10, 5), (C, 8, 4), (C, 4, 2), (C, 4, 2), (C, 4, 2), (C, 1, 1), (C, 1, 1)]  # noqa: E731
    w2v_tiny = dict(conv_layers=w2v_feat(64), agg_layers=[(64, k, 1) for k in range(2, 6)])
    w2v = {
        "tiny_wav2vec": dict(**w2v_tiny),
        "tiny_wav2vec_zeropad_noaffine": dict(agg_zero_pad=True, non_affine_group_norm=True, no_conv_bias=True,
                                              skip_connections_agg=False, log_compression=False, **w2v_tiny),
        "tiny_vq_wav2vec_gumbel": dict(vq_type="gumbel", vq_vars=32, vq_groups=2, vq_depth=2, **w2v_tiny),
        "tiny_vq_wav2vec_kmeans": dict(vq_type="kmeans", vq_vars=32, vq_groups=2, **w2v_tiny),
        # the released wav2vec_large shape as published with the model (a checkpoint's own config decides at load time)
        "wav2vec_large": dict(conv_layers=w2v_feat(512), agg_layers=[(512, k, 1) for k in range(2, 14)]),
    }
    if name in w2v:
        from .config import wav2vec_config

        return wav2vec_config(**w2v[name])
    # modified CPC: the five convolutions at their real kernels, strides and paddings (receptive field 159 + 160 n, hop 160)
    cpc = {
        "tiny_cpc": dict(hidden=64, ar_mode="LSTM", ar_layers=2),
        "tiny_cpc_gru": dict(hidden=64, ar_mode="GRU", ar_layers=1),
        "tiny_cpc_lstm1": dict(hidden=64, ar_mode="LSTM", ar_layers=1),
        # the shape the released 60k_epoch4 checkpoint is believed to carry (a checkpoint's own config decides at load time)
        "cpc_base": dict(hidden=256, ar_mode="LSTM", ar_layers=2),
    }
    if name in cpc:
        from .config import cpc_config

        return cpc_config(**cpc[name])
    # APC / VQ-APC: 25 ms / 10 ms hamming log-mel (80 bins, CMVN) into GRU layers on packed sequences
    apc = {
        "tiny_apc": dict(hidden=64, num_layers=3, residual=True),
        "tiny_apc_nores": dict(hidden=64, num_layers=3, residual=False),
        "tiny_apc_nocmvn": dict(hidden=64, num_layers=3, residual=True, cmvn=False),  # a one-frame utterance has no std
        "tiny_apc_l4": dict(hidden=64, num_layers=4, residual=True),
        "tiny_vq_apc": dict(hidden=128, num_layers=3, residual=True,
                            vq=dict(codebook_size=[32], code_dim=[128], gumbel_temperature=0.5)),
        # the released apc_360hr / vq_apc_360hr shape (a checkpoint's own config decides at load time)
        "apc_360hr": dict(hidden=512, num_layers=3, residual=True),
    }
    if name in apc:
        from .config import apc_config

        return apc_config(**apc[name])
    # DeCoAR / DeCoAR-layers: the same front end, Linear 80 -> H, a forward and a backward LSTM stack on packed sequences
    decoar = {
        "tiny_decoar": dict(hidden=64, num_layers=2),
        "tiny_decoar_layers": dict(hidden=64, num_layers=3, per_layer=True),
        "tiny_decoar_l1": dict(hidden=64, num_layers=1),
        "tiny_decoar_h192": dict(hidden=192, num_layers=2, per_layer=True),
        "tiny_decoar_sub2": dict(hidden=64, num_layers=2, per_layer=True, subsample=2),
        # the released shape (decoar/decoar.py hard-codes it): one state for `decoar`, four for `decoar_layers`
        "decoar": dict(hidden=1024, num_layers=4),
        "decoar_layers": dict(hidden=1024, num_layers=4, per_layer=True),
    }
    if name in decoar:
        from .config import decoar_config

        return decoar_config(**decoar[name])
    # NPC: APC's front end, ConvBlocks and masked convolutions; no length masking
    tiny_npc = dict(hidden=64, n_blocks=4, kernel_size=15, mask_size=5, feat_dim=16)
    npc = {
        "tiny_npc": dict(tiny_npc, vq=dict(codebook_size=[8, 8], code_dim=[32, 32], gumbel_temperature=1.0)),
        "tiny_npc_plain": dict(tiny_npc, batch_norm=False, activate="tanh", residual=False),
        "tiny_npc_nocmvn": dict(tiny_npc, cmvn=False),  # a one-frame utterance has no std
        "tiny_npc_last": dict(tiny_npc, disable_cross_layer=True),
        "tiny_npc_k9": dict(hidden=64, n_blocks=3, kernel_size=9, mask_size=1, feat_dim=16),
        "tiny_npc_h192": dict(tiny_npc, hidden=192, feat_dim=80),
        # the released npc_360hr / npc_960hr shape (a checkpoint's own config decides at load time)
        "npc_360hr": dict(hidden=512, n_blocks=4, kernel_size=15, mask_size=5, residual=True, batch_norm=True, activate="relu",
                          vq=dict(codebook_size=[64, 64, 64, 64], code_dim=[128, 128, 128, 128], gumbel_temperature=1.0)),
    }
    if name in npc:
        from .config import npc_config

        return npc_config(**npc[name])
    # VGGish: un-padded log-mel examples, a 3 x 3 conv + pool stack, three Linears, the PCA / 8-bit quantiser
    vggish = {
        "vggish": dict(),  # the released shape: 96 x 64 examples, [64, M, 128, M, 256, 256, M, 512, 512, M], 4096 / 4096 / 128
        "vggish_raw": dict(postprocess=False),
        "tiny_vggish": dict(layers=[16, "M", 32, "M", 32, 32, "M", 64, 64, "M"], fc=(128, 128, 32), example_frames=16, num_mel_bins=16),
        "tiny_vggish_raw": dict(layers=[16, "M", 32, "M", 32, 32, "M", 64, 64, "M"], fc=(128, 128, 32), example_frames=16,
                                num_mel_bins=16, postprocess=False),
        # channel counts that are no multiple of 64, a 3 x 1 last map
        "tiny_vggish_odd": dict(layers=[16, "M", 48, "M", 48, "M"], fc=(128, 128, 32), example_frames=24, num_mel_bins=8),
        "tiny_vggish_odd_raw": dict(layers=[16, "M", 48, "M", 48, "M"], fc=(128, 128, 32), example_frames=24, num_mel_bins=8,
                                    postprocess=False),
    }
    if name in vggish:
        from .config import vggish_config

        return vggish_config(**vggish[name])
    # BYOL-A: FFT log-mel segments, three conv + BatchNorm + floor-pool layers, two Linears, max + mean over time
    byol_a = {
        "byol_a_2048": dict(feature_d=2048), "byol_a_1024": dict(feature_d=1024), "byol_a_512": dict(feature_d=512),
        "tiny_byol_a": dict(feature_d=64),
        "tiny_byol_a_overlap": dict(feature_d=64, window_secs=1.0, stride_secs=0.5),
        "tiny_byol_a_win025": dict(feature_d=64, window_secs=0.25, stride_secs=0.1),  # 26 frames -> 13 -> 6 -> 3: odd at two levels
    }
    if name in byol_a:
        from .config import byol_a_config

        return byol_a_config(**byol_a[name])
    # MAE-AST: kaldi log-mel at 128 bins, kt x kc patches, sinusoidal positions, Transformer layers with key padding
    tiny_ma = dict(embed_dim=128, layers=2, heads=2, ffn=256, max_token_length=640)
    mae_ast = {
        "mae_ast_patch": dict(kt=16, kc=16), "mae_ast_frame": dict(kt=2, kc=128),
        # the released shapes with position tables of 1024 rows (the full-size fixtures: a 48000-row table is 147 MB a piece)
        "mae_ast_patch_t1024": dict(kt=16, kc=16, max_token_length=1024), "mae_ast_frame_t1024": dict(kt=2, kc=128, max_token_length=1024),
        "tiny_mae_ast": dict(kt=16, kc=16, **tiny_ma),
        "tiny_mae_ast_frame": dict(kt=2, kc=128, **tiny_ma),
        "tiny_mae_ast_preln": dict(kt=16, kc=16, **{**tiny_ma, "layers": 3}, layer_norm_first=True),
        "tiny_mae_ast_k3x32": dict(kt=3, kc=32, **tiny_ma),
    }
    if name in mae_ast:
        from .config import mae_ast_config

        return mae_ast_config(**mae_ast[name])
    # SSAST: fixed windows, hanning kaldi log-mel, overlapping Conv2d patches behind cls / dist, pre-LN timm blocks
    tiny_ss = dict(embed_dim=128, heads=2, layers=2, window_secs=0.5)
    ssast = {
        "ssast_patch_base": dict(model_type="p"), "ssast_frame_base": dict(model_type="f"),
        "ssast_patch_base_l2": dict(model_type="p", layers=2), "ssast_frame_base_l2": dict(model_type="f", layers=2),
        # 0.5 s windows: 50 image rows, 12 x 4 + 2 = 50 tokens (patch), 49 + 2 = 51 tokens (frame)
        "tiny_ssast_patch": dict(model_type="p", **tiny_ss, p_input_tdim=1024),  # p_t_dim 64 > t_dim 4: the centre cut
        "tiny_ssast_frame": dict(model_type="f", **tiny_ss, p_input_tdim=1024),  # p_t_dim 512 > t_dim 49: the centre cut
        "tiny_ssast_patch_interp": dict(model_type="p", **tiny_ss, p_input_tdim=48),  # p_t_dim 3 < t_dim 4: the interpolation
        "tiny_ssast_frame_interp": dict(model_type="f", **tiny_ss, p_input_tdim=60),  # p_t_dim 30 < t_dim 49
        "tiny_ssast_patch_d192": dict(model_type="p", model_size="tiny", layers=2, window_secs=0.5),
        "tiny_ssast_patch_w1": dict(model_type="p", embed_dim=128, heads=2, layers=2, window_secs=1.0),
    }
    if name in ssast:
        from .config import ssast_config

        return ssast_config(**ssast[name])
    # BYOL-S: centred windows, hann(400) log-mel, whole-batch statistics, AudioNTT2020 or a ResNet of BasicBlocks, mean + max
    byol_s = {
        "byol_s_default": dict(network="default"), "byol_s_resnetish34": dict(network="resnetish", blocks=(3, 4, 6, 3)),
        "tiny_byol_s_default": dict(network="default", window_secs=0.25, hop_secs=0.1),
        "tiny_byol_s_resnetish10": dict(network="resnetish", blocks=(1, 1, 1, 1)),
        # 26 frames -> 13 -> 7 -> 4 -> 2: odd at two levels
        "tiny_byol_s_resnetish10_win025": dict(network="resnetish", blocks=(1, 1, 1, 1), window_secs=0.25, hop_secs=0.1),
        "tiny_byol_s_resnetish10_hop02": dict(network="resnetish", blocks=(1, 1, 1, 1), window_secs=0.5, hop_secs=0.2),
    }
    if name in byol_s:
        from .config import byol_s_config

        return byol_s_config(**byol_s[name])
    # Mockingjay / TERA / AudioALBERT: a log-mel (or kaldi fbank) front end into post-LN BERT layers, long inputs in chunks
    tiny_mj = dict(hidden=128, layers=2, heads=2, intermediate=256, input_dim=16, sequence_length=0)
    mj = {
        "tiny_mockingjay": dict(**tiny_mj),
        "tiny_mockingjay_chunk": dict(**{**tiny_mj, "sequence_length": 16}),
        "tiny_mockingjay_chunk3": dict(**{**tiny_mj, "sequence_length": 3}),
        "tiny_mockingjay_eps": dict(**tiny_mj, layer_norm_eps=1e-2),
        "tiny_mockingjay_albert": dict(**{**tiny_mj, "layers": 3}, share_layer=True),
        "tiny_mockingjay_kaldi": dict(**{**tiny_mj, "input_dim": 24}, frontend="kaldi", mj_kaldi_mel_bins=8, mj_delta_order=2),
        # pretrain/{tera,mockingjay,audio_albert}/config_model*.yaml (a checkpoint's own config decides at load time)
        "tera_base": dict(hidden=768, layers=3, heads=12, intermediate=3072, input_dim=80, sequence_length=1500),
        "mockingjay_base": dict(hidden=768, layers=3, heads=12, intermediate=3072, input_dim=240, sequence_length=1500,
                                frontend="kaldi"),
        "mockingjay_large": dict(hidden=768, layers=12, heads=12, intermediate=3072, input_dim=80, sequence_length=500),
        "audio_albert_base": dict(hidden=768, layers=3, heads=12, intermediate=3072, input_dim=80, sequence_length=1500,
                                  share_layer=True),
    }
    if name in mj:
        from .config import mockingjay_config

        return mockingjay_config(**mj[name])
    if name not in table:
        raise KeyError(f"unknown config {name!r}; have {sorted(list(table) + list(w2v) + list(cpc) + list(apc) + list(decoar) + list(npc) + list(vggish) + list(byol_a) + list(byol_s) + list(mae_ast) + list(ssast) + list(mj))}")
    cfg = EncoderConfig(**table[name])
    cfg.validate()
    return cfg
