"""float64 restatement of the LightHuBERT expert (TEST HELPER, not product code): the cut of the supernet to its subnet and the
forward, written from the behaviour the fixtures pin (``tests/golden/lighthubert/``, produced by the reference's own expert).

Slicing (``subnet_weights``), stated independently of ``s3prl_amd.ckpt.lighthubert_slice``:

* LayerNorms, ``post_extract_proj``, q / k / v / out_proj: leading rows and columns;
* fc1: the supernet's 3072 rows are four blocks of 768; the subnet keeps the leading ``embed`` rows of each block (and the leading
  ``embed`` columns); fc2 the same along its columns;
* positional conv: ``w = g * v / ||v||`` with the norm per tap over ALL 768 x 48 entries of the unsliced ``weight_v``, THEN
  ``w[:embed, :embed // 16, :]`` with 16 groups kept: new group g owns filters [g dg, (g + 1) dg) and reads the first dg columns.

Forward: every waveform normalised, HuBERT's conv extractor / LayerNorm / frame mask / projection, padded frames zeroed, positional
conv + residual, LayerNorm, 12 post-LN layers with the padded frames masked as keys (the reference's padding of T to a multiple of 2
adds one masked key and changes nothing).  The states are the projection output (padded rows exactly zero) and the 12 layer outputs —
the front end, the positional conv and the layers are those of ``oracle.encoder_oracle`` on the sliced tensors."""

from __future__ import annotations

from typing import Dict, List

import numpy as np

from oracle import encoder_oracle as O

SUPER_E, SUPER_F, GROUPS_BLOCKS = 768, 3072, 4


def subnet_weights(cfg, sd: Dict[str, np.ndarray], fold_before_slice: bool = True) -> Dict[str, np.ndarray]:
    """The supernet state dict ``sd`` cut to ``cfg``'s subnet, float64, under HuBERT's names; the positional conv is returned folded,
    as ``encoder.pos_conv.0.weight``.  ``fold_before_slice=False`` is the WRONG order (norm over the sliced tensor), kept so that a
    test can show the two differ."""
    E, F, G = cfg.encoder_embed_dim, cfg.encoder_ffn_embed_dim, cfg.conv_pos_groups
    W = {k: np.asarray(v, dtype=np.float64) for k, v in sd.items()}
    out = {k: v for k, v in W.items() if k.startswith(("feature_extractor.", "layer_norm."))}
    out["post_extract_proj.weight"] = W["post_extract_proj.weight"][:E, :]
    out["post_extract_proj.bias"] = W["post_extract_proj.bias"][:E]
    v, g = W["encoder.pos_conv.0.weight_v"], W["encoder.pos_conv.0.weight_g"]
    assert v.shape[:2] == (SUPER_E, SUPER_E // G) and g.shape == (1, 1, v.shape[2])
    if fold_before_slice:
        w = (v * (g / np.sqrt(np.sum(v * v, axis=(0, 1), keepdims=True))))[:E, :E // G, :]
    else:
        vs = v[:E, :E // G, :]
        w = vs * (g / np.sqrt(np.sum(vs * vs, axis=(0, 1), keepdims=True)))
    out["encoder.pos_conv.0.weight"] = w
    out["encoder.pos_conv.0.bias"] = W["encoder.pos_conv.0.bias"][:E]
    for leaf in ("weight", "bias"):
        out[f"encoder.layer_norm.{leaf}"] = W[f"encoder.layer_norm.{leaf}"][:E]
    if F == SUPER_F:
        rows = np.arange(SUPER_F)
    else:
        assert F == GROUPS_BLOCKS * E
        rows = np.concatenate([np.arange(b * SUPER_E, b * SUPER_E + E) for b in range(GROUPS_BLOCKS)])
    for l in range(cfg.encoder_layers):
        p = f"encoder.layers.{l}"
        for n in ("q_proj", "k_proj", "v_proj", "out_proj"):
            out[f"{p}.self_attn.{n}.weight"] = W[f"{p}.self_attn.{n}.weight"][:E, :E]
            out[f"{p}.self_attn.{n}.bias"] = W[f"{p}.self_attn.{n}.bias"][:E]
        for n in ("self_attn_layer_norm", "final_layer_norm"):
            for leaf in ("weight", "bias"):
                out[f"{p}.{n}.{leaf}"] = W[f"{p}.{n}.{leaf}"][:E]
        out[f"{p}.fc1.weight"] = W[f"{p}.fc1.weight"][rows][:, :E]
        out[f"{p}.fc1.bias"] = W[f"{p}.fc1.bias"][rows]
        out[f"{p}.fc2.weight"] = W[f"{p}.fc2.weight"][:E][:, rows]
        out[f"{p}.fc2.bias"] = W[f"{p}.fc2.bias"][:E]
    return out


def hubert_view(cfg):
    """The subnet as a post-LN HuBERT configuration (HuBERT's frame mask; the waveform always normalised)."""
    from s3prl_amd.config import EncoderConfig

    keep = ("conv_layers", "extractor_mode", "conv_bias", "encoder_layers", "encoder_embed_dim", "encoder_ffn_embed_dim",
            "encoder_attention_heads", "layer_norm_first", "conv_pos", "conv_pos_groups")
    return EncoderConfig(family="hubert", normalize=True, **{k: getattr(cfg, k) for k in keep})


def forward(cfg, sd: Dict[str, np.ndarray], wavs: List[np.ndarray], n_max=None) -> List[np.ndarray]:
    """``UpstreamExpert(ckpt)(wavs)["hidden_states"]`` in float64: 13 x (B, T, embed)."""
    assert cfg.family == "lighthubert" and not cfg.layer_norm_first and cfg.pos_conv_depth == 1
    W = subnet_weights(cfg, sd)
    w = W.pop("encoder.pos_conv.0.weight")
    # the oracle folds weight_g * weight_v / ||weight_v||: hand it the folded filter with g = its own per-tap norm (an identity in float64)
    W["encoder.pos_conv.0.weight_v"] = w
    W["encoder.pos_conv.0.weight_g"] = np.sqrt(np.sum(w * w, axis=(0, 1), keepdims=True))
    hv = hubert_view(cfg)
    taps: dict = {}
    xs = [np.asarray(x, dtype=np.float64) for x in wavs]
    single = len(xs) == 1  # (the oracle's strided conv is ten times slower on a batch of one: run the utterance twice, keep one row)
    if single:
        n_max = len(xs[0]) if n_max is None else n_max
        xs = xs * 2
    layer_out = O.forward(hv, W, xs, dtype=np.float64, n_max=n_max, taps=taps, selection="fairseq_layers")
    states = [taps["proj"]] + list(layer_out)
    return [s[:1] for s in states] if single else states


def valid_frames(cfg, lengths, n_max=None) -> List[int]:
    n_max = max(lengths) if n_max is None else n_max
    hv = hubert_view(cfg)
    return [hv.valid_frames(int(n), int(n_max)) for n in lengths]
