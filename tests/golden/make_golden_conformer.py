#!/usr/bin/env python3
"""Generate the wav2vec 2.0 Conformer fixtures in this directory by RUNNING THE REFERENCE (PyTorch CPU).

Run in the build container only (it imports the reference tree through ``ref_shim``; it does not exist on the GPU box):

    python tests/golden/make_golden_conformer.py                 # all cases
    python tests/golden/make_golden_conformer.py conformer_relpos_tiny_pad

Same recipe and ``.npz`` meta format as ``make_golden.py``, written to ``tests/golden/conformer/`` (``conftest.load_golden``
reads them as ``"conformer/<case>"``; the Transformer suites enumerate the top-level fixtures only): the seeded numpy weights of
``s3prl_amd.synth.synth_weights`` are loaded into the reference ``Wav2Vec2Model(Wav2Vec2Config(layer_type="conformer",
pos_enc_type=..., attn_type="espnet"))``, saved in the reference's converted-checkpoint format, and the reference
``wav2vec2.expert.UpstreamExpert(ckpt)(wavs)["hidden_states"]`` is recorded.
"""

from __future__ import annotations

import dataclasses
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

from make_golden import _import_reference, _load  # noqa: E402
from s3prl_amd.synth import named_config, synth_wavs, synth_weights  # noqa: E402

# name -> (config, weight seed, wav seed, lengths, (t_stride, c_stride) subsampling of stored tensors, dc, scale)
# 800 samples = 2 frames: shorter than the 31-tap depthwise window; 16000 samples = 49 frames (T % 32 = 17)
CASES = {
    "conformer_relpos_tiny_pad": ("tiny_conformer_relpos", 71, 81, [4000, 2345, 3111, 800], (1, 1), 0.0, 1.0),
    "conformer_rope_tiny_pad": ("tiny_conformer_rope", 72, 82, [4000, 2345, 3111, 800], (1, 1), 0.0, 1.0),
    "conformer_rope_postln_tiny_pad": ("tiny_conformer_rope_postln", 73, 83, [3500, 4000, 1700], (1, 1), 0.0, 1.0),
    "conformer_relpos_tiny_eq": ("tiny_conformer_relpos", 74, 84, [3200, 3200], (1, 1), 0.1, 0.5),
    "conformer_relpos_tiny_t49": ("tiny_conformer_relpos", 75, 85, [16000], (1, 1), 0.0, 1.0),
    "conformer_relpos_large_pseudo": ("wav2vec2_conformer_large_relpos", 0, 86, [16000, 12000], (4, 16), 0.0, 1.0),
    "conformer_rope_large_pseudo": ("wav2vec2_conformer_large_rope", 0, 87, [16000, 12000], (4, 16), 0.0, 1.0),
}


def reference_hidden_states(cfg, weights, wavs):
    import torch

    _import_reference()
    from s3prl.upstream.wav2vec2.expert import UpstreamExpert
    from s3prl.upstream.wav2vec2.wav2vec2_model import AudioPretrainingConfig, Wav2Vec2Config, Wav2Vec2Model

    torch.manual_seed(0)
    mc = Wav2Vec2Config(
        extractor_mode=cfg.extractor_mode, conv_bias=cfg.conv_bias, encoder_layers=cfg.encoder_layers,
        encoder_embed_dim=cfg.encoder_embed_dim, encoder_ffn_embed_dim=cfg.encoder_ffn_embed_dim,
        encoder_attention_heads=cfg.encoder_attention_heads, layer_norm_first=cfg.layer_norm_first,
        conv_pos=cfg.conv_pos, conv_pos_groups=cfg.conv_pos_groups, conv_feature_layers=str([tuple(t) for t in cfg.conv_layers]),
        layer_type="conformer", pos_enc_type=cfg.pos_enc_type, attn_type=cfg.attn_type,
        depthwise_conv_kernel_size=cfg.depthwise_conv_kernel_size,
        quantize_targets=True, final_dim=32, latent_vars=8, latent_groups=2)
    tc = AudioPretrainingConfig(normalize=cfg.normalize)
    model = Wav2Vec2Model(mc)
    _load(model, weights)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "ckpt.pt")
        torch.save({"task_cfg": dataclasses.asdict(tc), "model_cfg": dataclasses.asdict(mc), "model_weight": model.state_dict()},
                   path)
        expert = UpstreamExpert(path).eval()
        with torch.no_grad():
            out = expert([torch.from_numpy(w.copy()) for w in wavs])
    return [h.numpy() for h in out["hidden_states"]]


def make_case(name: str):
    cfg_name, wseed, xseed, lengths, (ts, cs), dc, scale = CASES[name]
    cfg = named_config(cfg_name)
    weights = synth_weights(cfg, wseed)
    wavs = synth_wavs(lengths, xseed, dc=dc, scale=scale)
    hs = reference_hidden_states(cfg, weights, wavs)
    assert len(hs) == cfg.num_hidden_states
    meta = dict(config=cfg_name, weight_seed=wseed, wav_seed=xseed, lengths=lengths, t_stride=ts, c_stride=cs, dc=dc,
                scale=scale, shape=list(hs[0].shape), reference="s3prl 0.4.18 @ /root/reference, torch CPU fp32",
                n_states=len(hs))
    arrays = {f"hs{l}": np.ascontiguousarray(h[:, ::ts, ::cs]) for l, h in enumerate(hs)}
    arrays["norms"] = np.array([np.linalg.norm(h.astype(np.float64)) for h in hs])
    arrays["meta"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    path = os.path.join(HERE, "conformer", f"{name}.npz")
    np.savez_compressed(path, **arrays)
    print(f"{name}: {len(hs)} x {hs[0].shape} -> {os.path.getsize(path) / 1e3:.0f} kB")


if __name__ == "__main__":
    for n in sys.argv[1:] or list(CASES):
        make_case(n)
