"""Seeded sweep over the wav2vec 2.0 Conformer encoders EncoderConfig.validate accepts — rel_pos and rope, 1..4 heads (D = 64..256),
depthwise kernels 1..63, FFN widths off the tile, 1..3 layers, both norm placements and extractor modes — on ragged batches whose
longest utterance sits at the edges of the conv module's 128-frame tile, its 8-frame thread groups and the attention row tiles,
against the float64 restatement (tests/conformer_ref.py), scored per (state, utterance) over the utterance's valid frames.  The
fixtures of tests/test_conformer_gpu.py pin the released geometry at D = 128 / 256 and kernel 31; this guards the rest."""

import functools

import numpy as np
import pytest

from oracle import encoder_oracle as O

import conformer_ref as R

pytestmark = pytest.mark.gpu

FP32_TOL = 1e-4
N_SEEDS = 20
T_LONGEST = [1, 17, 63, 64, 65, 127, 128, 129, 136, 257]  # seed i: T_LONGEST[i % 10], so every entry is in the sweep twice
KERNELS = [1, 3, 7, 15, 31, 63]                            # seed i: KERNELS[i % 6], every kernel at three lengths or more


def _random_conformer_config(rng, seed=None):
    from s3prl_amd.config import EncoderConfig

    heads = int(rng.choice([1, 2, 3, 4]))
    if seed is not None and seed < 4:
        heads = seed + 1  # D = 64, 128, 192, 256 by construction
    D = 64 * heads
    groups = [g for g in (1, 2, 3, 4, 6, 8) if D % g == 0 and D // g in (32, 48, 64)]  # the group widths the library builds
    C = int(rng.choice([32, 64, 96]))
    n_mid = int(rng.integers(1, 5))
    conv = [(C, 10, 5)] + [(C, int(rng.choice([2, 3])), int(rng.choice([1, 2]))) for _ in range(n_mid)] + [(C, 2, 2)]
    K = int(rng.choice(KERNELS))
    pos = str(rng.choice(["rel_pos", "rope"]))
    if seed is not None:
        K = KERNELS[seed % len(KERNELS)]
        pos = ["rel_pos", "rope"][(seed // 2) % 2]  # with the lengths' period of 10: both kinds at every length
    cfg = EncoderConfig(family="wav2vec2", layer_type="conformer", attn_type="espnet", pos_enc_type=pos, conv_layers=conv,
                        encoder_embed_dim=D, encoder_attention_heads=heads, depthwise_conv_kernel_size=K,
                        conv_pos=int(rng.choice([3, 8, 15, 16, 31, 32])), conv_pos_groups=int(rng.choice(groups)),
                        encoder_ffn_embed_dim=int(rng.choice([64, 136, 256, 320])), encoder_layers=int(rng.integers(1, 4)),
                        layer_norm_first=bool(rng.integers(2)), extractor_mode=str(rng.choice(["default", "layer_norm"])),
                        conv_bias=bool(rng.integers(2)), normalize=bool(rng.integers(2)))
    cfg.validate()
    return cfg


def receptive_field(cfg):
    rf, hop = 1, 1
    for _, k, s in cfg.conv_layers:
        rf += (k - 1) * hop
        hop *= s
    return rf, hop


def case_inputs(seed):
    """(cfg, lengths, waveforms): 1..4 utterances, the longest of exactly T_LONGEST[seed % 10] frames at a random place of the
    batch, the others anywhere between one frame and that"""
    from s3prl_amd.synth import synth_wavs

    rng = np.random.default_rng(11000 + seed)
    cfg = _random_conformer_config(rng, seed)
    rf, hop = receptive_field(cfg)
    T = T_LONGEST[seed % len(T_LONGEST)]
    B = int(rng.integers(1, 5))
    longest = rf + (T - 1) * hop + int(rng.integers(hop))
    lengths = [int(rng.integers(rf, longest + 1)) for _ in range(B - 1)]
    lengths.insert(int(rng.integers(B)), longest)
    wavs = synth_wavs(lengths, seed + 1, dc=float(rng.choice([0.0, 0.2])), scale=float(rng.choice([1.0, 0.1])))
    return cfg, T, lengths, wavs


@functools.lru_cache(maxsize=None)
def case(seed):
    from s3prl_amd.synth import synth_weights

    cfg, T, lengths, wavs = case_inputs(seed)
    weights = synth_weights(cfg, seed)
    return cfg, T, lengths, wavs, weights, R.forward(cfg, weights, wavs)


def per_utterance_errors(got, ref, valid):
    """worst rel-err over (state, utterance), each over the utterance's valid frames only"""
    return max(O.rel_err(got[l][b, :v], ref[l][b, :v]) for l in range(len(ref)) for b, v in enumerate(valid))


@pytest.mark.parametrize("seed", range(N_SEEDS))
def test_random_conformer_matches_float64(seed):
    import torch

    from s3prl_amd.encoder import HipEncoder

    assert torch.cuda.is_available(), "these tests need the MI355X"
    cfg, T, lengths, wavs, weights, ref = case(seed)
    n_max = max(lengths)
    valid = [cfg.valid_frames(n, n_max) for n in lengths]
    enc = HipEncoder(cfg, weights)
    assert enc.num_states() == cfg.encoder_layers + 1 == len(ref) and enc.num_frames(n_max) == T == max(valid)
    hs = enc.forward([torch.from_numpy(w).cuda() for w in wavs])
    torch.cuda.synchronize()
    assert tuple(hs.shape) == (len(ref), len(wavs), T, cfg.encoder_embed_dim)
    got = hs.cpu().numpy()
    assert np.isfinite(got).all()
    err = per_utterance_errors(got, ref, valid)
    # the padded frames as the fixtures treat them: part of the whole-state comparison, at the same bar
    whole = max(O.rel_err(got[l], ref[l]) for l in range(len(ref)))
    what = (f"seed {seed}: {cfg.pos_enc_type} D {cfg.encoder_embed_dim} K {cfg.depthwise_conv_kernel_size} F {cfg.encoder_ffn_embed_dim} "
            f"NL {cfg.encoder_layers} pre-LN {cfg.layer_norm_first} {cfg.extractor_mode} T {T} valid {valid}")
    print(f"{what}: worst per-(state, utterance) rel-err {err:.2e}, whole states {whole:.2e}")
    assert err < FP32_TOL, (what, err)
    assert whole < FP32_TOL, (what, whole)
    assert enc.status() == 0
    enc.close()


def test_group_widths_the_library_refuses_are_refused_by_validate_too():
    """The handle packs the positional conv of a Conformer checkpoint as well, so s3enc_create holds embed_dim / conv_pos_groups
    to the widths the positional-conv kernels are built for; EncoderConfig.validate names the same limit."""
    import ctypes as C
    import dataclasses

    from s3prl_amd import _lib
    from s3prl_amd.synth import named_config

    cfg = dataclasses.replace(named_config("tiny_conformer_rope"), conv_pos_groups=16)  # 128 / 16 = 8
    with pytest.raises(ValueError, match="32, 48 or 64"):
        cfg.validate()
    lib = _lib.load()
    ccfg = _lib.make_config(cfg, "fp32")
    h = C.c_void_p()
    tensors = (_lib.S3Tensor * 1)()
    assert lib.s3enc_create(C.byref(ccfg), tensors, 0, 0, C.byref(h)) != 0
    assert b"32, 48 or 64" in lib.s3enc_last_error()
