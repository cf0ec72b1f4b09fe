"""The CPU leg of tests/test_fuzz_conformer_gpu.py: the generator only produces configurations EncoderConfig.validate accepts, the
sweep contains every length, kernel and width it promises, and the float64 reference runs every seed quickly."""

import time

import numpy as np
import pytest

import test_fuzz_conformer_gpu as F


def test_sweep_contains_every_length_kernel_and_width():
    cases = [F.case_inputs(seed) for seed in range(F.N_SEEDS)]
    assert F.N_SEEDS >= 16
    assert {T for _, T, _, _ in cases} == {1, 17, 63, 64, 65, 127, 128, 129, 136, 257}
    assert {c.depthwise_conv_kernel_size for c, _, _, _ in cases} == {1, 3, 7, 15, 31, 63}
    assert {c.encoder_embed_dim for c, _, _, _ in cases} == {64, 128, 192, 256}
    for T in F.T_LONGEST:  # rel_pos and rope at every length
        assert {c.pos_enc_type for c, t, _, _ in cases if t == T} == {"rel_pos", "rope"}
    assert {c.layer_norm_first for c, _, _, _ in cases} == {False, True}
    assert {c.extractor_mode for c, _, _, _ in cases} == {"default", "layer_norm"}
    assert {len(l) for _, _, l, _ in cases} == {1, 2, 3, 4}


def test_unseeded_draws_validate():
    rng = np.random.default_rng(5)
    for _ in range(200):
        cfg = F._random_conformer_config(rng)  # validate() inside
        assert cfg.layer_type == "conformer" and cfg.head_dim == 64 and cfg.depthwise_conv_kernel_size % 2 == 1


@pytest.mark.parametrize("seed", range(F.N_SEEDS))
def test_seed_validates_and_the_reference_runs_it(seed):
    cfg, T, lengths, wavs = F.case_inputs(seed)
    cfg.validate()
    rf, hop = F.receptive_field(cfg)
    assert cfg.num_frames(rf) == 1 and cfg.num_frames(rf - 1) == 0 and hop == cfg.downsample_rate
    assert 1 <= len(lengths) <= 4 and min(lengths) >= rf and cfg.num_frames(max(lengths)) == T
    F.case.cache_clear()
    t0 = time.perf_counter()
    ref = F.case(seed)[-1]
    dt = time.perf_counter() - t0
    assert len(ref) == cfg.encoder_layers + 1
    assert all(h.shape == (len(lengths), T, cfg.encoder_embed_dim) and np.isfinite(h).all() for h in ref)
    assert dt < 20.0, f"the float64 reference took {dt:.1f} s for seed {seed}"  # (a second at the largest seed; bounded, not tuned)


@pytest.mark.parametrize("D,groups,ok", [(128, 4, True), (128, 2, True), (192, 4, True), (128, 16, False), (64, 4, False), (256, 1, False)])
def test_validate_names_the_positional_conv_group_widths(D, groups, ok):
    """embed_dim / conv_pos_groups must be 32, 48 or 64 for every layer type, as s3enc_create demands (include/s3enc.h)"""
    import dataclasses

    from s3prl_amd.synth import named_config

    for name in ("tiny_conformer_relpos", "tiny_hubert"):
        cfg = dataclasses.replace(named_config(name), encoder_embed_dim=D, encoder_attention_heads=D // 64, conv_pos_groups=groups)
        if ok:
            cfg.validate()
        else:
            with pytest.raises(ValueError, match="32, 48 or 64"):
                cfg.validate()
    with pytest.raises(ValueError, match="1..256"):
        dataclasses.replace(named_config("tiny_hubert"), conv_pos=257).validate()
