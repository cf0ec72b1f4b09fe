"""The CPU leg of tests/test_fuzz_wav2vec_gpu.py: every seed of the sweep is a configuration both config checks accept, the sweep
contains the pinned corners, a weight seed without near-tie decisions exists within the cap, and the float32 run of the restatement
decides like its float64 run — so an id the GPU gets wrong is the GPU's, not the rounding's."""

import numpy as np
import pytest

from oracle import encoder_oracle as O

import test_fuzz_wav2vec_gpu as F
import wav2vec_ref as R


def test_sweep_contains_the_pinned_corners():
    cfgs = [F.case_inputs(seed)[0] for seed in range(F.N_SEEDS)]
    assert F.N_SEEDS >= 24
    km = [c for c in cfgs if c.vq_type == "kmeans"]
    gb = [c for c in cfgs if c.vq_type == "gumbel"]
    assert {512, 4} <= {c.conv_dim // c.vq_groups for c in km}
    assert any(c.vq_groups == 16 for c in km + gb)
    assert {1, 3, 4} <= {c.vq_depth for c in gb}
    assert any(c.vq_vars == 1 for c in gb) and any(c.vq_vars == 1 for c in km)
    assert any(c.combine_groups for c in km + gb) and any(not c.combine_groups for c in km + gb)
    assert {544, 1024} <= {c.conv_dim for c in cfgs}                                   # gn1_apply templates 3 and 4
    assert {1, 64} <= {k for c in cfgs for _, k, _ in c.agg_layers}                   # pad == 0 and the largest kernel
    assert 2 in {len(c.conv_layers) for c in cfgs}
    assert {1, 2, 3, 5, 8} == {c.conv_layers[0][2] for c in cfgs}                      # every conv0 stride of the draw
    assert {0.5, 0.25} == {c.residual_scale for c in cfgs}
    assert any(c.vq_type == "none" for c in cfgs)


@pytest.mark.parametrize("seed", range(F.N_SEEDS))
def test_seed_is_valid_and_its_decisions_are_no_near_ties(seed):
    from s3prl_amd.synth import param_shapes

    cfg, lengths, wavs = F.case_inputs(seed)
    cfg.validate()
    rf, hop = F.receptive_field(cfg)
    assert hop == cfg.downsample_rate and cfg.num_frames(rf) == 1 and cfg.num_frames(rf - 1) == 0
    assert 1 <= len(lengths) <= 4 and min(lengths) == rf
    T = cfg.num_frames(max(lengths))
    assert T == 1 if len(lengths) == 1 else 20 <= T <= 70
    wseed, weights, ref = F.pick_weights(cfg, wavs, seed)  # raises when the cap of MAX_TRIES weight seeds is not enough
    assert 100 * seed <= wseed < 100 * seed + F.MAX_TRIES and set(weights) == set(param_shapes(cfg))
    assert len(ref["hidden_states"]) == len(cfg.agg_layers) + 1
    assert all(h.shape == (len(lengths), T, cfg.conv_dim) and np.isfinite(h).all() for h in ref["hidden_states"])
    f32 = R.forward(cfg, weights, wavs, dtype=np.float32)
    valid = [cfg.valid_frames(n, max(lengths)) for n in lengths]
    err = F.per_utterance_errors(f32["hidden_states"], ref["hidden_states"], valid)
    assert err < 1e-5, (seed, err)
    if cfg.vq_type != "none":
        assert ref["margin"] >= F.MIN_MARGIN
        assert ref["codeids"].shape == (len(lengths), T, cfg.vq_groups)
        assert np.array_equal(f32["codeids"], ref["codeids"]), (seed, wseed, ref["margin"])
        assert O.rel_err(f32["codewords"], ref["codewords"]) < 1e-5
        assert ref["codeids"].min() >= 0 and ref["codeids"].max() < cfg.vq_vars
    print(f"seed {seed}: weight seed {wseed} margin {ref['margin']} float32-vs-float64 {err:.1e}")
