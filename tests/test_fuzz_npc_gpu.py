"""Seeded sweep over the NPC configurations s3enc_create_npc accepts — 1..5 blocks, kernel sizes 5 / 9 / 15 with every mask that
leaves a tap, BatchNorm on and off, both activations, with and without the residual and the cross-layer sum — on ragged batches of
1..4 utterances between 400 and 6000 samples, with utterances of exactly one frame drawn in, against the float64 restatement
(tests/npc_ref.py) FROM THE WAVEFORMS, scored per (state, utterance) on ALL rows: the rows behind an utterance's frames are the
reference's values, not zeros.  The fixtures of tests/test_npc_gpu.py pin the released geometry against the reference itself; this
guards the generality npc_check_config promises.

A one-frame utterance has no standard deviation over time (CMVN gives nan in torch, in the restatement and here alike), so the
seeds that draw one in run without CMVN."""

import functools

import numpy as np
import pytest

from oracle import encoder_oracle as O

import npc_ref as R

pytestmark = pytest.mark.gpu

FP32_TOL = 1e-4  # the suite's exact-fp32 bar
N_SEEDS = 24
WIDTHS = (64, 128, 192, 256)
KERNELS = (5, 9, 15)


def case_inputs(seed):
    """(cfg, lengths, waveforms, weights) of a sweep seed: widths, kernel sizes, the flags cycle so that every value appears with
    every other, the rest is drawn."""
    from s3prl_amd.config import npc_config
    from s3prl_amd.synth import synth_wavs, synth_weights

    rng = np.random.default_rng(9700 + seed)
    H = WIDTHS[seed % 4]
    k = KERNELS[seed % 3]
    cross = bool((seed // 2) % 2)
    one_frame = seed % 5 == 0
    # blocks 1..5 and an odd mask such that the last masked conv keeps a tap: mask + 2 n_blocks < k (cross-layer or not)
    n_blocks = int(rng.integers(1, min(5, (k - 2) // 2) + 1))
    mask = int(rng.choice(np.arange(1, k - 2 * n_blocks, 2)))
    cfg = npc_config(H, n_blocks, k, mask, residual=bool((seed // 4) % 2), batch_norm=bool((seed // 8) % 2 == 0),
                     activate=("relu", "tanh")[(seed // 3) % 2], disable_cross_layer=not cross, feat_dim=(16, 80, 32)[seed % 3],
                     cmvn=not one_frame)
    B = int(rng.integers(1, 5))
    lengths = [int(rng.integers(560, 6001)) for _ in range(B)]
    if one_frame:
        lengths[int(rng.integers(B))] = int(rng.choice([400, 559]))  # exactly one frame (alone in the batch: T = 1)
    wavs = synth_wavs(lengths, seed + 1, dc=float(rng.choice([0.0, 0.2])), scale=float(rng.choice([1.0, 0.1])))
    return cfg, lengths, wavs, synth_weights(cfg, 900 + seed)


@functools.lru_cache(maxsize=None)
def case(seed):
    cfg, lengths, wavs, weights = case_inputs(seed)
    return cfg, lengths, wavs, weights, R.forward(cfg, weights, wavs)


def test_the_sweep_covers_what_it_says():
    cfgs = [case_inputs(s)[0] for s in range(N_SEEDS)]
    assert {c.npc_blocks for c in cfgs} >= {1, 2, 3, 4} and {c.npc_kernel_size for c in cfgs} == set(KERNELS)
    assert {c.npc_activate for c in cfgs} == {"relu", "tanh"}
    for flag in ("npc_residual", "npc_batch_norm", "npc_disable_cross_layer", "apc_cmvn"):
        assert {getattr(c, flag) for c in cfgs} == {True, False}, flag
    assert any(min(case_inputs(s)[1]) < 560 for s in range(N_SEEDS))


@pytest.mark.parametrize("seed", range(N_SEEDS))
def test_random_npc_matches_float64(seed):
    import torch

    from s3prl_amd.encoder import HipEncoder

    assert torch.cuda.is_available(), "these tests need the MI355X"
    cfg, lengths, wavs, weights, ref = case(seed)
    n_max = max(lengths)
    T, H, B = cfg.num_frames(n_max), cfg.conv_dim, len(wavs)
    valid = [cfg.valid_frames(n, n_max) for n in lengths]
    assert valid == ref["lengths"] and min(valid) >= 1
    NS = cfg.num_hidden_states
    dev = [torch.from_numpy(w).cuda() for w in wavs]
    enc = HipEncoder(cfg, weights)
    assert enc.num_states() == NS == len(ref["hidden_states"])
    assert [enc.valid_frames(n, n_max) for n in lengths] == valid
    hs = enc.forward(dev).clone()
    torch.cuda.synchronize()
    assert tuple(hs.shape) == (NS, B, T, H)
    got = hs.cpu().numpy()
    assert np.isfinite(got).all()
    worst = 0.0
    for l in range(NS):
        for b in range(B):  # all T rows: the padded ones are the reference's values too
            worst = max(worst, O.rel_err(got[l][b], ref["hidden_states"][l][b]))
    what = (f"seed {seed}: H {H} x {cfg.npc_blocks} blocks k {cfg.npc_kernel_size} mask {cfg.npc_mask_size} bn {cfg.npc_batch_norm} "
            f"{cfg.npc_activate} residual {cfg.npc_residual} cross {not cfg.npc_disable_cross_layer} cmvn {cfg.apc_cmvn} F {cfg.apc_feat_dim}")
    print(f"{what} lengths {lengths} frames {valid}: worst per-(state, utterance) rel-err {worst:.2e}")
    assert worst < FP32_TOL, (what, lengths, worst)
    assert enc.status() == 0

    # a second handle: the batch permuted, and a shard of it padded to the batch's n_max, reproduce the rows bit for bit
    other = HipEncoder(cfg, weights)
    perm = [int(i) for i in np.random.default_rng(seed).permutation(B)]
    permuted = other.forward([dev[i] for i in perm]).clone()
    for j, i in enumerate(perm):
        assert torch.equal(permuted[:, j], hs[:, i]), (what, "permuted", j, i)
    lo = B // 2
    shard = other.forward(dev[lo:], n_max=n_max).clone()
    torch.cuda.synchronize()
    assert torch.equal(shard, hs[:, lo:]), (what, "shard")
    enc.close()
    other.close()
