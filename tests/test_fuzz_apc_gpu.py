"""Seeded sweep over the APC configurations s3enc_create_apc accepts — hidden sizes 64..256, three or four GRU layers, with and
without the residual — on ragged batches of 1..4 utterances between 400 and 6000 samples, with utterances of exactly one frame
drawn in, against the float64 restatement (tests/apc_ref.py) FROM THE WAVEFORMS, scored per (state, utterance).  The fixtures of
tests/test_apc_gpu.py pin the released geometry against the reference itself; this guards the generality apc_check_config promises.

A one-frame utterance has no standard deviation over time (CMVN gives nan in torch, in the restatement and here alike), so the
seeds that draw one in run without CMVN."""

import functools

import numpy as np
import pytest

from oracle import encoder_oracle as O

import apc_ref as R

pytestmark = pytest.mark.gpu

FP32_TOL = 1e-4  # the suite's exact-fp32 bar
N_SEEDS = 24
WIDTHS = (64, 128, 192, 256)


def case_inputs(seed):
    """(cfg, lengths, waveforms, weights) of a sweep seed: widths, layer counts and the residual cycle so that every combination
    appears, the rest is drawn."""
    from s3prl_amd.config import apc_config
    from s3prl_amd.synth import synth_wavs, synth_weights

    rng = np.random.default_rng(9500 + seed)
    H = WIDTHS[seed % 4]
    layers = 3 + (seed // 4) % 2
    residual = bool((seed // 8) % 2)
    one_frame = seed % 3 == 0
    cfg = apc_config(H, layers, residual, cmvn=not one_frame)
    B = int(rng.integers(1, 5))
    lengths = [int(rng.integers(560, 6001)) for _ in range(B)]
    if one_frame:
        lengths[int(rng.integers(B))] = int(rng.choice([400, 559]))  # exactly one frame (alone in the batch: T = 1)
    wavs = synth_wavs(lengths, seed + 1, dc=float(rng.choice([0.0, 0.2])), scale=float(rng.choice([1.0, 0.1])))
    return cfg, lengths, wavs, synth_weights(cfg, 700 + seed)


@functools.lru_cache(maxsize=None)
def case(seed):
    cfg, lengths, wavs, weights = case_inputs(seed)
    return cfg, lengths, wavs, weights, R.forward(cfg, weights, wavs)


@pytest.mark.parametrize("seed", range(N_SEEDS))
def test_random_apc_matches_float64(seed):
    import torch

    from s3prl_amd.encoder import HipEncoder

    assert torch.cuda.is_available(), "these tests need the MI355X"
    cfg, lengths, wavs, weights, ref = case(seed)
    n_max = max(lengths)
    T, H, B = cfg.num_frames(n_max), cfg.conv_dim, len(wavs)
    valid = [cfg.valid_frames(n, n_max) for n in lengths]
    assert valid == ref["lengths"] and min(valid) >= 1
    dev = [torch.from_numpy(w).cuda() for w in wavs]
    enc = HipEncoder(cfg, weights)
    assert enc.num_states() == 3 == len(ref["hidden_states"])
    assert [enc.valid_frames(n, n_max) for n in lengths] == valid
    hs = enc.forward(dev).clone()
    torch.cuda.synchronize()
    assert tuple(hs.shape) == (3, B, T, H)
    got = hs.cpu().numpy()
    assert np.isfinite(got).all()
    worst = 0.0
    for l in range(3):
        for b, v in enumerate(valid):
            assert not got[l][b, v:].any(), (seed, l, b, "rows behind the length must be exactly 0")
            worst = max(worst, O.rel_err(got[l][b, :v], ref["hidden_states"][l][b, :v]))
    what = (f"seed {seed}: H {H} x {cfg.apc_layers} residual {cfg.apc_residual} cmvn {cfg.apc_cmvn} "
            f"gate std {['%.2f' % s for s in ref['gate_std']]}")
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
