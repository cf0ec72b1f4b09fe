"""Seeded sweep over the modified-CPC configurations s3enc_create_cpc accepts — widths 64..256 (every channel-norm template and
both row-per-thread classes of the recurrent kernel), LSTM and GRU, 1..3 recurrent layers — on ragged batches of 1..4 utterances
between 159 and 6000 samples against the float64 restatement (tests/cpc_ref.py), scored per (state, utterance).  The fixtures of
tests/test_cpc_gpu.py pin the released geometry against the reference itself; this guards the generality cpc_check_config promises."""

import functools

import numpy as np
import pytest

from oracle import encoder_oracle as O

import cpc_ref as R

pytestmark = pytest.mark.gpu

FP32_TOL = 1e-4  # the suite's exact-fp32 bar
N_SEEDS = 24
WIDTHS = (64, 128, 192, 256)


def case_inputs(seed):
    """(cfg, lengths, waveforms, weights) of a sweep seed: the widths, cells and layer counts cycle so that every combination of
    width and cell appears, the rest is drawn."""
    from s3prl_amd.config import cpc_config
    from s3prl_amd.synth import synth_wavs, synth_weights

    rng = np.random.default_rng(9000 + seed)
    C = WIDTHS[seed % 4]
    cell = ("LSTM", "GRU")[(seed // 4) % 2]
    layers = 1 + (seed // 8) % 3
    cfg = cpc_config(C, cell, layers)
    B = int(rng.integers(1, 5))
    lengths = [int(rng.integers(159, 6001)) for _ in range(B)]
    if seed % 3 == 0:
        lengths[int(rng.integers(B))] = 159  # an utterance of exactly one frame (alone in the batch: T = 1)
    wavs = synth_wavs(lengths, seed + 1, dc=float(rng.choice([0.0, 0.2])), scale=float(rng.choice([1.0, 0.1])))
    return cfg, lengths, wavs, synth_weights(cfg, 300 + seed)


@functools.lru_cache(maxsize=None)
def case(seed):
    cfg, lengths, wavs, weights = case_inputs(seed)
    return cfg, lengths, wavs, weights, R.forward(cfg, weights, wavs)


def per_utterance_errors(got, ref, valid):
    """worst rel-err over (state, utterance): every utterance's row, and its own frames alone — a short utterance does not hide
    behind a long one, nor behind the frames of its own padding"""
    worst = 0.0
    for l in range(len(ref)):
        for b, v in enumerate(valid):
            worst = max(worst, O.rel_err(got[l][b], ref[l][b]))
            if v:
                worst = max(worst, O.rel_err(got[l][b, :v], ref[l][b, :v]))
    return worst


@pytest.mark.parametrize("seed", range(N_SEEDS))
def test_random_cpc_matches_float64(seed):
    import torch

    from s3prl_amd.encoder import HipEncoder

    assert torch.cuda.is_available(), "these tests need the MI355X"
    cfg, lengths, wavs, weights, ref = case(seed)
    n_max = max(lengths)
    T, C, B = cfg.num_frames(n_max), cfg.conv_dim, len(wavs)
    valid = [cfg.valid_frames(n, n_max) for n in lengths]
    dev = [torch.from_numpy(w).cuda() for w in wavs]
    enc = HipEncoder(cfg, weights)
    assert enc.num_states() == 2 == len(ref["hidden_states"])
    assert [enc.num_frames(n) for n in lengths] == [cfg.num_frames(n) for n in lengths] and min(valid) >= 1
    assert [enc.valid_frames(n, n_max) for n in lengths] == valid
    hs = enc.forward(dev).clone()
    torch.cuda.synchronize()
    assert tuple(hs.shape) == (2, B, T, C)
    got = hs.cpu().numpy()
    assert np.isfinite(got).all()
    err = per_utterance_errors(got, ref["hidden_states"], valid)
    what = f"seed {seed}: C {C} {cfg.ar_mode} x {cfg.ar_layers} gate std {['%.2f' % s for s in ref['gate_std']]}"
    print(f"{what} lengths {lengths} T {T}: worst per-(state, utterance) rel-err {err:.2e}")
    assert err < FP32_TOL, (what, lengths, err)
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
    assert other.status() == 0
    enc.close()
    other.close()
