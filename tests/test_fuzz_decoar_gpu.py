"""Seeded sweep over the DeCoAR configurations s3enc_create_decoar accepts — hidden sizes 64..320, one to four LSTM layers per
direction, one state or one per layer, every or every second frame — on ragged batches of 1..5 utterances between 560 and 6000
samples, with utterances of exactly two fbank frames drawn in, against the float64 restatement (tests/decoar_ref.py) FROM THE
WAVEFORMS, scored per (state, utterance).  The fixtures of tests/test_decoar_gpu.py pin the model against the reference itself; this
guards the generality decoar_check_config promises."""

import functools

import numpy as np
import pytest

from oracle import encoder_oracle as O

import decoar_ref as R

pytestmark = pytest.mark.gpu

FP32_TOL = 1e-4  # the suite's exact-fp32 bar
N_SEEDS = 16
WIDTHS = (64, 128, 192, 320)


def case_inputs(seed):
    """(cfg, lengths, waveforms, weights) of a sweep seed: widths, layer counts, the state list and the subsampling cycle so that
    every value appears, the rest is drawn."""
    from s3prl_amd.config import decoar_config
    from s3prl_amd.synth import synth_wavs, synth_weights

    rng = np.random.default_rng(9700 + seed)
    H = WIDTHS[seed % 4]
    layers = 1 + (seed // 4) % 4
    cfg = decoar_config(H, layers, per_layer=bool(seed % 2), subsample=1 + (seed // 2) % 2)
    B = int(rng.integers(1, 6))
    lengths = [int(rng.integers(560, 6001)) for _ in range(B)]
    if seed % 3 == 0:
        lengths[int(rng.integers(B))] = int(rng.choice([560, 719]))  # exactly two fbank frames
    wavs = synth_wavs(lengths, seed + 1, dc=float(rng.choice([0.0, 0.2])), scale=float(rng.choice([1.0, 0.1])))
    return cfg, lengths, wavs, synth_weights(cfg, 800 + seed)


@functools.lru_cache(maxsize=None)
def case(seed):
    cfg, lengths, wavs, weights = case_inputs(seed)
    return cfg, lengths, wavs, weights, R.forward(cfg, weights, wavs)


@pytest.mark.parametrize("seed", range(N_SEEDS))
def test_random_decoar_matches_float64(seed):
    import torch

    from s3prl_amd.encoder import HipEncoder

    assert torch.cuda.is_available(), "these tests need the MI355X"
    cfg, lengths, wavs, weights, ref = case(seed)
    n_max = max(lengths)
    T, D, B, NS = cfg.num_frames(n_max), 2 * cfg.decoar_hidden, len(wavs), cfg.num_hidden_states
    valid = [cfg.valid_frames(n, n_max) for n in lengths]
    assert valid == ref["lengths"] and min(valid) >= 1
    dev = [torch.from_numpy(w).cuda() for w in wavs]
    enc = HipEncoder(cfg, weights)
    assert enc.num_states() == NS == len(ref["hidden_states"])
    assert [enc.valid_frames(n, n_max) for n in lengths] == valid
    hs = enc.forward(dev).clone()
    torch.cuda.synchronize()
    assert tuple(hs.shape) == (NS, B, T, D)
    got = hs.cpu().numpy()
    assert np.isfinite(got).all()
    worst = 0.0
    for l in range(NS):
        for b, v in enumerate(valid):
            assert not got[l][b, v:].any(), (seed, l, b, "rows behind the length must be exactly 0")
            worst = max(worst, O.rel_err(got[l][b, :v], ref["hidden_states"][l][b, :v]))
    what = (f"seed {seed}: H {cfg.decoar_hidden} x {cfg.decoar_layers} per_layer {cfg.decoar_per_layer} subsample {cfg.decoar_subsample} "
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
