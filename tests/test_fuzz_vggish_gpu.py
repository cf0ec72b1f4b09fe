"""Seeded sweep over the VGGish configurations s3enc_create_vggish accepts — 1..6 conv layers of 16..192 channels with 0..3 pools
placed anywhere, examples of 8..32 frames by 8..32 bands, Linear widths 32..256, with and without the post-processor — on ragged
batches of 1..4 utterances holding 1..7 examples each, the shortest legal utterance drawn in, against the float64 restatement
(tests/vggish_ref.py) FROM THE WAVEFORMS, scored per utterance.  The fixtures of tests/test_vggish_gpu.py pin the released geometry
against the reference itself; this guards the generality vggish_check_config promises."""

import functools

import numpy as np
import pytest

from oracle import encoder_oracle as O

import vggish_ref as R

pytestmark = pytest.mark.gpu

FP32_TOL = 1e-4   # the suite's exact-fp32 bar
HALF_BAND = 0.02  # tests/test_vggish_gpu.py's band around the float64 pre-rounding value
N_SEEDS = 24
CHANNELS = (16, 32, 48, 64, 96, 128, 192)


def case_inputs(seed):
    """(cfg, lengths, waveforms, weights) of a sweep seed: the layer count, the pool count and the post-processor cycle so that
    every value appears with every other, the rest is drawn."""
    from s3prl_amd.config import vggish_config
    from s3prl_amd.synth import synth_wavs, synth_weights

    rng = np.random.default_rng(9900 + seed)
    n_layers = 1 + seed % 6
    pools = min((seed // 2) % 4, n_layers)
    where = set(int(i) for i in rng.choice(n_layers, size=pools, replace=False))
    layers = [(int(rng.choice(CHANNELS)), i in where) for i in range(n_layers)]
    div = 1 << pools
    frames = div * int(rng.integers(max(1, 8 // div), 32 // div + 1))
    bands = div * int(rng.integers(max(1, 8 // div), 32 // div + 1))
    fc = tuple(int(4 * rng.integers(8, 65)) for _ in range(3))
    cfg = vggish_config(layers=layers, fc=fc, example_frames=frames, num_mel_bins=bands, postprocess=bool((seed // 3) % 2))
    m, hop = cfg.vg_min_samples, frames * 160
    B = int(rng.integers(1, 5))
    lengths = [m + int(rng.integers(0, 7 * hop)) for _ in range(B)]
    if seed % 4 == 0:
        lengths[int(rng.integers(B))] = m  # the shortest legal utterance
    wavs = synth_wavs(lengths, seed + 1, dc=float(rng.choice([0.0, 0.2])), scale=float(rng.choice([1.0, 0.1])))
    return cfg, lengths, wavs, synth_weights(cfg, 1900 + seed)


@functools.lru_cache(maxsize=None)
def case(seed):
    cfg, lengths, wavs, weights = case_inputs(seed)
    return cfg, lengths, wavs, weights, R.forward(cfg, weights, wavs)


def test_the_sweep_covers_what_it_says():
    cfgs = [case_inputs(s)[0] for s in range(N_SEEDS)]
    assert {len(c.vg_layers) for c in cfgs} == {1, 2, 3, 4, 5, 6} and {c.vg_pools for c in cfgs} == {0, 1, 2, 3}
    assert {c.vg_postprocess for c in cfgs} == {True, False}
    assert any(ch % 64 for c in cfgs for ch, _ in c.vg_layers) and any(ch > 128 for c in cfgs for ch, _ in c.vg_layers)
    assert any(c.vg_layers[-1][1] for c in cfgs) and any(not c.vg_layers[-1][1] for c in cfgs)
    assert any(min(case_inputs(s)[1]) == case_inputs(s)[0].vg_min_samples for s in range(N_SEEDS))


@pytest.mark.parametrize("seed", range(N_SEEDS))
def test_random_vggish_matches_float64(seed):
    import torch

    from s3prl_amd.encoder import HipEncoder

    assert torch.cuda.is_available(), "these tests need the MI355X"
    cfg, lengths, wavs, weights, ref = case(seed)
    n_max = max(lengths)
    E, D, B = cfg.num_frames(n_max), cfg.vg_fc[2], len(wavs)
    counts = [cfg.valid_frames(n, n_max) for n in lengths]
    assert counts == ref["counts"] and min(counts) >= 1
    dev = [torch.from_numpy(w).cuda() for w in wavs]
    enc = HipEncoder(cfg, weights)
    assert enc.num_states() == 1 and [enc.valid_frames(n, n_max) for n in lengths] == counts
    hs = enc.forward(dev).clone()
    torch.cuda.synchronize()
    assert tuple(hs.shape) == (1, B, E, D)
    got = hs[0].cpu().numpy()
    assert np.isfinite(got).all()
    what = (f"seed {seed}: {cfg.vg_example_frames} x {cfg.vg_num_mel_bins} layers {cfg.vg_layers} fc {cfg.vg_fc} "
            f"postprocess {cfg.vg_postprocess}")
    emb = enc.debug_tap("emb").reshape(sum(counts), D)
    o, worst = 0, 0.0
    for b, n in enumerate(counts):
        worst = max(worst, O.rel_err(emb[o:o + n], ref["emb"][b, :n]))
        assert not got[b, n:].any(), (what, "pad rows", b)
        o += n
    print(f"{what} lengths {lengths} examples {counts}: worst per-utterance rel-err of the embedding {worst:.2e}")
    assert worst < FP32_TOL, (what, lengths, worst)
    if cfg.vg_postprocess:
        assert np.array_equal(got, np.rint(got)) and got.min() >= 0 and got.max() <= 255
        for b, n in enumerate(counts):
            assert np.abs(got[b, :n] - ref["pre"][b, :n]).max() <= 0.5 + HALF_BAND, (what, b)
    else:
        o = 0
        for b, n in enumerate(counts):
            assert np.array_equal(got[b, :n], emb[o:o + n])
            o += n
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
