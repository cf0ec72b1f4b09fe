"""Seeded sweep over what s3enc_create_byol_s accepts — both networks, block counts of 1 and 2 per layer, windows from a quarter of a
second (frame counts odd at several levels) to one second, hops below and above the window's half, 1..4 ragged utterances from one
sample to several windows — against the float64 restatement (tests/byol_s_ref.py), scored per utterance.  The restatement is given
the batch's two statistics from the GPU's debug tap (they are checked on their own in tests/test_byol_s_frontend_gpu.py), so a window
row is scored on its own samples: an error of the network cannot hide behind, or be blamed on, a difference in the statistics.  The
fixtures of tests/test_byol_s_gpu.py pin the family against the reference itself; this guards the generality."""

import functools

import numpy as np
import pytest

from oracle import encoder_oracle as O

import byol_s_ref as R

pytestmark = pytest.mark.gpu

FP32_TOL = 1e-4  # the suite's exact-fp32 bar
N_SEEDS = 12
# seconds: 26 frames (-> 13 -> 7 -> 4 -> 2), 41 (-> 21 -> 11 -> 6 -> 3), 51 (-> 26 -> 13 -> 7 -> 4), 77, 101
WINDOWS = (0.25, 0.4, 0.5, 0.76, 1.0)
HOPS = (0.05, 0.11, 0.2, 0.3)


def case_inputs(seed):
    from s3prl_amd.config import byol_s_config
    from s3prl_amd.synth import synth_wavs, synth_weights

    rng = np.random.default_rng(8800 + seed)
    network = "default" if seed % 4 == 3 else "resnetish"
    blocks = tuple(int(b) for b in rng.integers(1, 3, size=4))
    cfg = byol_s_config(network, blocks, window_secs=WINDOWS[seed % len(WINDOWS)], hop_secs=HOPS[seed % len(HOPS)])
    _, window, step = cfg.conv_layers[0]
    B = 1 + seed % 4
    lengths = [int(rng.integers(1, 5 * step)) for _ in range(B)]
    if seed % 5 == 0:
        lengths[0] = int(rng.integers(1, 4)) * step  # exactly k * step
    if seed % 5 == 1:
        lengths[-1] = int(rng.integers(1, 4)) * step + 1
    wavs = synth_wavs(lengths, seed + 1, dc=float(rng.choice([0.0, 0.1])), scale=float(rng.choice([1.0, 0.1])))
    return cfg, lengths, wavs, synth_weights(cfg, 3900 + seed)


def test_the_sweep_covers_what_it_says():
    cases = [case_inputs(s) for s in range(N_SEEDS)]
    assert {c[0].bs_network for c in cases} == {"default", "resnetish"}
    assert {b for c in cases if c[0].bs_network == "resnetish" for b in c[0].bs_blocks} == {1, 2}
    assert {c[0].bs_window_secs for c in cases} == set(WINDOWS) and {c[0].bs_hop_secs for c in cases} == set(HOPS)
    assert {len(c[1]) for c in cases} == {1, 2, 3, 4}
    assert any(min(c[1]) < c[0].conv_layers[0][2] for c in cases) and any(len(set(c[1])) > 1 for c in cases)


@functools.lru_cache(maxsize=None)
def case(seed):
    return case_inputs(seed)


@pytest.mark.parametrize("seed", range(N_SEEDS))
def test_random_byol_s_matches_float64(seed):
    import torch

    from s3prl_amd.encoder import HipEncoder

    assert torch.cuda.is_available(), "these tests need the MI355X"
    cfg, lengths, wavs, weights = case(seed)
    _, window, step = cfg.conv_layers[0]
    S = cfg.num_frames(max(lengths))
    dev = [torch.from_numpy(w).cuda() for w in wavs]
    enc = HipEncoder(cfg, weights)
    try:
        hs = enc.forward(dev).clone()
        torch.cuda.synchronize()
        stats = enc.debug_tap("stats").astype(np.float64)
        assert tuple(hs.shape) == (1, len(wavs), S, 2048)
        got = hs[0].cpu().numpy()
        assert np.isfinite(got).all() and enc.status() == 0
    finally:
        enc.close()
    ref = R.forward(cfg, weights, wavs, stats=(float(stats[0]), float(stats[1])))
    own = np.array(ref["stats"])
    assert np.abs(stats - own).max() <= 2e-6 * np.abs(own).min(), (stats, own)
    errs = [O.rel_err(got[b], ref["state"][b]) for b in range(len(wavs))]
    rows = [O.rel_err(got[b, s], ref["state"][b, s]) for b in range(len(wavs)) for s in range(S)]
    what = f"seed {seed}: {cfg.bs_network} {cfg.bs_blocks} window {window} step {step} lengths {lengths} windows {S}"
    print(f"{what}: worst per-utterance rel-err {max(errs):.2e}, worst window row {max(rows):.2e}")
    assert max(errs) < FP32_TOL and max(rows) < FP32_TOL, (what, errs, max(rows))
