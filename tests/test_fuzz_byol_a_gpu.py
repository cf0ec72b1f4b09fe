"""Seeded sweep over what s3enc_create_byol_a accepts — feature_d of 64 / 128 / 512, windows from the shortest legal one (1120
samples, 8 frames) to 1.2 s with frame counts odd at every pooling level among them, strides below, at and above the window, 1..4
ragged utterances from one sample to several windows — against the float64 restatement (tests/byol_a_ref.py), scored per utterance.
The fixtures of tests/test_byol_a_gpu.py pin the family against the reference itself; this guards the generality."""

import functools

import numpy as np
import pytest

from oracle import encoder_oracle as O

import byol_a_ref as R

pytestmark = pytest.mark.gpu

FP32_TOL = 1e-4  # the suite's exact-fp32 bar
N_SEEDS = 20
DIMS = (64, 128, 512)
# seconds: 1120 samples (8 frames -> 4 -> 2 -> 1), 11 frames (-> 5 -> 2 -> 1), 26 frames (-> 13 -> 6 -> 3), 51, 77, 101, 121 frames
WINDOWS = (0.07, 0.1, 0.25, 0.5, 0.76, 1.0, 1.2)


def case_inputs(seed):
    from s3prl_amd.config import byol_a_config
    from s3prl_amd.synth import synth_wavs, synth_weights

    rng = np.random.default_rng(7700 + seed)
    d = DIMS[seed % 3]
    window_secs = WINDOWS[seed % len(WINDOWS)]
    stride_secs = round(window_secs * float((0.4, 1.0, 1.5, 0.75)[(seed // 3) % 4]), 3)
    cfg = byol_a_config(d, window_secs=window_secs, stride_secs=stride_secs)
    _, window, stride = cfg.conv_layers[0]
    B = 1 + seed % 4
    lengths = [int(rng.integers(1, 4 * max(window, stride))) for _ in range(B)]
    if seed % 5 == 0:
        lengths[0] = int(rng.integers(1, 4)) * stride  # exactly k * stride
    if seed % 5 == 1:
        lengths[-1] = int(rng.integers(1, 4)) * stride + 1
    reach = (-(-max(lengths) // stride) - 1) * stride + window  # starts[-1] + window: what the reference pads every utterance to
    lengths = [min(n, reach) for n in lengths]  # stride > window: the reference raises on a longer utterance (negative padding)
    wavs = synth_wavs(lengths, seed + 1, dc=float(rng.choice([0.0, 0.1])), scale=float(rng.choice([1.0, 0.1])))
    return cfg, lengths, wavs, synth_weights(cfg, 2900 + seed)


@functools.lru_cache(maxsize=None)
def case(seed):
    cfg, lengths, wavs, weights = case_inputs(seed)
    return cfg, lengths, wavs, weights, R.forward(cfg, weights, wavs)["state"]


def test_the_sweep_covers_what_it_says():
    cases = [case_inputs(s) for s in range(N_SEEDS)]
    assert {c[0].conv_layers[0][0] for c in cases} == set(DIMS)
    assert {c[0].ba_window_secs for c in cases} == set(WINDOWS)
    rel = [c[0].conv_layers[0][2] / c[0].conv_layers[0][1] for c in cases]
    assert min(rel) < 0.5 and max(rel) > 1.2 and any(abs(r - 1.0) < 1e-3 for r in rel)
    assert {len(c[1]) for c in cases} == {1, 2, 3, 4}
    assert any(min(c[1]) < c[0].conv_layers[0][1] for c in cases)


@pytest.mark.parametrize("seed", range(N_SEEDS))
def test_random_byol_a_matches_float64(seed):
    import torch

    from s3prl_amd.encoder import HipEncoder

    assert torch.cuda.is_available(), "these tests need the MI355X"
    cfg, lengths, wavs, weights, ref = case(seed)
    d, window, stride = cfg.conv_layers[0]
    S = cfg.num_frames(max(lengths))
    dev = [torch.from_numpy(w).cuda() for w in wavs]
    enc = HipEncoder(cfg, weights)
    try:
        hs = enc.forward(dev).clone()
        torch.cuda.synchronize()
        assert tuple(hs.shape) == (1, len(wavs), S, d) == (1,) + ref.shape
        got = hs[0].cpu().numpy()
        assert np.isfinite(got).all()
        errs = [O.rel_err(got[b], ref[b]) for b in range(len(wavs))]
        what = f"seed {seed}: d {d} window {window} stride {stride} lengths {lengths} segments {S}"
        print(f"{what}: worst per-utterance rel-err {max(errs):.2e}")
        assert max(errs) < FP32_TOL, (what, errs)
        assert enc.status() == 0
        perm = [int(i) for i in np.random.default_rng(seed).permutation(len(wavs))]
        permuted = enc.forward([dev[i] for i in perm]).clone()
        torch.cuda.synchronize()
        for j, i in enumerate(perm):
            assert torch.equal(permuted[:, j], hs[:, i]), (what, "permuted", j, i)
    finally:
        enc.close()
