"""Seeded sweep over what s3enc_create_ssast accepts — both released geometries, widths of 64 / 128 / 192 (the checkpoint's tiny
width among them), 1..3 blocks, window_secs from 0.2 to 1.0, 1..4 utterances whose longest is just below, at or just above a whole
number of windows, some shorter than one analysis window, the pretraining grid on either side of t_dim — against the float64
restatement (tests/ssast_ref.py), scored per utterance.  The fixtures of tests/test_ssast_gpu.py pin the family to recorded states;
this guards the generality."""

import functools

import numpy as np
import pytest

from oracle import encoder_oracle as O

import ssast_ref as R

pytestmark = pytest.mark.gpu

FP32_TOL = 1e-4  # the suite's exact-fp32 bar
N_SEEDS = 16
WINDOWS = (0.5, 0.2, 1.0, 0.33, 0.25)  # 8000, 3200, 16000, 5280, 4000 samples: multiples of 4


def case_inputs(seed):
    from s3prl_amd.config import ssast_config
    from s3prl_amd.synth import synth_wavs, synth_weights

    rng = np.random.default_rng(9900 + seed)
    mtype = "pf"[seed % 2]
    heads = 1 + (seed // 2) % 3
    secs = WINDOWS[seed % len(WINDOWS)]
    t_probe = ssast_config(model_type=mtype, embed_dim=64, heads=1, layers=1, window_secs=secs).ss_t_dim
    tshape = 16 if mtype == "p" else 2
    p_t = [max(1, t_probe - 1), t_probe, t_probe + 3][(seed // 4) % 3]  # the pretraining grid below, at and above t_dim
    cfg = ssast_config(model_type=mtype, embed_dim=64 * heads, heads=heads, layers=1 + (seed // 3) % 3, ffn=4 * int(rng.integers(16, 80)),
                       window_secs=secs, p_input_tdim=p_t * tshape)
    W = cfg.ss_window_samples
    B = 1 + seed % 4
    k = int(rng.integers(1, 4))
    longest = k * W + (-1, 0, 1, int(rng.integers(2, W)))[seed % 4] if not (k == 1 and seed % 4 == 0) else W - 1
    lengths = [longest] + [int(rng.integers(1, longest + 1)) for _ in range(B - 1)]
    if seed % 5 == 3 and B > 1:
        lengths[1] = int(rng.integers(1, 400))  # shorter than one analysis window
    wavs = synth_wavs(lengths, seed + 1, dc=float(rng.choice([0.0, 0.1])), scale=float(rng.choice([1.0, 0.1])))
    return cfg, lengths, wavs, synth_weights(cfg, 4900 + seed)


@functools.lru_cache(maxsize=None)
def case(seed):
    cfg, lengths, wavs, weights = case_inputs(seed)
    return cfg, lengths, wavs, weights, R.forward(cfg, weights, wavs)["states"]


def test_the_sweep_covers_what_it_says():
    cases = [case_inputs(s) for s in range(N_SEEDS)]
    assert {c[0].ss_fshape for c in cases} == {16, 128} and {c[0].encoder_embed_dim for c in cases} == {64, 128, 192}
    assert {len(c[1]) for c in cases} == {1, 2, 3, 4} and len({c[0].ss_window_secs for c in cases}) >= 4
    rel = {np.sign(c[0].ss_pretrain_grid[1] - c[0].ss_t_dim) for c in cases}
    assert rel == {-1, 0, 1}
    assert any(min(c[1]) < 400 for c in cases)
    assert any(c[0].num_frames(max(c[1])) < c[0].ss_num_windows(max(c[1])) * c[0].ss_t_dim for c in cases)  # the cut binds
    assert any(max(c[1]) % c[0].ss_window_samples == 0 for c in cases) and any(max(c[1]) % c[0].ss_window_samples == 1 for c in cases)


@pytest.mark.parametrize("seed", range(N_SEEDS))
def test_random_ssast_matches_float64(seed):
    import torch

    from s3prl_amd.encoder import HipEncoder

    assert torch.cuda.is_available(), "these tests need the MI355X"
    cfg, lengths, wavs, weights, ref = case(seed)
    T, width = cfg.num_frames(max(lengths)), cfg.ss_f_dim * cfg.encoder_embed_dim
    dev = [torch.from_numpy(w).cuda() for w in wavs]
    enc = HipEncoder(cfg, weights)
    try:
        hs = enc.forward(dev).clone()
        torch.cuda.synchronize()
        assert tuple(hs.shape) == (cfg.encoder_layers, len(wavs), T, width) == (cfg.encoder_layers,) + ref[0].shape
        got = hs.cpu().numpy()
        assert np.isfinite(got).all()
        errs = [O.rel_err(got[l][b], ref[l][b]) for l in range(cfg.encoder_layers) for b in range(len(wavs))]
        what = (f"seed {seed}: ({cfg.ss_fshape}, {cfg.ss_tshape}) D {cfg.encoder_embed_dim} layers {cfg.encoder_layers} window "
                f"{cfg.ss_window_secs} s grid {cfg.ss_pretrain_grid} -> {(cfg.ss_f_dim, cfg.ss_t_dim)} lengths {lengths} rows {T}")
        print(f"{what}: worst per-utterance rel-err {max(errs):.2e}")
        assert max(errs) < FP32_TOL, (what, errs)
        assert [enc.valid_frames(n, max(lengths)) for n in lengths] == [cfg.valid_frames(n, max(lengths)) for n in lengths]
        perm = [int(i) for i in np.random.default_rng(seed).permutation(len(wavs))]
        permuted = enc.forward([dev[i] for i in perm]).clone()
        torch.cuda.synchronize()
        for j, i in enumerate(perm):  # windows are independent sequences: an utterance's rows are its bits at any place in the batch
            assert np.array_equal(permuted[:, j].cpu().numpy(), got[:, i]), (what, "permuted", j, i)
    finally:
        enc.close()
