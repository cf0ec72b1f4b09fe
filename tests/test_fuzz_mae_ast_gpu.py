"""Seeded sweep over what s3enc_create_mae_ast accepts — both released patch geometries and others of the kernel's set (an odd kt
among them), both LayerNorm orders, widths of 64 / 128 / 192, 1..3 layers, 1..4 utterances: equal, ragged, with a mask index that
reaches the token count — against the float64 restatement (tests/mae_ast_ref.py), scored per utterance.  The fixtures of
tests/test_mae_ast_gpu.py pin the family against the reference model itself; this guards the generality."""

import functools

import numpy as np
import pytest

from oracle import encoder_oracle as O

import mae_ast_ref as R

pytestmark = pytest.mark.gpu

FP32_TOL = 1e-4  # the suite's exact-fp32 bar
N_SEEDS = 20
GEOMETRIES = ((16, 16), (2, 128), (3, 32), (4, 64), (1, 16), (5, 128), (8, 32))


def case_inputs(seed):
    from s3prl_amd.config import mae_ast_config
    from s3prl_amd.synth import synth_wavs, synth_weights

    rng = np.random.default_rng(8800 + seed)
    kt, kc = GEOMETRIES[seed % len(GEOMETRIES)]
    heads = 1 + seed % 3
    cfg = mae_ast_config(kt=kt, kc=kc, embed_dim=64 * heads, layers=1 + (seed // 2) % 3, heads=heads, ffn=4 * int(rng.integers(16, 80)),
                         layer_norm_first=bool((seed // 3) % 2), max_token_length=1024)
    B = 1 + seed % 4
    steps = int(rng.integers(2, 9))                       # time steps of the longest utterance
    Fmax = steps * kt + int(rng.integers(0, kt))          # ... plus frames that no patch reads
    frames = [Fmax] + [int(rng.integers(1, Fmax + 1)) for _ in range(B - 1)]
    if seed % 4 == 1:
        frames = [Fmax] * B                               # an equal-length batch
    if seed % 4 == 2 and B > 1:
        frames[1] = (steps - 1) * kt + 1                  # shorter than the longest, and its mask index reaches Ttok
    lengths = [400 + 160 * (f - 1) + int(rng.integers(0, 160)) for f in frames]
    wavs = synth_wavs(lengths, seed + 1, dc=float(rng.choice([0.0, 0.1])), scale=float(rng.choice([1.0, 0.1])))
    return cfg, lengths, frames, wavs, synth_weights(cfg, 3900 + seed)


@functools.lru_cache(maxsize=None)
def case(seed):
    cfg, lengths, frames, wavs, weights = case_inputs(seed)
    return cfg, lengths, wavs, weights, R.forward(cfg, weights, wavs)


def test_the_sweep_covers_what_it_says():
    cases = [case_inputs(s) for s in range(N_SEEDS)]
    geo = {(c[0].ma_kt, c[0].ma_kc) for c in cases}
    assert {(16, 16), (2, 128)} <= geo and any(kt % 2 == 1 and kt > 1 for kt, _ in geo)
    assert {c[0].layer_norm_first for c in cases} == {True, False}
    assert {len(c[1]) for c in cases} == {1, 2, 3, 4}
    equal = [c for c in cases if len(c[1]) > 1 and len(set(c[2])) == 1]
    ragged = [c for c in cases if len(set(c[0].ma_key_counts(c[1]))) > 1]
    reach = [c for c in cases if any(f < max(c[2]) and -(-f // c[0].ma_kt) >= max(c[2]) // c[0].ma_kt for f in c[2])]
    assert equal and ragged and reach
    assert all(max(c[2]) == c[2][0] and min(c[2]) >= 1 for c in cases)


@pytest.mark.parametrize("seed", range(N_SEEDS))
def test_random_mae_ast_matches_float64(seed):
    import torch

    from s3prl_amd.encoder import HipEncoder

    assert torch.cuda.is_available(), "these tests need the MI355X"
    cfg, lengths, wavs, weights, ref = case(seed)
    Tt, width = cfg.num_frames(max(lengths)), cfg.ma_tokens_per_step * cfg.encoder_embed_dim
    dev = [torch.from_numpy(w).cuda() for w in wavs]
    enc = HipEncoder(cfg, weights)
    try:
        hs = enc.forward(dev).clone()
        torch.cuda.synchronize()
        assert tuple(hs.shape) == (cfg.encoder_layers, len(wavs), Tt, width) == (cfg.encoder_layers,) + ref["states"][0].shape
        got = hs.cpu().numpy()
        assert np.isfinite(got).all()
        errs = [O.rel_err(got[l][b], ref["states"][l][b]) for l in range(cfg.encoder_layers) for b in range(len(wavs))]
        what = (f"seed {seed}: ({cfg.ma_kt}, {cfg.ma_kc}) D {cfg.encoder_embed_dim} layers {cfg.encoder_layers} "
                f"pre-LN {cfg.layer_norm_first} lengths {lengths} steps {Tt} keys {ref['kv']}")
        print(f"{what}: worst per-utterance rel-err {max(errs):.2e}")
        assert max(errs) < FP32_TOL, (what, errs)
        assert [enc.valid_frames(n, max(lengths)) * cfg.ma_tokens_per_step for n in lengths] == ref["kv"]
        assert enc.status() == 0
        perm = [int(i) for i in np.random.default_rng(seed).permutation(len(wavs))]
        permuted = enc.forward([dev[i] for i in perm]).clone()
        torch.cuda.synchronize()
        for j, i in enumerate(perm):
            assert O.rel_err(permuted[:, j].cpu().numpy(), got[:, i]) < FP32_TOL, (what, "permuted", j, i)
    finally:
        enc.close()
