"""Seeded sweep over the Mockingjay / TERA / AudioALBERT configurations s3enc_create_mockingjay accepts — 1 to 4 layers, hidden sizes
128 / 192 / 768, 16 / 40 / 80 mel bins, sequence_length 0 / 7 / 16 (no chunking, many short chunks, two or three chunks), with and
without layer sharing — on ragged batches of 1..4 utterances between 201 and 6000 samples, against the float64 restatement
(tests/mockingjay_ref.py) FROM THE WAVEFORMS, scored per (state, utterance) on the live rows.  The fixtures of
tests/test_mockingjay_gpu.py pin the released geometry against the reference itself; this guards the generality mj_check_config
promises.

An utterance that is a single frame inside its batch has no standard deviation for the CMVN (nan in torch, refused here): such a
draw is redrawn."""

import functools

import numpy as np
import pytest

from oracle import encoder_oracle as O

import mockingjay_ref as R

pytestmark = pytest.mark.gpu

FP32_TOL = 1e-4  # the suite's exact-fp32 bar
N_SEEDS = 16
WIDTHS = (128, 192, 768)
MELS = (16, 40, 80)
SEQ = (0, 7, 16)


def case_inputs(seed):
    """(cfg, lengths, waveforms, weights) of a sweep seed: widths, chunk lengths and sharing cycle so that every value appears, the
    rest is drawn."""
    from s3prl_amd.config import mockingjay_config
    from s3prl_amd.synth import synth_wavs, synth_weights

    rng = np.random.default_rng(9700 + seed)
    D = WIDTHS[seed % 3]
    layers = 1 + int(rng.integers(0, 4)) if D < 768 else 1 + seed % 2  # (the wide ones stay shallow: test time)
    cfg = mockingjay_config(D, layers, D // 64, 2 * D, MELS[(seed // 3) % 3], "mel", SEQ[(seed // 2) % 3], share_layer=bool(seed % 2))
    while True:
        B = int(rng.integers(1, 5))
        lengths = [int(rng.integers(201, 6001)) for _ in range(B)]
        if min(R.frame_counts(lengths)) >= 2:
            break
    wavs = synth_wavs(lengths, seed + 1, dc=float(rng.choice([0.0, 0.2])), scale=float(rng.choice([1.0, 0.1])))
    return cfg, lengths, wavs, synth_weights(cfg, 800 + seed)


@functools.lru_cache(maxsize=None)
def case(seed):
    cfg, lengths, wavs, weights = case_inputs(seed)
    return cfg, lengths, wavs, weights, R.forward(cfg, weights, wavs)


@pytest.mark.parametrize("seed", range(N_SEEDS))
def test_random_mockingjay_matches_float64(seed):
    import torch

    from s3prl_amd.encoder import HipEncoder

    assert torch.cuda.is_available(), "these tests need the MI355X"
    cfg, lengths, wavs, weights, ref = case(seed)
    n_max = max(lengths)
    T, D, B, NS = cfg.num_frames(n_max), cfg.encoder_embed_dim, len(wavs), cfg.encoder_layers + 1
    valid = [cfg.valid_frames(n, n_max) for n in lengths]
    assert valid == ref["lengths"] and min(valid) >= 2
    dev = [torch.from_numpy(w).cuda() for w in wavs]
    enc = HipEncoder(cfg, weights)
    assert enc.num_states() == NS == len(ref["hidden_states"])
    assert [enc.valid_frames(n, n_max) for n in lengths] == valid
    hs = enc.forward(dev).clone()
    torch.cuda.synchronize()
    assert tuple(hs.shape) == (NS, B, T, D)
    got = hs.cpu().numpy()
    assert np.isfinite(got).all()  # padding rows included
    worst = 0.0
    for l in range(NS):
        for b, v in enumerate(valid):
            worst = max(worst, O.rel_err(got[l][b, :v], ref["hidden_states"][l][b, :v]))
    what = (f"seed {seed}: D {D} x {cfg.encoder_layers} mels {cfg.mj_input_dim} seq {cfg.mj_sequence_length} "
            f"chunks {R.chunk_sizes(T, cfg.mj_sequence_length)} share {cfg.mj_share_layer}")
    print(f"{what} lengths {lengths} frames {valid}: worst per-(state, utterance) rel-err {worst:.2e}")
    assert worst < FP32_TOL, (what, lengths, worst)
    assert enc.status() == 0
    enc.close()
