"""Seeded sweep of the DeCoAR 2.0 path against the float64 restatement (tests/decoar2_ref.py, held to the reference's own fixtures by
tests/test_decoar2_cpu.py): embed_dim, the positional conv's groups (group widths 24 .. 64) and kernel (odd and even), FFN width,
layer count, batch size 1-4 and lengths from two fbank frames (one model frame) to about 1.5 s.  Per utterance and state rel_err <
5e-5 (tests/test_lighthubert_gpu.py's oracle band), over ALL rows of the utterance: the padded rows are defined values here.  No case
is skipped: every drawn configuration is one the path builds."""

import zlib

import numpy as np
import pytest

import decoar2_ref as R
from oracle import encoder_oracle as O
from test_encoder_gpu import _encoder, _run
from test_lighthubert_gpu import ORACLE_TOL

pytestmark = pytest.mark.gpu

N_CASES = 12
SHAPES = ((128, 4), (128, 2), (192, 4), (192, 8), (256, 8), (320, 8), (384, 8), (256, 4))  # (embed_dim, groups): widths 32 64 48 24 32 40 48 64


def _case(i):
    from s3prl_amd.config import decoar2_config

    rng = np.random.default_rng(zlib.crc32(f"fuzz/decoar2/{i}".encode()))
    D, G = SHAPES[i % len(SHAPES)]  # every group width occurs whatever the draws are
    K = int(rng.integers(3, 65)) if i % 3 else (16, 31, 128, 16)[i // 3]  # the tiny, an odd and the released kernel occur
    cfg = decoar2_config(D, int(rng.choice([D, 2 * D, 4 * D])), 1 + i % 3, K, G)
    B = 1 + i % 4
    lengths = [int(x) for x in rng.integers(560, 24000, size=B)]
    if i % 3 == 0:
        lengths[-1] = int(rng.integers(560, 720))  # two fbank frames, ONE model frame: beside longer ones, or alone
    return cfg, lengths, int(rng.integers(1 << 16))


@pytest.mark.parametrize("i", range(N_CASES))
def test_fuzz_against_the_restatement(i):
    from s3prl_amd.synth import synth_wavs, synth_weights

    cfg, lengths, seed = _case(i)
    NS = cfg.encoder_layers + 1
    weights = synth_weights(cfg, seed, ("synthetic", "pretrained_like")[i % 2])
    wavs = synth_wavs(lengths, seed + 1)
    ref = R.forward(cfg, weights, wavs)
    enc = _encoder(cfg, weights)
    try:
        hs = _run(enc, wavs)
        assert enc.status() == 0
        assert [enc.num_frames(n) for n in lengths] == [R.num_frames(n) for n in lengths]
    finally:
        enc.close()
    assert hs.shape == (NS,) + ref[0].shape and np.isfinite(hs).all()
    errs = [O.rel_err(hs[l][b], ref[l][b]) for l in range(NS) for b in range(len(wavs))]
    print(f"D2FUZZ case {i}: D={cfg.encoder_embed_dim} G={cfg.conv_pos_groups} K={cfg.conv_pos} F={cfg.encoder_ffn_embed_dim} "
          f"layers={cfg.encoder_layers} lengths={lengths} frames={[R.num_frames(n) for n in lengths]} worst={max(errs):.2e}")
    assert max(errs) < ORACLE_TOL, (i, lengths, ["%.2e" % e for e in errs])
