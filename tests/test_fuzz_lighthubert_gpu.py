"""Seeded sweep of the LightHuBERT path against the float64 restatement (tests/lighthubert_ref.py, held to the reference's own
fixtures by tests/test_lighthubert_cpu.py): supernet type, ``cfg.model._name``, ``extractor_mode``, ``conv_bias``, batch size 1-4 and
lengths from one frame to about 1.5 s.  Per utterance and state rel_err < 5e-5 (tests/test_encoder_gpu.py's oracle band), over ALL
rows of the utterance: the padded rows of the layer states are defined values here, and state 0's are exactly zero.  No case is
skipped: every drawn configuration is one the path builds."""

import zlib

import numpy as np
import pytest

import lighthubert_ref as R
from oracle import encoder_oracle as O
from test_encoder_gpu import _encoder, _run

pytestmark = pytest.mark.gpu

ORACLE_TOL = 5e-5
N_CASES = 8


def _case(i):
    from s3prl_amd.config import config_from_lighthubert

    rng = np.random.default_rng(zlib.crc32(f"fuzz/lighthubert/{i}".encode()))
    stype = ("base", "small")[i % 2]                      # both supernet types and both names occur whatever the draws are
    name = ("hubert_pruner", "student_hubert")[(i // 2) % 2]
    model_cfg = dict(_name=name, extractor_mode=("layer_norm", "default")[int(rng.integers(2))], conv_bias=bool(rng.integers(2)))
    if name == "hubert_pruner":
        model_cfg["pruner_supernet"] = f"lighthubert_{stype}.yaml"
    else:
        model_cfg["supernet_type"] = stype
    cfg = config_from_lighthubert(model_cfg)
    B = 1 + i % 4
    lengths = [int(x) for x in rng.integers(400, 24000, size=B)]
    if i % 3 == 0:
        lengths[-1] = int(rng.integers(1, 320)) if B > 1 else 400  # one valid frame beside longer ones; alone: a one-frame batch
    return cfg, lengths, int(rng.integers(1 << 16))


@pytest.mark.parametrize("i", range(N_CASES))
def test_fuzz_against_the_restatement(i):
    from s3prl_amd.synth import synth_wavs, synth_weights

    cfg, lengths, seed = _case(i)
    weights = synth_weights(cfg, seed, ("synthetic", "pretrained_like")[i % 2 if cfg.extractor_mode == "layer_norm" else 0])
    wavs = synth_wavs(lengths, seed + 1)
    ref = R.forward(cfg, weights, wavs)
    enc = _encoder(cfg, weights)
    try:
        hs = _run(enc, wavs)
        assert enc.status() == 0
    finally:
        enc.close()
    assert hs.shape == (13,) + ref[0].shape and np.isfinite(hs).all()
    valid = R.valid_frames(cfg, lengths)
    errs = [O.rel_err(hs[l][b], ref[l][b]) for l in range(13) for b in range(len(wavs))]
    print(f"LHFUZZ case {i}: {cfg.lh_model}/{cfg.lh_supernet} D={cfg.encoder_embed_dim} {cfg.extractor_mode} bias={cfg.conv_bias} "
          f"lengths={lengths} valid={valid} worst={max(errs):.2e}")
    assert max(errs) < ORACLE_TOL, (i, cfg.lh_model, cfg.lh_supernet, lengths, ["%.2e" % e for e in errs])
    for b, v in enumerate(valid):
        assert not hs[0][b, v:].any(), "state 0: padded rows exactly zero"
