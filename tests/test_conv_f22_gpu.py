"""The two-output form of the k = 3, stride-2 conv layers (convf22.hip, tuning key `conv_f22`) in the exact-fp32 mode.

A short extractor (conv0 + three k = 3 layers) keeps every k = 3 output as a tap.  Each tap is checked against the float64
oracle with the key on and off, on and off against each other, at conv1 lengths whose residue mod 128 is 1, 63, 64 and 127
(odd and even lengths; the longest utterance last in the buffer), for both extractor kinds.  With the key on, an utterance's
rows are bit-identical alone and inside a batch (ragged for the LayerNorm extractor; the GroupNorm one normalises over the
padded length, as the reference does, so its batch shares one length)."""

import numpy as np
import pytest

from oracle import encoder_oracle as O

pytestmark = pytest.mark.gpu

KINDS = {"group_norm": "tiny_hubert", "layer_norm": "tiny_data2vec"}
TAPS = ("conv1", "conv2", "conv3")


def _cfg(kind):
    from s3prl_amd.synth import named_config

    cfg = named_config(KINDS[kind])
    cfg.conv_layers = [(128, 10, 5)] + [(128, 3, 2)] * 3
    cfg.encoder_layers = 1
    return cfg


def _samples_for_conv1(l1):  # waveform length whose conv1 output has l1 frames
    return 5 * (2 * l1 + 1 - 1) + 10


def _taps(enc, wavs):
    import torch

    enc.forward([torch.from_numpy(w).cuda() for w in wavs])
    torch.cuda.synchronize()
    return {t: enc.debug_tap(t) for t in TAPS}


def _set_key(on):
    from s3prl_amd import _lib

    _lib.check(_lib.load().s3enc_set_tuning(b"conv_f22", on), "s3enc_set_tuning")


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_conv_f22_taps_match_oracle_at_boundary_lengths(kind):
    from s3prl_amd.encoder import HipEncoder
    from s3prl_amd.synth import synth_wavs, synth_weights

    cfg = _cfg(kind)
    weights = synth_weights(cfg, 3)
    enc = HipEncoder(cfg, weights, dtype="fp32")
    try:
        for l1 in (129, 191, 192, 255):  # conv1 L_out mod 128 = 1, 63, 64, 127; conv2 / conv3 lengths vary with it
            n = _samples_for_conv1(l1)
            wavs = synth_wavs([n - 777, n], l1)
            on = _taps(enc, wavs)
            _set_key(0)
            try:
                off = _taps(enc, wavs)
            finally:
                _set_key(1)
            ref = {}
            O.forward(cfg, weights, wavs, dtype=np.float64, taps=ref)
            for t in TAPS:
                r = ref[t]
                a, b = on[t].reshape(r.shape), off[t].reshape(r.shape)
                assert O.rel_err(a, r) < 2e-5, f"{kind} L1={l1} {t}: two-output form {O.rel_err(a, r):.2e} from float64"
                assert O.rel_err(b, r) < 2e-5, f"{kind} L1={l1} {t}: implicit GEMM {O.rel_err(b, r):.2e} from float64"
                assert O.rel_err(a, b) <= 2e-6, f"{kind} L1={l1} {t}: on vs off {O.rel_err(a, b):.2e}"
            assert not np.array_equal(on["conv1"], off["conv1"]), "conv_f22 = 0 did not change the kernel"
    finally:
        enc.close()


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_conv_f22_rows_do_not_depend_on_the_batch(kind):
    from s3prl_amd.encoder import HipEncoder
    from s3prl_amd.synth import synth_wavs, synth_weights

    cfg = _cfg(kind)
    enc = HipEncoder(cfg, synth_weights(cfg, 4), dtype="fp32")
    try:
        # GroupNorm spans the padded batch length (as in the reference): ragged batches only for the LayerNorm extractor
        n = _samples_for_conv1(255) + 3
        lens = [n, n, n] if kind == "group_norm" else [n, _samples_for_conv1(129) + 7, _samples_for_conv1(192)]
        wavs = synth_wavs(lens, 5)
        batch = _taps(enc, wavs)
        alone = _taps(enc, wavs[1:2])
        for t in TAPS:
            rows = alone[t].size // 128
            got = batch[t].reshape(len(lens), -1, 128)[1, :rows]
            assert np.array_equal(got, alone[t].reshape(rows, 128)), f"{kind} {t}: rows differ alone vs in a batch"
    finally:
        enc.close()
