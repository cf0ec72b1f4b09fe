"""One handle, many lengths: a Conformer handle grows its position tables to the longest batch seen and reads the centre rows of
the rel_pos table for every shorter one; every handle regrows its workspace, its small device state and its pinned slots.  The
tables hold values that depend on the position only, so a forward on a handle that has seen other lengths must give the bits of a
fresh handle's forward of the same batch — long, short, longer (across the conv module's 128-frame tile), the first short batch
again, then batches of 3, 4 and 5 utterances."""

import numpy as np
import pytest

from oracle import encoder_oracle as O

import conformer_ref as CR
import wav2vec_ref as WR

pytestmark = pytest.mark.gpu

FP32_TOL = 1e-4

# frames of every utterance, in the order the batches are forwarded on the one handle
BATCHES = [
    [100, 37],               # long
    [40, 12],                # short: the centre rows of a longer table
    [150, 129],              # longer: both tables grow, T crosses 128
    [40, 12],                # the first short batch again, now under a table that has grown twice
    [128, 64, 1],            # B grows from 2 ...
    [90, 127, 33, 65],
    [160, 1, 129, 17, 70],   # ... to 5, on a fourth table size
]


def _frames_to_lengths(cfg, rng, frames):
    rf, hop = 1, 1
    for _, k, s in cfg.conv_layers:
        rf += (k - 1) * hop
        hop *= s
    return [rf + (t - 1) * hop + int(rng.integers(hop)) for t in frames]


@pytest.mark.parametrize("cfg_name", ["tiny_conformer_relpos", "tiny_conformer_rope", "tiny_wav2vec", "tiny_vq_wav2vec_kmeans"])
def test_a_reused_handle_gives_the_bits_of_a_fresh_one(cfg_name):
    import torch

    from s3prl_amd.encoder import HipEncoder
    from s3prl_amd.synth import named_config, synth_wavs, synth_weights

    assert torch.cuda.is_available(), "these tests need the MI355X"
    cfg = named_config(cfg_name)
    weights = synth_weights(cfg, 3)
    vq = cfg.family == "wav2vec" and cfg.vq_type != "none"
    rng = np.random.default_rng(17)
    lengths = [_frames_to_lengths(cfg, rng, frames) for frames in BATCHES]
    lengths[3] = lengths[1]
    wavs = [synth_wavs(ls, 40 + i) for i, ls in enumerate(lengths)]
    wavs[3] = wavs[1]

    def run(enc, ws):
        aux = {} if vq else None
        hs = enc.forward([torch.from_numpy(w).cuda() for w in ws], aux=aux).clone()
        torch.cuda.synchronize()
        assert enc.status() == 0
        return hs, ((aux["codeids"].clone(), aux["codewords"].clone()) if vq else None)

    def reference(ws):
        if cfg.family == "wav2vec":
            return WR.forward(cfg, weights, ws, dtype=np.float64)
        return dict(hidden_states=CR.forward(cfg, weights, ws))

    one = HipEncoder(cfg, weights)
    for i, (frames, ls, ws) in enumerate(zip(BATCHES, lengths, wavs)):
        assert [cfg.num_frames(n) for n in ls] == frames
        hs, a = run(one, ws)
        fresh = HipEncoder(cfg, weights)
        hs_f, a_f = run(fresh, ws)
        fresh.close()
        assert tuple(hs.shape) == (cfg.num_hidden_states, len(ws), max(frames), cfg.encoder_embed_dim)
        assert torch.equal(hs, hs_f), f"{cfg_name}: forward {i} (frames {frames}) differs from a fresh handle's"
        if vq:
            assert torch.equal(a[0], a_f[0]) and torch.equal(a[1], a_f[1]), f"{cfg_name}: forward {i}: codes differ"
        if i in (0, len(BATCHES) - 1):
            ref = reference(ws)
            got = hs.cpu().numpy()
            valid = [cfg.valid_frames(n, max(ls)) for n in ls]
            err = max(O.rel_err(got[l][b, :v], ref["hidden_states"][l][b, :v]) for l in range(len(got)) for b, v in enumerate(valid))
            whole = max(O.rel_err(got[l], ref["hidden_states"][l]) for l in range(len(got)))
            print(f"{cfg_name}: forward {i} frames {frames}: per-(state, utterance) rel-err {err:.2e}, whole states {whole:.2e}")
            assert max(err, whole) < FP32_TOL, (cfg_name, i, err, whole)
            if vq:  # weight seed 3 decides both batches with float64 margins of 1.8e-4 and 1.2e-4: no near-tie, the ids are exact
                assert ref["margin"] >= 1e-4
                assert np.array_equal(a[0].cpu().numpy(), ref["codeids"])
    one.close()


def _samples_for_frames(cfg, rng, t):
    """A length the config's own ``num_frames`` maps to exactly ``t`` frames (``num_frames`` never decreases with the length)."""

    def first(frames):  # the shortest length with at least `frames` frames
        lo, hi = 1, 1 << 22
        while lo < hi:
            mid = (lo + hi) // 2
            lo, hi = (lo, mid) if cfg.num_frames(mid) >= frames else (mid + 1, hi)
        return lo

    return int(rng.integers(first(t), first(t + 1)))


def _reuse_bits(cfg_name, batches, seed):
    """Forward `batches` (frames per utterance) on ONE handle; each result must be the bits of a fresh handle's forward."""
    import torch

    from s3prl_amd.encoder import HipEncoder
    from s3prl_amd.synth import named_config, synth_wavs, synth_weights

    assert torch.cuda.is_available(), "these tests need the MI355X"
    cfg = named_config(cfg_name)
    weights = synth_weights(cfg, 3)
    rng = np.random.default_rng(seed)
    lengths = [[_samples_for_frames(cfg, rng, t) for t in frames] for frames in batches]
    wavs = [synth_wavs(ls, 60 + i) for i, ls in enumerate(lengths)]
    for i, frames in enumerate(batches):  # an equal list of frames is the same batch again
        j = batches.index(frames)
        lengths[i], wavs[i] = lengths[j], wavs[j]

    def run(enc, ws):
        hs = enc.forward([torch.from_numpy(w).cuda() for w in ws]).clone()
        torch.cuda.synchronize()
        assert enc.status() == 0
        return hs

    one = HipEncoder(cfg, weights)
    for i, (frames, ls, ws) in enumerate(zip(batches, lengths, wavs)):
        assert [cfg.num_frames(n) for n in ls] == frames
        hs = run(one, ws)
        fresh = HipEncoder(cfg, weights)
        hs_f = run(fresh, ws)
        fresh.close()
        assert tuple(hs.shape) == (cfg.num_hidden_states, len(ws), cfg.num_output_frames(max(ls)), cfg.encoder_embed_dim)
        assert torch.equal(hs, hs_f), f"{cfg_name}: forward {i} (frames {frames}) differs from a fresh handle's"
    one.close()


# 2 utterances, then 5 with a longer longest one (the workspace and the small device state regrow), then the first 2 again.  Five
# frames at least: more than 200 samples and two frames inside the batch for Mockingjay's mel front end and CMVN, and a frame left
# at multires-HuBERT's coarsest resolution.  (Each family's own test file scores it against the reference.)
REGROW = [[24, 9], [40, 5, 17, 33, 12], [24, 9]]


@pytest.mark.parametrize("cfg_name", ["tiny_hubert", "tiny_multires", "tiny_cpc_gru", "tiny_apc", "tiny_mockingjay_chunk"])
def test_a_reused_handle_regrows_for_a_larger_batch(cfg_name):
    _reuse_bits(cfg_name, REGROW, 23)


def test_the_staging_ring_regrows_for_a_table_beyond_its_slot():
    """The first batch sizes a slot of the pinned staging ring at 4 * bytes + 4096: wav2vec's 16-byte rows of B = 2 make 4224 bytes,
    which the 4608 bytes of B = 288 outgrow — the ring is freed and reallocated behind forwards that read it."""
    rng = np.random.default_rng(5)
    _reuse_bits("tiny_wav2vec", [[3, 1], [int(t) for t in rng.integers(1, 4, 288)], [3, 1]], 29)
