"""Seeded sweep over the wav2vec / vq-wav2vec configurations s3enc_create accepts — widths 32..1024 (every gn1_apply template),
conv0 strides 1..8, extractors of 2..6 layers, aggregator kernels 1..64, both quantizers at depths 1..4, 1..16 groups, 1..320
variables, shared and per-group codebooks — on ragged batches against the float64 restatement (tests/wav2vec_ref.py), scored per
(state, utterance); code ids exact.  The fixtures of tests/test_wav2vec_gpu.py pin the released geometry; this guards the
generality wav2vec_check_config promises.  tests/test_fuzz_wav2vec_cpu.py proves on the CPU that every seed has a weight seed
whose quantizer decisions are no near-ties (the rule of tests/golden/make_golden_wav2vec.py)."""

import functools

import numpy as np
import pytest

from oracle import encoder_oracle as O

import wav2vec_ref as R

pytestmark = pytest.mark.gpu

FP32_TOL = 1e-4     # the suite's exact-fp32 bar
MIN_MARGIN = 1e-4   # tests/golden/make_golden_wav2vec.py: every quantizer decision's relative top-2 margin
MAX_TRIES = 8       # weight seeds tried per sweep seed
N_SEEDS = 24
WIDE = (512, 544, 1024)

# what the sweep must contain by construction, not by luck (a draw is overridden by these)
PINNED = {
    0: dict(C=512, vq_type="kmeans", vq_groups=1),                 # k-means group width 512: the whole LDS row of kmeans_scores
    1: dict(C=64, vq_type="kmeans", vq_groups=16),                 # k-means group width 4, G = 16
    2: dict(vq_type="gumbel", vq_depth=1),                         # the differently named single projection
    3: dict(vq_type="gumbel", vq_depth=3),                         # h0 -> h1
    4: dict(vq_type="gumbel", vq_depth=4),                         # h0 -> h1 -> h0
    5: dict(vq_type="gumbel", vq_vars=1),                          # V = 1: idle lanes only
    6: dict(agg_kernels=[64, 3]),                                  # the largest aggregator kernel (63 pad rows)
    7: dict(C=1024, vq_type="none"),                               # gn1_apply_kernel<4>
    8: dict(C=544, vq_type="gumbel", vq_groups=2, vq_vars=70),     # gn1_apply_kernel<3>, quads that do not fill the third wave pass
    9: dict(n_mid=0, last_kernel=1, agg_kernels=[1]),              # n_conv = 2; aggregator kernel 1: pad == 0
    10: dict(vq_type="kmeans", vq_vars=1, combine_groups=True),    # V = 1 through the distance kernel
    11: dict(C=288, vq_type="kmeans", vq_groups=8, vq_vars=130),
}


def _random_wav2vec_config(rng, pin=None):
    from s3prl_amd.config import wav2vec_config

    pin = pin or {}
    C = int(pin.get("C", rng.choice([32, 64, 96, 160, 288])))  # 512 and above: the pinned seeds only, on short inputs
    wide = C in WIDE
    s0 = int(rng.choice([1, 2, 3, 5, 8]))
    n_mid = int(pin.get("n_mid", rng.integers(0, 2 if wide else 5)))
    conv = [(C, 10, s0)] + [(C, int(rng.choice([1, 2, 3, 5, 8])), int(rng.choice([1, 2, 3]))) for _ in range(n_mid)]
    conv.append((C, int(pin.get("last_kernel", rng.choice([1, 2]))), 1))
    n_agg = int(rng.integers(1, 3 if wide else 5))
    kernels = pin.get("agg_kernels", [int(rng.choice([1, 2, 3, 7, 12])) for _ in range(n_agg)])
    flags = dict(agg_zero_pad=bool(rng.integers(2)), log_compression=bool(rng.integers(2)), skip_connections_agg=bool(rng.integers(2)),
                 non_affine_group_norm=bool(rng.integers(2)), no_conv_bias=bool(rng.integers(2)),
                 residual_scale=float(rng.choice([0.5, 0.25])))
    vq_type = str(rng.choice(["none", "gumbel", "kmeans"]))
    vq_type = pin.get("vq_type", vq_type)
    groups = [g for g in (1, 2, 4, 8, 16) if C % g == 0 and (C // g) % 4 == 0]
    G = int(rng.choice(groups))
    V = int(rng.choice([1, 5, 32, 70, 130, 320]))
    combine = bool(rng.integers(2))
    depth = int(rng.integers(1, 5))
    if vq_type != "none":
        flags.update(vq_type=vq_type, vq_groups=int(pin.get("vq_groups", G)), vq_vars=int(pin.get("vq_vars", V)),
                     combine_groups=bool(pin.get("combine_groups", combine)))
        if vq_type == "gumbel":
            flags["vq_depth"] = int(pin.get("vq_depth", depth))
    return wav2vec_config(conv, [(C, k, 1) for k in kernels], **flags)


def receptive_field(cfg):
    """the fewest samples that give one frame, and the hop between frames"""
    rf, hop = 1, 1
    for _, k, s in cfg.conv_layers:
        rf += (k - 1) * hop
        hop *= s
    return rf, hop


def _lengths(rng, cfg):
    """B = 1..4 ragged lengths: one utterance exactly at the receptive field (a single frame of its own: alone in the batch,
    T = 1), the others 20..70 frames — fewer where the early, long layers of a small-stride extractor would make the float64
    reference slow (its cost is what is bounded, the frame count of the widest configurations stays at 20..24)."""
    rf, hop = receptive_field(cfg)
    C = cfg.conv_dim
    B = int(rng.integers(1, 3 if C in WIDE else 5))
    t_hi = 24 if C in WIDE else 70
    while t_hi > 20:  # operand of the reference's widest im2col: B x L1 x k1 x C values
        n = rf + (t_hi - 1) * hop
        L = cfg.conv_lengths(n)
        if B * max(L[i] * cfg.conv_layers[i][1] for i in range(1, len(L))) * C <= 6e6:
            break
        t_hi -= 1
    lengths = [rf + int(rng.integers(19 * hop, t_hi * hop)) for _ in range(B - 1)]
    lengths.insert(int(rng.integers(B)), rf)
    return lengths


def case_inputs(seed):
    """(cfg, lengths, waveforms) of a sweep seed"""
    from s3prl_amd.synth import synth_wavs

    rng = np.random.default_rng(7000 + seed)
    cfg = _random_wav2vec_config(rng, PINNED.get(seed))
    lengths = _lengths(rng, cfg)
    wavs = synth_wavs(lengths, seed + 1, dc=float(rng.choice([0.0, 0.2])), scale=float(rng.choice([1.0, 0.1])))
    return cfg, lengths, wavs


def pick_weights(cfg, wavs, seed):
    """The near-tie rule of make_golden_wav2vec.py: the first weight seed of 100 * seed + (0 .. MAX_TRIES - 1) whose float64
    decisions all have a relative top-2 margin >= MIN_MARGIN.  Returns (weight seed, weights, float64 reference)."""
    from s3prl_amd.synth import synth_weights

    tried = []
    for wseed in range(100 * seed, 100 * seed + MAX_TRIES):
        weights = synth_weights(cfg, wseed)
        ref = R.forward(cfg, weights, wavs, dtype=np.float64)
        if ref["margin"] is None or ref["margin"] >= MIN_MARGIN:
            return wseed, weights, ref
        tried.append(ref["margin"])
    raise AssertionError(f"seed {seed}: no weight seed within {MAX_TRIES} tries has a margin >= {MIN_MARGIN:g}: {tried}")


@functools.lru_cache(maxsize=None)
def case(seed):
    cfg, lengths, wavs = case_inputs(seed)
    wseed, weights, ref = pick_weights(cfg, wavs, seed)
    return cfg, lengths, wavs, wseed, weights, ref


def per_utterance_errors(got, ref, valid):
    """worst rel-err over (state, utterance): every utterance's row, and its own frames alone — a short utterance does not hide
    behind a long one, nor behind the frames of its own padding"""
    worst = 0.0
    for l in range(len(ref)):
        for b, v in enumerate(valid):
            worst = max(worst, O.rel_err(got[l][b], ref[l][b]), O.rel_err(got[l][b, :v], ref[l][b, :v]))
    return worst


@pytest.mark.parametrize("seed", range(N_SEEDS))
def test_random_wav2vec_matches_float64(seed):
    import torch

    from s3prl_amd.encoder import HipEncoder

    assert torch.cuda.is_available(), "these tests need the MI355X"
    cfg, lengths, wavs, wseed, weights, ref = case(seed)
    vq = cfg.vq_type != "none"
    n_max = max(lengths)
    T, C, B = cfg.num_frames(n_max), cfg.conv_dim, len(wavs)
    valid = [cfg.valid_frames(n, n_max) for n in lengths]
    dev = [torch.from_numpy(w).cuda() for w in wavs]
    enc = HipEncoder(cfg, weights)
    assert enc.num_states() == len(cfg.agg_layers) + 1 == len(ref["hidden_states"])
    assert [enc.num_frames(n) for n in lengths] == [cfg.num_frames(n) for n in lengths] and min(valid) == 1
    aux = {} if vq else None
    hs = enc.forward(dev, aux=aux).clone()
    torch.cuda.synchronize()
    assert tuple(hs.shape) == (len(cfg.agg_layers) + 1, B, T, C)
    got = hs.cpu().numpy()
    assert np.isfinite(got).all()
    err = per_utterance_errors(got, ref["hidden_states"], valid)
    what = f"seed {seed}: C {C} conv {[(k, s) for _, k, s in cfg.conv_layers]} agg {[k for _, k, _ in cfg.agg_layers]} vq {cfg.vq_type}"
    if vq:
        what += f" G {cfg.vq_groups} V {cfg.vq_vars} depth {cfg.vq_depth} shared {cfg.combine_groups} weight seed {wseed} margin {ref['margin']:.2e}"
    print(f"{what} lengths {lengths} T {T}: worst per-(state, utterance) rel-err {err:.2e}")
    assert err < FP32_TOL, (what, lengths, err)
    if vq:
        ids, cw = aux["codeids"].cpu().numpy(), aux["codewords"].cpu().numpy()
        assert ids.dtype == np.int64 and ids.shape == (B, T, cfg.vq_groups) and cw.shape == (B, T, C)
        assert np.array_equal(ids, ref["codeids"]), (what, f"{(ids != ref['codeids']).sum()} of {ids.size} code ids differ")
        cw_err = max(max(O.rel_err(cw[b], ref["codewords"][b]), O.rel_err(cw[b, :v], ref["codewords"][b, :v])) for b, v in enumerate(valid))
        print(f"seed {seed}: codewords rel-err {cw_err:.2e}")
        assert cw_err < FP32_TOL, (what, cw_err)
        # a gather of fp32 table rows: exact
        Dv = C // cfg.vq_groups
        key = "vector_quantizer.vars" if cfg.vq_type == "gumbel" else "vector_quantizer.embedding"
        table = weights[key].reshape(-1, cfg.vq_vars, Dv) if cfg.vq_type == "gumbel" else weights[key].transpose(1, 0, 2)
        want = np.stack([table[g % table.shape[0]][ids[..., g]] for g in range(cfg.vq_groups)], axis=2).reshape(B, T, C)
        assert np.array_equal(cw, want), what
    assert enc.status() == 0

    # a second handle: the batch permuted, and a shard of it padded to the batch's n_max, reproduce the rows bit for bit
    other = HipEncoder(cfg, weights)
    perm = [int(i) for i in np.random.default_rng(seed).permutation(B)]
    paux = {} if vq else None
    permuted = other.forward([dev[i] for i in perm], aux=paux).clone()
    for j, i in enumerate(perm):
        assert torch.equal(permuted[:, j], hs[:, i]), (what, "permuted", j, i)
        if vq:
            assert torch.equal(paux["codeids"][j], aux["codeids"][i]) and torch.equal(paux["codewords"][j], aux["codewords"][i])
    lo = B // 2
    saux = {} if vq else None
    shard = other.forward(dev[lo:], n_max=n_max, aux=saux).clone()
    torch.cuda.synchronize()
    assert torch.equal(shard, hs[:, lo:]), (what, "shard")
    if vq:
        assert torch.equal(saux["codeids"], aux["codeids"][lo:]) and torch.equal(saux["codewords"], aux["codewords"][lo:])
    assert other.status() == 0
    enc.close()
    other.close()
