"""Mockingjay / TERA / AudioALBERT on the MI355X, every test through the C ABI: the log-mel front end per frame against float64, the
LayerNorm with a run-time eps and the input representation against float64, the model pinned to the reference's own outputs
(tests/golden/make_golden_mockingjay.py) from the waveforms and from the stored features, the chunked forward against the same
chunks run as separate sequences bit for bit, layer sharing against copies bit for bit, featurize, shards, handle reuse and the
refusals.  Only LIVE rows (in front of an utterance's frame count) are compared with a reference; padding rows must be finite."""

import ctypes as C

import numpy as np
import pytest

from oracle import encoder_oracle as O

import mockingjay_ref as R

pytestmark = pytest.mark.gpu

FP32_TOL = 1e-4  # the project's fixture bound
OP_TOL = 2e-5    # the project's op bound
FBANK_TOL_CMVN, FBANK_TOL_RAW = 5e-4, 2e-4  # tests/test_fbank_gpu.py: the log-mel bins behind / without CMVN, absolute
NAMES = ["tiny_pad", "tiny_eq", "tiny_chunk", "tiny_chunk3", "tiny_eps", "tiny_albert", "tiny_kaldi", "tera_base_pseudo"]
FIXTURES = ["mockingjay/" + n for n in NAMES]
GUARD = 3  # NaN rows in front of and behind an output buffer: nothing outside it may be written


def _torch():
    import torch

    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def _ptr(t, offset_elems=0):
    return C.c_void_p(t.data_ptr() + 4 * offset_elems) if t is not None else None


def _dev(x, dtype=np.float32):
    torch = _torch()
    return torch.from_numpy(np.ascontiguousarray(x, dtype=dtype)).cuda()


def _encoder(cfg, weights, dtype="fp32"):
    from s3prl_amd.encoder import HipEncoder

    return HipEncoder(cfg, weights, dtype=dtype)


# ---- the front end: s3enc_logmel_forward ----------------------------------------------------------------------------------------
def _logmel(wavs, n_mels, cmvn, n_max=0):
    """(B, T, n_mels) behind GUARD NaN rows on either side, and the frame counts the library hands out"""
    from s3prl_amd import _lib

    torch = _torch()
    lib = _lib.load()
    dev = [_dev(w) for w in wavs]
    lengths = [len(w) for w in wavs]
    B, T = len(wavs), 1 + (n_max or max(lengths)) // 160
    lens = (C.c_int64 * B)(*lengths)
    counts = (C.c_int32 * B)()
    _lib.check(lib.s3enc_logmel_frame_counts(lens, B, n_max, counts), "s3enc_logmel_frame_counts")
    buf = torch.full((GUARD + B * T + GUARD, n_mels), float("nan"), device="cuda")
    ptrs = (C.c_void_p * B)(*[w.data_ptr() for w in dev])
    _lib.check(lib.s3enc_logmel_forward(ptrs, lens, B, n_max, n_mels, -25.0, int(cmvn), counts, _ptr(buf, GUARD * n_mels), 0, None),
               "s3enc_logmel_forward")
    torch.cuda.synchronize()
    assert torch.isnan(buf[:GUARD]).all() and torch.isnan(buf[GUARD + B * T:]).all(), "rows outside the output were written"
    return buf[GUARD:GUARD + B * T].reshape(B, T, n_mels).cpu().numpy(), list(counts)


@pytest.mark.parametrize("cmvn", [True, False])
@pytest.mark.parametrize("lengths, scale", [([201], 1.0), ([320], 1.0), ([4000, 3900], 1.0), ([8000, 16000], 1.0),
                                            ([4000, 2345, 3111], 1e-3), ([4000, 2345, 3111], 30.0)])
def test_logmel_per_frame_against_float64(lengths, scale, cmvn):
    """Every live frame against the float64 front end (tests/test_mockingjay_cpu.py pins that one to torch.stft): n = 201 is T = 2,
    3900 beside 4000 ends within 200 samples of max_len (zeros and reflection mixed), 8000 beside 16000 is normalised over 50
    frames.  Gaussian noise without digital silence; input scales 1e-3 and 30 go through the decibel normalisation."""
    from s3prl_amd.synth import synth_wavs

    wavs = synth_wavs(lengths, 900 + len(lengths), scale=scale)
    got, counts = _logmel(wavs, 80, cmvn)
    ref, ref_counts = R.logmel(wavs, 80, cmvn=cmvn)
    live = R.frame_counts(lengths)
    assert counts == live and got.shape == ref.shape and np.isfinite(got).all()
    tol = FBANK_TOL_CMVN if cmvn else FBANK_TOL_RAW
    for b, n in enumerate(live):
        err = np.abs(got[b, :n] - ref[b, :n]).max(axis=1)
        print(f"logmel lengths {lengths} scale {scale:g} cmvn={cmvn} utt {b} ({n} live frames): max abs err {err.max():.2e} at frame "
              f"{int(err.argmax())}, last frame {err[-1]:.2e}")
        assert err.max() < tol, (lengths, scale, cmvn, b, err.max())
        if cmvn:
            assert not got[b, n:].any(), "rows behind the frame count must be exactly 0"
    if lengths == [8000, 16000]:
        assert live == [50, 101] and (not cmvn or (not got[0, 50].any() and got[0, 49].any()))


def test_logmel_inside_a_longer_padding_length():
    """n_max beyond the longest utterance (a data-parallel shard): the frame count and the edge frames follow n_max"""
    from s3prl_amd.synth import synth_wavs

    wavs = synth_wavs([4000, 2345], 17)
    got, counts = _logmel(wavs, 16, True, n_max=5000)
    ref, _ = R.logmel(wavs, 16, max_len=5000)
    assert counts == R.frame_counts([4000, 2345], 5000) and got.shape == (2, 32, 16)
    for b, n in enumerate(counts):
        assert np.abs(got[b, :n] - ref[b, :n]).max() < FBANK_TOL_CMVN and not got[b, n:].any()


# ---- s3enc_op_layernorm_eps -------------------------------------------------------------------------------------------------------
def _ln_eps(x, g, b, eps):
    from s3prl_amd import _lib

    torch = _torch()
    rows, Cc = x.shape
    buf = torch.full((GUARD + rows + GUARD, Cc), float("nan"), device="cuda")
    dx, dg, db = _dev(x), _dev(g), _dev(b)  # (held: a temporary's block would be handed to the next allocation)
    _lib.check(_lib.load().s3enc_op_layernorm_eps(_ptr(dx), _ptr(dg), _ptr(db), eps, rows, Cc, _ptr(buf, GUARD * Cc), None),
               "s3enc_op_layernorm_eps")
    torch.cuda.synchronize()
    assert torch.isnan(buf[:GUARD]).all() and torch.isnan(buf[GUARD + rows:]).all()
    return buf[GUARD:GUARD + rows].cpu().numpy()


@pytest.mark.parametrize("eps", [1e-12, 1e-2])
@pytest.mark.parametrize("Cc", [128, 768])
@pytest.mark.parametrize("rows", [1, 3, 4, 5, 9])
def test_layernorm_eps_against_float64(rows, Cc, eps):
    """Rows of variance 1e-6, 1e-4, 1e-2 and 1 (cycled over the rows; a kernel of 4 rows per workgroup: 3 / 4 / 5 / 9 straddle the
    tile) against float64 at the eps handed in.  Each row's mean is of the size of its standard deviation: an fp32 row whose mean
    dwarfs its deviation carries ulp(mean) / sigma of error into ANY fp32 evaluation, which is not what this test is about.  With
    1e-5 baked in, the variance-1e-6 rows at eps 1e-12 come out 3.3 times too small."""
    rng = np.random.default_rng(rows * 1000 + Cc)
    sig = np.array([1e-3, 1e-2, 1e-1, 1.0])[np.arange(rows) % 4][:, None]
    x = ((rng.standard_normal((rows, Cc)) + 0.5) * sig).astype(np.float32)
    g = (1.0 + 0.1 * rng.standard_normal(Cc)).astype(np.float32)
    b = (0.1 * rng.standard_normal(Cc)).astype(np.float32)
    got = _ln_eps(x, g, b, eps)
    ref = R.layer_norm(x.astype(np.float64), g.astype(np.float64), b.astype(np.float64), eps)
    for r in range(rows):
        err = O.rel_err(got[r], ref[r])
        assert err < OP_TOL, (rows, Cc, eps, r, err)
    wrong = R.layer_norm(x[:1].astype(np.float64), g.astype(np.float64), b.astype(np.float64), 1e-5)
    assert O.rel_err(got[0], wrong[0]) > 1e-3  # row 0 has variance 1e-6: neither eps is 1e-5


# ---- s3enc_op_input_repr ----------------------------------------------------------------------------------------------------------
def _input_repr(feat, w, bias, pos, Tc, g, b, eps):
    from s3prl_amd import _lib

    torch = _torch()
    rows, F = feat.shape
    D = w.shape[0]
    buf = torch.full((GUARD + rows + GUARD, D), float("nan"), device="cuda")
    p = np.ascontiguousarray(pos, dtype=np.float32)
    dfeat, dw, dbias, dg, db = _dev(feat), _dev(w), _dev(bias), _dev(g), _dev(b)  # (held: see _ln_eps)
    _lib.check(_lib.load().s3enc_op_input_repr(_ptr(dfeat), _ptr(dw), _ptr(dbias), C.c_void_p(p.ctypes.data), Tc,
                                               _ptr(dg), _ptr(db), eps, rows, F, D, _ptr(buf, GUARD * D), None),
               "s3enc_op_input_repr")
    torch.cuda.synchronize()
    assert torch.isnan(buf[:GUARD]).all() and torch.isnan(buf[GUARD + rows:]).all()
    return buf[GUARD:GUARD + rows].cpu().numpy()


@pytest.mark.parametrize("F, D", [(16, 128), (80, 768)])
@pytest.mark.parametrize("Tc", [1, 3, 4, 5, 13])
def test_input_repr_against_float64(Tc, F, D):
    """Linear + position row + LayerNorm(1e-12), every row against float64; three sequences of Tc rows each, so that row r must
    carry the position row of r mod Tc (Tc = 3, 4, 5 straddle the row kernel's tile of 4)."""
    rng = np.random.default_rng(Tc * 100 + F)
    rows = 3 * Tc
    feat = rng.standard_normal((rows, F)).astype(np.float32)
    w = (rng.standard_normal((D, F)) / np.sqrt(F)).astype(np.float32)
    bias = (0.05 * rng.standard_normal(D)).astype(np.float32)
    g = (1.0 + 0.1 * rng.standard_normal(D)).astype(np.float32)
    b = (0.1 * rng.standard_normal(D)).astype(np.float32)
    pos = R.position_table(Tc, D)
    got = _input_repr(feat, w, bias, pos, Tc, g, b, 1e-12)
    f64 = lambda a: a.astype(np.float64)  # noqa: E731
    pre = f64(feat) @ f64(w).T + f64(bias) + np.tile(f64(pos), (3, 1))
    ref = R.layer_norm(pre, f64(g), f64(b), 1e-12)
    for r in range(rows):
        assert O.rel_err(got[r], ref[r]) < OP_TOL, (Tc, F, D, r)
    if Tc > 1:  # a position row taken from the global row index instead of r mod Tc is far outside the bound
        shifted = R.layer_norm(f64(feat) @ f64(w).T + f64(bias) + f64(R.position_table(rows, D)), f64(g), f64(b), 1e-12)
        assert O.rel_err(got[Tc], shifted[Tc]) > 1e-3


# ---- the model through its ops: chunks as separate sequences ------------------------------------------------------------------------
def _chunk_plan(cfg, T):
    sizes = R.chunk_sizes(T, cfg.mj_sequence_length)
    return sizes[0], len(sizes)


def _op_chain(cfg, weights, feats_dev, counts):
    """The states from (B, T, F) features through s3enc_op_input_repr / s3enc_op_gemm / s3enc_op_attention / s3enc_op_layernorm_eps,
    with NO chunk logic: every chunk is handed over as a sequence of its own (B * n sequences of Tc rows, the last chunk padded with
    zero feature rows), with its own key count (at least 1).  Returns (NL + 1) x (B, T, D)."""
    from s3prl_amd import _lib

    torch = _torch()
    lib = _lib.load()
    B, T, F = feats_dev.shape
    D, FF, H, eps = cfg.encoder_embed_dim, cfg.encoder_ffn_embed_dim, cfg.encoder_attention_heads, cfg.mj_layer_norm_eps
    Tc, n = _chunk_plan(cfg, T)
    Tp = n * Tc
    feat = torch.zeros((B, Tp, F), device="cuda")
    feat[:, :T] = feats_dev
    rows = B * Tp
    kv = [max(1, min(max(c - ch * Tc, 0), min(Tc, T - ch * Tc))) for c in counts for ch in range(n)]
    dkv = torch.tensor(kv, dtype=torch.int32, device="cuda")
    w = lambda name: weights[name]  # noqa: E731
    dw = lambda name: _dev(weights[name])  # noqa: E731

    def gemm(a, K, W, bias, N, act=0, res=None):
        out = torch.empty((rows, N), device="cuda")
        _lib.check(lib.s3enc_op_gemm(_lib.F32, _ptr(a), K, 0, _ptr(W), _ptr(bias), rows, N, K, 1, act, _ptr(res), None, _ptr(out), None, N,
                                     0, None), "s3enc_op_gemm")
        return out

    def ln(a, g, b):
        out = torch.empty((rows, D), device="cuda")
        _lib.check(lib.s3enc_op_layernorm_eps(_ptr(a), _ptr(g), _ptr(b), eps, rows, D, _ptr(out), None), "s3enc_op_layernorm_eps")
        return out

    ir = "input_representations."
    x = torch.empty((rows, D), device="cuda")
    pos = R.position_table(Tc, D)
    in_w, in_b, in_g, in_beta = (dw(ir + n) for n in ("spec_transform.weight", "spec_transform.bias", "LayerNorm.weight", "LayerNorm.bias"))
    _lib.check(lib.s3enc_op_input_repr(_ptr(feat), _ptr(in_w), _ptr(in_b), C.c_void_p(pos.ctypes.data), Tc, _ptr(in_g), _ptr(in_beta),
                                       eps, rows, F, D, _ptr(x), None), "s3enc_op_input_repr")
    states = [x]
    for l in range(cfg.encoder_layers):
        p = f"encoder.layer.{0 if cfg.mj_share_layer else l}."
        sc = np.float32(0.125)
        wqkv = np.concatenate([w(p + "attention.self.query.weight") * sc, w(p + "attention.self.key.weight"),
                               w(p + "attention.self.value.weight")])
        bqkv = np.concatenate([w(p + "attention.self.query.bias") * sc, w(p + "attention.self.key.bias"), w(p + "attention.self.value.bias")])
        qkv = gemm(x, D, _dev(wqkv), _dev(bqkv), 3 * D)
        ctx = torch.empty((rows, D), device="cuda")
        _lib.check(lib.s3enc_op_attention(_lib.F32, _ptr(qkv), _ptr(ctx), C.c_void_p(dkv.data_ptr()), B * n, Tc, H, None, 0, None, None),
                   "s3enc_op_attention")
        a = gemm(ctx, D, dw(p + "attention.output.dense.weight"), dw(p + "attention.output.dense.bias"), D, res=x)
        a = ln(a, dw(p + "attention.output.LayerNorm.weight"), dw(p + "attention.output.LayerNorm.bias"))
        h = gemm(a, D, dw(p + "intermediate.dense.weight"), dw(p + "intermediate.dense.bias"), FF, act=1)
        y = gemm(h, FF, dw(p + "output.dense.weight"), dw(p + "output.dense.bias"), D, res=a)
        x = ln(y, dw(p + "output.LayerNorm.weight"), dw(p + "output.LayerNorm.bias"))
        states.append(x)
    torch.cuda.synchronize()
    return [s.reshape(B, Tp, D)[:, :T].contiguous() for s in states]


def _score_live(got, hs, counts, meta, what):
    ts, cs = meta["t_stride"], meta["c_stride"]
    worst = 0.0
    for l in range(len(hs)):
        g = got[l].cpu().numpy()
        assert np.isfinite(g).all(), (what, l, "padding rows must be finite")
        for b, n in enumerate(counts):
            err = O.rel_err(g[b, :n:ts, ::cs], hs[l][b, :-(-n // ts)])
            worst = max(worst, err)
    return worst


def _live_norm(h, counts):
    return float(np.linalg.norm(np.concatenate([h[b, :n].astype(np.float64).reshape(-1) for b, n in enumerate(counts)])))


@pytest.mark.parametrize("name", FIXTURES)
def test_model_from_the_fixture_features(name, golden_loader):
    """The features the reference was fed (mockingjay_ref's front end, rounded to fp32) through the op chain: every state per utterance."""
    meta, cfg, weights, wavs, hs, norms = golden_loader(name)
    feats, counts = R.features(cfg, wavs)
    got = _op_chain(cfg, weights, _dev(feats.astype(np.float32)), counts)
    err = _score_live(got, hs, counts, meta, name)
    print(f"{name}: model from the fixture's features, worst per-(state, utterance) rel-err {err:.2e}")
    assert err < FP32_TOL, (name, err)


# ---- the family ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_fp32_from_waveforms(name, golden_loader):
    torch = _torch()
    meta, cfg, weights, wavs, hs, norms = golden_loader(name)
    enc = _encoder(cfg, weights)
    assert enc.num_states() == len(hs) == cfg.encoder_layers + 1
    out = enc.forward([torch.from_numpy(w).cuda() for w in wavs])
    torch.cuda.synchronize()
    assert list(out.shape[1:]) == meta["shape"]
    assert [enc.valid_frames(n, max(meta["lengths"])) for n in meta["lengths"]] == meta["frames"]
    err = _score_live(out, hs, meta["frames"], meta, name)
    print(f"{name}: from waveforms, worst per-(state, utterance) rel-err {err:.2e}")
    assert err < FP32_TOL, (name, err)
    for l in range(len(hs)):
        n = _live_norm(out[l].cpu().numpy(), meta["frames"])
        assert abs(n - norms[l]) / norms[l] < FP32_TOL
    assert enc.status() == 0


def _family_features(cfg, wavs_np):
    """what the family's own front end computes, through the front end's C entry: (B, T, F) on the device and the frame counts"""
    torch = _torch()
    if cfg.mj_frontend == "mel":
        got, counts = _logmel(wavs_np, cfg.mj_input_dim, cfg.mj_cmvn)
        return _dev(got), counts if cfg.mj_cmvn else [got.shape[1]] * len(wavs_np)
    from s3prl_amd import _lib

    c = _lib.S3FbankConfig()
    c.sample_rate, c.num_mel_bins, c.frame_length_ms, c.frame_shift_ms = 16000, cfg.mj_kaldi_mel_bins, cfg.mj_kaldi_frame_length, cfg.mj_kaldi_frame_shift
    c.preemphasis, c.delta_order, c.delta_win_length, c.use_cmvn, c.cmvn_eps = cfg.mj_kaldi_preemphasis, cfg.mj_delta_order, cfg.mj_delta_win, int(cfg.mj_cmvn), 1e-10
    dev = [_dev(w) for w in wavs_np]
    lengths = [len(w) for w in wavs_np]
    counts = [cfg.num_frames(n) for n in lengths]
    B, T = len(dev), max(counts)
    out = torch.empty((B, T, cfg.mj_input_dim), device="cuda")
    _lib.check(_lib.load().s3enc_fbank_forward(C.byref(c), (C.c_void_p * B)(*[w.data_ptr() for w in dev]), (C.c_int64 * B)(*lengths), B,
                                               _ptr(out), T, 0, None), "s3enc_fbank_forward")
    torch.cuda.synchronize()
    return out, counts


@pytest.mark.parametrize("name", ["tiny_chunk", "tiny_chunk3", "tiny_pad", "tiny_kaldi", "tiny_albert"])
def test_family_is_its_ops_with_the_chunks_as_separate_sequences_bit_for_bit(name, golden_loader):
    """A handle takes waveforms, so "the chunks as separate utterances" are handed to the kernels directly: the front end's C entry,
    then the op chain above, which knows nothing of chunking — B * n sequences of Tc rows, positions from 0, own key counts.  The
    chunked handle's states equal it BIT FOR BIT on every row (live or not); so do the unchunked fixtures' (n = 1)."""
    torch = _torch()
    meta, cfg, weights, wavs, hs, norms = golden_loader("mockingjay/" + name)
    enc = _encoder(cfg, weights)
    out = enc.forward([torch.from_numpy(w).cuda() for w in wavs]).clone()
    torch.cuda.synchronize()
    feats, counts = _family_features(cfg, wavs)
    assert counts == meta["frames"]
    want = _op_chain(cfg, weights, feats, counts)
    for l in range(len(want)):
        assert torch.equal(out[l], want[l]), (name, l)
    if name.startswith("tiny_chunk"):
        assert _chunk_plan(cfg, out.shape[2])[1] == len(meta["chunks"]) > 1


def test_shared_layer_equals_a_handle_with_copies_of_the_weights(golden_loader):
    """tiny_albert (one layer uploaded once, run three times) against a non-shared handle given three copies, bit for bit"""
    import dataclasses

    torch = _torch()
    meta, cfg, weights, wavs, hs, norms = golden_loader("mockingjay/tiny_albert")
    plain = dataclasses.replace(cfg, mj_share_layer=False)
    copies = {k: v for k, v in weights.items() if not k.startswith("encoder.layer.")}
    for l in range(cfg.encoder_layers):
        copies.update({k.replace("encoder.layer.0.", f"encoder.layer.{l}."): v for k, v in weights.items() if k.startswith("encoder.layer.0.")})
    dev = [torch.from_numpy(w).cuda() for w in wavs]
    a = _encoder(cfg, weights).forward(dev).clone()
    b = _encoder(plain, copies).forward(dev).clone()
    torch.cuda.synchronize()
    assert a.shape[0] == 4 and torch.equal(a, b)


def test_frame_arithmetic_of_the_library():
    from s3prl_amd.synth import named_config, synth_weights

    cfg = named_config("tiny_mockingjay")
    enc = _encoder(cfg, synth_weights(cfg, 0))
    assert [enc.num_frames(n) for n in (240000, 160000, 16000, 8000, 201, 200, 1)] == [1501, 1001, 101, 51, 2, 0, 0]
    assert enc.num_output_frames(160000) == 1001
    assert enc.valid_frames(8000, 16000) == cfg.valid_frames(8000, 16000) == 50 and enc.valid_frames(8000, 8000) == 51  # batch-dependent
    assert enc.downsample_rate() == 160 and enc.num_states() == 3
    kal = named_config("tiny_mockingjay_kaldi")
    enc = _encoder(kal, synth_weights(kal, 0))
    assert [enc.num_frames(n) for n in (16000, 400, 399)] == [98, 1, 0] and enc.valid_frames(2345, 4000) == 13


@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("cfg_name", ["tiny_mockingjay", "tiny_mockingjay_chunk3"])
def test_featurize_is_the_weighted_sum_of_the_states(cfg_name, normalize):
    from s3prl_amd import _lib
    from s3prl_amd.synth import named_config, synth_wavs, synth_weights

    torch = _torch()
    lib = _lib.load()
    cfg = named_config(cfg_name)
    enc = _encoder(cfg, synth_weights(cfg, 4))
    lengths = [4000, 2345, 3111] if cfg_name == "tiny_mockingjay" else [1500, 1100]
    wavs = [torch.from_numpy(w).cuda() for w in synth_wavs(lengths, 6)]
    hs = enc.forward(wavs).clone()
    NS, B, T, D = hs.shape
    for w in ([0.2, 0.3, 0.5], [0.0, 0.0, 1.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]):
        feat = enc.forward_featurized(wavs, w, normalize=normalize)
        want = torch.empty((B, T, D), device="cuda")
        wp = (C.c_float * 3)(*w)
        _lib.check(lib.s3enc_weighted_sum(_ptr(hs), B * T * D, 3, wp, int(normalize), B * T, D, _ptr(want), None), "s3enc_weighted_sum")
        torch.cuda.synchronize()
        assert O.rel_err(feat.cpu().numpy(), want.cpu().numpy()) < OP_TOL, w
    assert enc.status() == 0


@pytest.mark.parametrize("cfg_name", ["tiny_mockingjay", "tiny_mockingjay_chunk"])
def test_permutation_and_shard_are_bit_exact(cfg_name):
    """An utterance's rows depend on the padding length (its frame count does) and on nothing else of the batch: a two-shard forward
    padded to the global length reproduces the full batch bit for bit."""
    from s3prl_amd.synth import named_config, synth_wavs, synth_weights

    torch = _torch()
    cfg = named_config(cfg_name)
    enc = _encoder(cfg, synth_weights(cfg, 3))
    lengths = [4000, 2345, 800, 3111, 1999]
    wavs = [torch.from_numpy(w).cuda() for w in synth_wavs(lengths, 5)]
    full = enc.forward(wavs).clone()
    perm = [3, 0, 4, 2, 1]
    permuted = enc.forward([wavs[i] for i in perm]).clone()
    shards = [enc.forward(wavs[:2], n_max=max(lengths)).clone(), enc.forward(wavs[2:], n_max=max(lengths)).clone()]
    torch.cuda.synchronize()
    for j, i in enumerate(perm):
        assert torch.equal(permuted[:, j], full[:, i])
    assert torch.equal(torch.cat(shards, dim=1), full)


@pytest.mark.parametrize("cfg_name", ["tiny_mockingjay_chunk", "tiny_mockingjay_kaldi"])
def test_one_handle_at_three_lengths_equals_fresh_handles(cfg_name):
    from s3prl_amd.synth import named_config, synth_wavs, synth_weights

    torch = _torch()
    cfg = named_config(cfg_name)
    weights = synth_weights(cfg, 2)
    enc = _encoder(cfg, weights)
    for n in (4000, 16000, 2345):  # the workspace, the tables and (chunk) the sequence count grow and shrink
        wavs = [torch.from_numpy(w).cuda() for w in synth_wavs([n, max(900, n // 2)], n)]
        got = enc.forward(wavs).clone()
        fresh = _encoder(cfg, weights)
        want = fresh.forward(wavs).clone()
        torch.cuda.synchronize()
        assert got.shape[2] == cfg.num_frames(n) and torch.isfinite(got).all()
        assert torch.equal(got, want), n
        fresh.close()
    assert enc.status() == 0


def test_output_rows_outside_the_slab_are_not_written():
    """T = 10 in chunks of 3 pads every utterance to 12 rows inside: the two extra rows must never reach the caller's (B, 10, D) slab"""
    from s3prl_amd.synth import named_config, synth_wavs, synth_weights

    torch = _torch()
    cfg = named_config("tiny_mockingjay_chunk3")
    enc = _encoder(cfg, synth_weights(cfg, 1))
    wavs = [torch.from_numpy(w).cuda() for w in synth_wavs([1500, 1100], 2)]
    NS, B, T, D = 3, 2, 10, 128
    buf = torch.full((GUARD * D + NS * B * T * D + GUARD * D,), float("nan"), device="cuda")
    out = buf[GUARD * D:GUARD * D + NS * B * T * D].view(NS, B, T, D)
    enc.forward(wavs, out=out)
    torch.cuda.synchronize()
    assert torch.isfinite(out).all() and torch.isnan(buf[:GUARD * D]).all() and torch.isnan(buf[GUARD * D + NS * B * T * D:]).all()


REFUSALS = [("pre_layer_norm", 1, "pre_layer_norm"), ("hidden_act", 1, "hidden_act"), ("heads", 4, "must be 64"),
            ("input_dim", 18, "multiple of 4"), ("dtype", "bf16", "fp32 only"), ("dtype", "fp16x2", "fp32 only")]


@pytest.mark.parametrize("field, value, match", REFUSALS)
def test_create_refusals_are_error_codes_with_a_message(field, value, match):
    from s3prl_amd import _lib
    from s3prl_amd.synth import named_config, synth_weights

    _torch()
    lib = _lib.load()
    cfg = named_config("tiny_mockingjay")
    ccfg, mj = _lib.make_config(cfg, value if field == "dtype" else "fp32"), _lib.make_mockingjay_config(cfg)
    if field == "heads":
        ccfg.heads = value
    elif field != "dtype":
        setattr(mj, field, value)
    h = C.c_void_p()
    tensors = (_lib.S3Tensor * 1)()
    assert lib.s3enc_create_mockingjay(C.byref(ccfg), C.byref(mj), tensors, 0, 0, C.byref(h)) != 0 and not h.value
    assert match in lib.s3enc_last_error().decode()
    weights = synth_weights(cfg, 0)
    del weights["encoder.layer.1.output.LayerNorm.bias"]
    with pytest.raises(_lib.S3EncError, match="encoder.layer.1.output.LayerNorm.bias"):
        _encoder(cfg, weights)


def test_forward_refusals():
    from s3prl_amd import _lib
    from s3prl_amd._lib import S3EncError
    from s3prl_amd.synth import named_config, synth_wavs, synth_weights

    torch = _torch()
    cfg = named_config("tiny_mockingjay")
    enc = _encoder(cfg, synth_weights(cfg, 0))
    wavs = [torch.from_numpy(w).cuda() for w in synth_wavs([3000, 200, 210], 1)]
    with pytest.raises(S3EncError, match="feature_selection"):
        enc.forward(wavs[:1], selection="fairseq_layers")
    with pytest.raises(S3EncError, match="feature_selection"):
        enc.num_states("fairseq_layers_before_residual")
    with pytest.raises(ValueError, match="n <= 200"):
        enc.forward(wavs[:2])  # torch.stft's refusal, for ANY utterance of the batch
    with pytest.raises(ValueError, match="vq-wav2vec"):
        enc.forward(wavs[:1], aux={})
    lib = _lib.load()
    T = cfg.num_frames(3000)
    out = torch.full((3, 2, T, 128), float("nan"), device="cuda")
    ptrs = (C.c_void_p * 2)(wavs[0].data_ptr(), wavs[1].data_ptr())
    lens = (C.c_int64 * 2)(3000, 200)
    assert lib.s3enc_forward(enc._h, ptrs, lens, 2, 0, _ptr(out), 2 * T * 128, None) != 0 and b"200 samples" in lib.s3enc_last_error()
    # 210 samples beside 3000 are ONE frame inside this batch: no standard deviation for the CMVN
    ptrs = (C.c_void_p * 2)(wavs[0].data_ptr(), wavs[2].data_ptr())
    lens = (C.c_int64 * 2)(3000, 210)
    assert lib.s3enc_forward(enc._h, ptrs, lens, 2, 0, _ptr(out), 2 * T * 128, None) != 0 and b"single frame" in lib.s3enc_last_error()
    opts = _lib.S3ForwardOpts(_lib.SEL_HIDDEN, _lib.F16, 0, 0, None)
    assert lib.s3enc_forward_ex(enc._h, ptrs, lens, 1, 0, C.byref(opts), _ptr(out), 2 * T * 128, None) != 0
    assert b"S3ENC_F32" in lib.s3enc_last_error()
    torch.cuda.synchronize()
    assert torch.isnan(out).all()


def test_expert_returns_the_fixture_states(tmp_path, golden_loader):
    """hub entry -> checkpoint written from synth_weights -> expert forward, CPU waveforms in, CPU states out."""
    torch = _torch()
    import s3prl_amd.hub as amd
    from s3prl_amd.ckpt import save_checkpoint

    for name, entry in (("tiny_chunk", amd.tera_local), ("tiny_albert", amd.audio_albert_local), ("tiny_kaldi", amd.mockingjay_local)):
        meta, cfg, weights, wavs, hs, norms = golden_loader("mockingjay/" + name)
        path = str(tmp_path / "c.ckpt")
        save_checkpoint(path, cfg, weights)
        expert = entry(path)
        with torch.no_grad():
            out = expert([torch.from_numpy(w) for w in wavs])
        n = cfg.encoder_layers + 1
        assert set(out) == {"hidden_states", "last_hidden_state", "_hidden_states_info"} | {f"hidden_state_{i}" for i in range(n)}
        assert len(out["hidden_states"]) == n and out["last_hidden_state"] is out["hidden_states"][-1]
        assert all(h.device.type == "cpu" and list(h.shape) == meta["shape"] for h in out["hidden_states"])
        assert _score_live(out["hidden_states"], hs, meta["frames"], meta, name) < FP32_TOL
        assert expert.get_downsample_rates("hidden_states") == 160
