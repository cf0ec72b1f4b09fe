"""VGGish on the MI355X, every test through the C ABI: the family pinned to the reference's own outputs from the waveforms
(tests/golden/make_golden_vggish.py) — raw embeddings to FP32_TOL, quantised ones element by element against the float64
pre-rounding value — exact zero pad rows in both forms, the tiny configurations against float64 per example, the family against
its own ops bit for bit, an utterance alone against its rows in the batch, handle reuse, featurize, the expert and the refusals.
The full-size weights (72 M parameters) are synthesised once per weight seed of the fixtures (two: the generator moved vggish_eq
to the next seed) and one full-size handle of each form at a time serves the module."""

import ctypes as C

import numpy as np
import pytest

from oracle import encoder_oracle as O

import vggish_ref as R

pytestmark = pytest.mark.gpu

FP32_TOL = 1e-4   # the project's fixture bound
HALF_BAND = 0.02  # 63.75 x the error FP32_TOL allows on a PCA output of magnitude about 3
RAW = ["vggish/vggish_raw_pad"]
QUANT = ["vggish/" + n for n in ["vggish_pad", "vggish_one", "vggish_10s", "vggish_eq"]]
TINY = ["tiny_vggish", "tiny_vggish_odd"]


def _torch():
    import torch

    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _dev(x):
    return _torch().from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda()


def _encoder(cfg, weights):
    from s3prl_amd.encoder import HipEncoder

    return HipEncoder(cfg, weights, dtype="fp32")


def _wavs(lengths, seed, **kw):
    from s3prl_amd.synth import synth_wavs

    return synth_wavs(lengths, seed, **kw)


def _forward(enc, wavs, **kw):
    torch = _torch()
    out = enc.forward([torch.from_numpy(w).cuda() for w in wavs], **kw)
    torch.cuda.synchronize()
    return out


def _live(a, counts):
    return np.concatenate([a[b, :n] for b, n in enumerate(counts)])


class _Full(dict):
    """the full-size weights of ONE weight seed at a time, their float64 copy, and one handle per form.  The fixtures are listed
    so that the seed changes once (the generator moved vggish_eq to the next seed under its rule (d))."""

    def at(self, seed):
        from s3prl_amd.synth import named_config, synth_weights

        if self.get("seed") != seed:
            self.close()
            cfg, raw_cfg = named_config("vggish"), named_config("vggish_raw")
            weights = synth_weights(cfg, seed)
            self.update(seed=seed, cfg=cfg, raw_cfg=raw_cfg, weights=weights, w64={k: v.astype(np.float64) for k, v in weights.items()},
                        enc=_encoder(cfg, weights), raw=_encoder(raw_cfg, {k: v for k, v in weights.items() if not k.startswith("pca_")}),
                        ref={})
        return self

    def close(self):
        for k in ("enc", "raw"):
            if k in self:
                self.pop(k).close()
        self.clear()


@pytest.fixture(scope="module")
def full_at():
    box = _Full()
    yield box.at
    box.close()


@pytest.fixture
def full(full_at, golden_loader):
    """the handles at the seed most fixtures share"""
    return full_at(golden_loader(QUANT[0])[0]["weight_seed"])


def _ref64(full, name, wavs):
    if name not in full["ref"]:
        full["ref"][name] = R.forward(full["cfg"], full["w64"], wavs)
    return full["ref"][name]


# ---- pinned to the reference -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", RAW)
def test_raw_fixture_from_waveforms(name, golden_loader, full_at):
    """the embeddings within FP32_TOL of the reference's: whole, per utterance and on the norm; pad rows exact zeros"""
    meta, cfg, _, wavs, hs, norms = golden_loader(name)
    full = full_at(meta["weight_seed"])
    enc = full["raw"]
    assert enc.num_states() == 1 == meta["n_states"]
    out = _forward(enc, wavs)
    assert list(out.shape[1:]) == meta["shape"]
    g = out[0].cpu().numpy()
    errs = [O.rel_err(g, hs[0])] + [O.rel_err(g[b, :n], hs[0][b, :n]) for b, n in enumerate(meta["frames"])]
    print(f"{name}: whole / per-utterance rel-err {errs}")
    assert max(errs) < FP32_TOL, (name, errs)
    n = np.linalg.norm(g.astype(np.float64))
    assert abs(n - norms[0]) / norms[0] < FP32_TOL
    for b, cnt in enumerate(meta["frames"]):
        assert not g[b, cnt:].any(), "a pad row is not exact zeros"
    assert enc.status() == 0


@pytest.mark.parametrize("name", QUANT)
def test_quantised_fixture_from_waveforms(name, golden_loader, full_at):
    """every element q is a whole number in 0..255 with |q - pre64| <= 0.5 + HALF_BAND, pre64 the restatement's float64 pre-rounding
    value; at least 95 % of the live elements equal the reference's own quantised values; pad rows exact zeros"""
    meta, cfg, _, wavs, hs, _ = golden_loader(name)
    full = full_at(meta["weight_seed"])
    out = _forward(full["enc"], wavs)
    assert list(out.shape[1:]) == meta["shape"]
    g = out[0].cpu().numpy()
    counts = meta["frames"]
    ref = _ref64(full, name, wavs)
    assert ref["counts"] == counts
    q, pre, theirs = _live(g, counts).astype(np.float64), _live(ref["pre"], counts), _live(hs[0], counts)
    assert np.array_equal(q, np.rint(q)) and q.min() >= 0 and q.max() <= 255
    worst = np.abs(q - pre).max()
    same = (q == theirs).mean()
    print(f"{name}: worst |q - pre64| {worst:.4f}, equal to the reference's values on {same:.4f} of {q.size} live elements, "
          f"off by one on {(np.abs(q - theirs) == 1).mean():.4f}")
    assert worst <= 0.5 + HALF_BAND, (name, worst)
    assert same >= 0.95, (name, same)
    for b, cnt in enumerate(counts):
        assert not g[b, cnt:].any(), "a pad row is not exact zeros"
    assert full["enc"].status() == 0


def test_the_quantised_form_is_the_post_processor_of_the_raw_form(golden_loader, full):
    """both handles compute the same embedding (bit for bit: the tap), and the quantised state is its PCA / clamp / rint"""
    meta, cfg, weights, wavs, _, _ = golden_loader(QUANT[0])
    out = _forward(full["enc"], wavs)[0].cpu().numpy()
    emb_q = full["enc"].debug_tap("emb").reshape(-1, 128)
    raw = _forward(full["raw"], wavs)[0].cpu().numpy()
    counts = meta["frames"]
    assert np.array_equal(_live(raw, counts), emb_q)
    pre = R.pre_round(cfg, full["w64"], emb_q.astype(np.float64))
    assert np.abs(_live(out, counts) - pre).max() <= 0.5 + 1e-3  # the product itself in fp32: 128 terms of magnitude <= 3


# ---- the tiny configurations against float64, per example --------------------------------------------------------------------
@pytest.mark.parametrize("lengths", [[2800], [9000, 2800, 5599, 5600, 12000], [40000, 2801]])
@pytest.mark.parametrize("cfg_name", TINY)
def test_tiny_per_example_against_float64(cfg_name, lengths):
    from s3prl_amd.synth import named_config, synth_weights

    cfg, raw_cfg = named_config(cfg_name), named_config(cfg_name + "_raw")
    lengths = [max(n, cfg.vg_min_samples) for n in lengths]
    weights = synth_weights(cfg, 31)
    wavs = _wavs(lengths, 77 + len(lengths))
    ref = R.forward(cfg, weights, wavs)
    counts = ref["counts"]
    assert counts == [cfg.num_frames(n) for n in lengths]
    enc, raw = _encoder(cfg, weights), _encoder(raw_cfg, {k: v for k, v in weights.items() if not k.startswith("pca_")})
    try:
        g = _forward(raw, wavs)[0].cpu().numpy()
        logmel = raw.debug_tap("logmel").reshape(sum(counts), cfg.vg_example_frames + 2, cfg.vg_num_mel_bins + 2)
        ex = np.concatenate(ref["examples"])
        assert O.rel_err(logmel[:, 1:-1, 1:-1], ex) < FP32_TOL
        assert not logmel[:, 0].any() and not logmel[:, -1].any() and not logmel[:, :, 0].any() and not logmel[:, :, -1].any()
        errs = [O.rel_err(g[b, e], ref["emb"][b, e]) for b, n in enumerate(counts) for e in range(n)]
        print(f"{cfg_name} {lengths}: worst per-example rel-err {max(errs):.2e} over {len(errs)} examples")
        assert max(errs) < FP32_TOL, errs
        q = _forward(enc, wavs)[0].cpu().numpy()
        assert np.array_equal(q, np.rint(q)) and q.min() >= 0 and q.max() <= 255
        assert np.abs(_live(q, counts) - _live(ref["pre"], counts)).max() <= 0.5 + HALF_BAND
        for b, n in enumerate(counts):
            assert not g[b, n:].any() and not q[b, n:].any()
        assert enc.status() == 0 and raw.status() == 0
    finally:
        enc.close()
        raw.close()


# ---- bit for bit -----------------------------------------------------------------------------------------------------------------
def _conv(x, w, bias, pool, pad):
    from s3prl_amd import _lib

    torch = _torch()
    nb, H, W = x.shape[0], x.shape[1] - 2, x.shape[2] - 2
    N, Cin = w.shape[:2]
    Ho, Wo = H >> pool, W >> pool
    out = torch.zeros((nb, Ho + 2 * pad, Wo + 2 * pad, N), device="cuda")
    wh = np.ascontiguousarray(w, dtype=np.float32)
    _lib.check(_lib.load().s3enc_op_conv2d3x3(_ptr(x), C.c_void_p(wh.ctypes.data), _ptr(_dev(bias)), nb, H, W, Cin, N, 1, pool,
                                              _ptr(out), pad, N, None), "s3enc_op_conv2d3x3")
    return out


def _gemm(x, w, b):
    """s3enc_op_gemm in exact fp32, then ReLU"""
    from s3prl_amd import _lib

    torch = _torch()
    M, K = x.shape
    N = w.shape[0]
    out = torch.empty((M, N), device="cuda")
    x, wd, bd = x.contiguous(), _dev(w), _dev(b)
    _lib.check(_lib.load().s3enc_op_gemm(_lib.F32, _ptr(x), K, M * K, _ptr(wd), _ptr(bd), M, N, K, 1, 0, None, None, _ptr(out), None, N,
                                         M * N, None), "s3enc_op_gemm")
    torch.cuda.synchronize()
    return torch.relu(out)


@pytest.mark.parametrize("cfg_name", TINY)
def test_family_equals_its_own_ops(cfg_name):
    """from the front end's own examples (the tap) through s3enc_op_conv2d3x3 layer by layer and s3enc_op_gemm: the embedding bit
    for bit"""
    from s3prl_amd.synth import named_config, synth_weights

    torch = _torch()
    cfg = named_config(cfg_name + "_raw")
    weights = synth_weights(cfg, 41)
    wavs = _wavs([cfg.vg_min_samples * 3 + 17, cfg.vg_min_samples, cfg.vg_min_samples * 2 + 160], 5)
    enc = _encoder(cfg, weights)
    try:
        g = _forward(enc, wavs)[0]
        counts = [cfg.num_frames(len(w)) for w in wavs]
        x = _dev(enc.debug_tap("logmel").reshape(sum(counts), cfg.vg_example_frames + 2, cfg.vg_num_mel_bins + 2, 1))
        for i, (_, pool) in enumerate(cfg.vg_layers):
            p = f"features.{cfg.vg_seq_index(i)}."
            x = _conv(x, weights[p + "weight"], weights[p + "bias"], int(pool), 0 if i == len(cfg.vg_layers) - 1 else 1)
        x = x.reshape(x.shape[0], -1)
        for i in (0, 2, 4):
            x = _gemm(x, weights[f"embeddings.{i}.weight"], weights[f"embeddings.{i}.bias"])
        o = 0
        for b, n in enumerate(counts):
            assert torch.equal(g[b, :n], x[o:o + n]), (cfg_name, b)
            o += n
    finally:
        enc.close()


def test_an_utterance_alone_equals_its_rows_in_the_batch_and_forward_twice(full):
    torch = _torch()
    wavs = _wavs([48123, 15600, 40000], 801)
    for enc in (full["enc"], full["raw"]):
        a = _forward(enc, wavs)[0].clone()
        assert torch.equal(_forward(enc, wavs)[0], a), "forward twice differs"
        for b, w in enumerate(wavs):
            alone = _forward(enc, [w])[0]
            n = alone.shape[1]
            assert torch.equal(alone[0], a[b, :n]) and not a[b, n:].any(), ("alone", b)
        rev = _forward(enc, wavs[::-1])[0]
        for b in range(3):
            assert torch.equal(rev[2 - b], a[b])


@pytest.mark.parametrize("cfg_name", TINY)
def test_one_handle_at_several_lengths_equals_fresh_handles(cfg_name):
    from s3prl_amd.synth import named_config, synth_weights

    torch = _torch()
    cfg = named_config(cfg_name)
    weights = synth_weights(cfg, 51)
    m = cfg.vg_min_samples
    batches = [[m * 9, m], [m], [m * 30 + 5, m * 2, m * 7 - 1], [m * 2]]
    one = _encoder(cfg, weights)
    try:
        for i, lengths in enumerate(batches):
            wavs = _wavs(lengths, 60 + i)
            got = _forward(one, wavs).clone()
            fresh = _encoder(cfg, weights)
            try:
                assert torch.equal(_forward(fresh, wavs), got), lengths
            finally:
                fresh.close()
    finally:
        one.close()


def test_a_larger_n_max_adds_zero_rows(full):
    torch = _torch()
    wavs = _wavs([31000, 15600], 9)
    a = _forward(full["enc"], wavs)[0]
    b = _forward(full["enc"], wavs, n_max=50000)[0]
    assert a.shape[1] == 2 and b.shape[1] == 3
    assert torch.equal(b[:, :2], a) and not b[:, 2:].any()


def test_misaligned_waveforms(full):
    """a waveform that starts 4 bytes into a 16-byte line is staged, same bits"""
    torch = _torch()
    w = _wavs([15600 + 321], 13)[0]
    buf = torch.zeros(len(w) + 8, device="cuda")
    buf[1:1 + len(w)] = torch.from_numpy(w).cuda()
    a = full["raw"].forward([torch.from_numpy(w).cuda()])
    b = full["raw"].forward([buf[1:1 + len(w)]])
    torch.cuda.synchronize()
    assert torch.equal(a, b)


# ---- the handle's arithmetic, featurize, the expert, refusals ---------------------------------------------------------------------
def test_frame_arithmetic_of_the_library(full):
    enc = full["enc"]
    for n, want in [(399, 0), (400, 0), (15599, 0), (15600, 1), (30959, 1), (30960, 2), (160000, 10), (100000, 6)]:
        assert enc.num_frames(n) == want == full["cfg"].num_frames(n) == R.num_examples(full["cfg"], n), n
        assert enc.num_output_frames(n) == want
    assert enc.valid_frames(15600, 48123) == 1 and enc.valid_frames(48123, 48123) == 3 and enc.valid_frames(48123, 15600) == 1
    assert enc.downsample_rate() == 16000
    assert enc.num_states() == 1


def test_featurizer_weighted_sum_over_the_one_state(full):
    torch = _torch()
    wavs = _wavs([31000, 15600], 21)
    dev = [torch.from_numpy(w).cuda() for w in wavs]
    for enc in (full["enc"], full["raw"]):
        hs = enc.forward(dev)
        got = enc.forward_featurized(dev, [0.75])
        torch.cuda.synchronize()
        assert torch.equal(got, 0.75 * hs[0])
        zero = enc.forward_featurized(dev, [0.0])
        torch.cuda.synchronize()
        assert not zero.any()


def test_expert_returns_the_fixture_states(golden_loader, full):
    from s3prl_amd.upstream.vggish.expert import UpstreamExpert

    torch = _torch()
    meta, cfg, weights, wavs, hs, _ = golden_loader(QUANT[0])
    sd = {k: torch.from_numpy(v) for k, v in weights.items() if not k.startswith("pca_")}
    ckpt = {"vggish": sd, "pca": {"pca_eigen_vectors": weights["pca_eigen_vectors"], "pca_means": weights["pca_means"].reshape(-1, 1)}}
    expert = UpstreamExpert(ckpt=ckpt, postprocess=True, progress=False)
    assert expert.get_downsample_rates("hidden_states") == 16000 and expert.cfg == cfg
    out = expert([torch.from_numpy(w) for w in wavs])  # CPU waveforms: encoded on the GPU, returned on the CPU
    assert len(out["hidden_states"]) == 1 and out["last_hidden_state"] is out["hidden_states"][0]
    g = out["hidden_states"][0]
    assert g.device.type == "cpu" and list(g.shape) == meta["shape"]
    assert torch.equal(g.cuda(), _forward(full["enc"], wavs)[0])
    counts = meta["frames"]
    assert (_live(g.numpy(), counts) == _live(hs[0], counts)).mean() >= 0.95


def test_refusals(full):
    from s3prl_amd import _lib
    from s3prl_amd.synth import named_config, synth_weights

    torch = _torch()
    enc = full["enc"]
    wavs = [torch.from_numpy(w).cuda() for w in _wavs([20000, 15599], 3)]
    with pytest.raises(ValueError, match=r"utterance 1 has 15599 samples"):
        enc.forward(wavs)
    # the same through the C entry point: by index and length
    lib = _lib.load()
    out = torch.empty((1, 2, 1, 128), device="cuda")
    ptrs = (C.c_void_p * 2)(*[w.data_ptr() for w in wavs])
    lens = (C.c_int64 * 2)(20000, 15599)
    opts = _lib.S3ForwardOpts(_lib.SELECTIONS[None], _lib.F32, 0, 0, None)
    assert lib.s3enc_forward_ex(enc._h, ptrs, lens, 2, 0, C.byref(opts), _ptr(out), 2 * 128, None) != 0
    assert b"utterance 1 has 15599 samples" in lib.s3enc_last_error()
    with pytest.raises(_lib.S3EncError, match="feature_selection is not defined for VGGish"):
        enc.num_states("fairseq_layers")
    opts16 = _lib.S3ForwardOpts(_lib.SELECTIONS[None], _lib.BF16, 0, 0, None)
    lens1 = (C.c_int64 * 1)(20000)
    assert lib.s3enc_forward_ex(enc._h, ptrs, lens1, 1, 0, C.byref(opts16), _ptr(out), 128, None) != 0
    assert b"out_dtype must be S3ENC_F32 for a VGGish handle" in lib.s3enc_last_error()
    cfg = named_config("tiny_vggish")
    with pytest.raises(ValueError, match="VGGish is built for compute dtype fp32 only; bf16 is not built"):
        from s3prl_amd.encoder import HipEncoder

        HipEncoder(cfg, synth_weights(cfg, 1), dtype="bf16")
