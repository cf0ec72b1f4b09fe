"""wav2vec / vq-wav2vec on the MI355X, every test through the C ABI: the reference's own outputs (tests/golden/make_golden_wav2vec.py)
including exact code ids, the two new kernels against float64, batch invariances, featurize, and the refusals."""

import ctypes as C
import itertools
import os

import numpy as np
import pytest

from oracle import encoder_oracle as O

import wav2vec_ref as R

pytestmark = pytest.mark.gpu

FP32_TOL = 1e-4
OP_TOL = 2e-5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = ["wav2vec/" + n for n in ["wav2vec_tiny_pad", "wav2vec_tiny_eq", "wav2vec_tiny_t1", "wav2vec_tiny_zeropad_noaffine",
                                     "vq_gumbel_tiny_pad", "vq_kmeans_tiny_pad", "wav2vec_large_pseudo"]]


def _torch():
    import torch

    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _dev(x, dtype=np.float32):
    torch = _torch()
    return torch.from_numpy(np.ascontiguousarray(x, dtype=dtype)).cuda()


def _encoder(cfg, weights, dtype="fp32"):
    from s3prl_amd.encoder import HipEncoder

    return HipEncoder(cfg, weights, dtype=dtype)


@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_fp32(name, golden_loader):
    torch = _torch()
    meta, cfg, weights, wavs, hs, norms = golden_loader(name)
    enc = _encoder(cfg, weights)
    assert enc.num_states() == len(hs) == len(cfg.agg_layers) + 1
    aux = {} if cfg.vq_type != "none" else None
    out = enc.forward([torch.from_numpy(w).cuda() for w in wavs], aux=aux)
    torch.cuda.synchronize()
    assert list(out.shape[1:]) == meta["shape"]
    ts, cs = meta["t_stride"], meta["c_stride"]
    errs = [O.rel_err(out[l].cpu().numpy()[:, ::ts, ::cs], hs[l]) for l in range(len(hs))]
    print(f"{name}: per-state rel-err {['%.2e' % e for e in errs]}")
    assert max(errs) < FP32_TOL, f"{name}: per-state rel-err {['%.2e' % e for e in errs]}"
    for l in range(len(hs)):
        n = np.linalg.norm(out[l].cpu().numpy().astype(np.float64))
        assert abs(n - norms[l]) / norms[l] < FP32_TOL
    if aux is not None:
        z = np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"))
        ids = aux["codeids"].cpu().numpy()
        assert ids.dtype == np.int64 and ids.shape == z["codeids"].shape
        assert np.array_equal(ids, z["codeids"]), f"{name}: {(ids != z['codeids']).sum()} of {ids.size} code ids differ"
        cw = aux["codewords"].cpu().numpy()
        assert O.rel_err(cw[:, ::ts, ::cs], z["codewords"]) < FP32_TOL
        assert abs(np.linalg.norm(cw.astype(np.float64)) - z["codewords_norm"][0]) / z["codewords_norm"][0] < FP32_TOL
    assert enc.status() == 0


def test_frame_arithmetic_of_the_library():
    from s3prl_amd.synth import named_config, synth_weights

    cfg = named_config("tiny_wav2vec")
    enc = _encoder(cfg, synth_weights(cfg, 0))
    assert [enc.num_frames(n) for n in (160000, 465, 4000)] == [998, 1, 23]
    assert [enc.valid_frames(n, 160000) for n in (160000, 465, 4000)] == [998, 1, 23]
    assert enc.downsample_rate() == 160 and enc.num_states() == 5


# launch_gn1_apply picks gn1_apply_kernel<1..4> by ceil((C / 4) / 64): 64 -> 1, 512 -> 2 (the released width), 544 and 768 -> 3,
# 1024 -> 4; 32, 96, 288 and 544 leave lanes of the last pass without a channel quad
GN1_SHAPES = [(T, C_) for C_ in (64, 512) for T in (1, 17, 31, 49, 998)] + \
             [(T, C_) for C_ in (32, 96, 288, 544, 768, 1024) for T in (1, 17, 49)]


@pytest.mark.parametrize("T,C_", GN1_SHAPES)
def test_gn1_apply_op(T, C_):
    """GroupNorm(1, C) + ReLU [+ skip] [+ log] into the padded operand, the state slot and the Featurizer term, against float64:
    pad rows 0 / 1 / 12 of both kinds, with and without residual, log compression and a (plain / normalised) Featurizer term."""
    from s3prl_amd import _lib

    torch = _torch()
    lib = _lib.load()
    B = 3
    rng = np.random.default_rng(1000 * C_ + T)
    x = (rng.standard_normal((B, T, C_)) * rng.uniform(0.5, 2.0, (B, 1, 1)) + rng.uniform(-1, 1, (B, 1, 1))).astype(np.float32)
    gamma = (1 + 0.1 * rng.standard_normal(C_)).astype(np.float32)
    beta = (0.05 * rng.standard_normal(C_)).astype(np.float32)
    res = rng.standard_normal((B, T, C_)).astype(np.float32)
    acc0 = rng.standard_normal((B, T, C_)).astype(np.float32)
    dx, dg, db, dres = _dev(x), _dev(gamma), _dev(beta), _dev(res)
    scale, aw = float(np.sqrt(0.5)), 0.37
    refs = {}
    worst = 0.0
    for case, (pad, pad_zero, use_res, log, accm) in enumerate(itertools.product([0, 1, 12], [0, 1], [0, 1], [0, 1], [0, 1, 2])):
        affine = case % 3 != 2  # every third case: non_affine_group_norm
        key = (use_res, log, affine)
        if key not in refs:
            refs[key] = R.gn1_apply(x.astype(np.float64), gamma.astype(np.float64) if affine else None,
                                    beta.astype(np.float64) if affine else None, res.astype(np.float64) if use_res else None,
                                    np.sqrt(0.5), bool(log))
        y = refs[key]
        dst = torch.full((B, pad + T, C_), float("nan"), device="cuda")
        state = torch.full((B, T, C_), float("nan"), device="cuda")
        init = case % 2
        acc = _dev(acc0) if accm else None
        _lib.check(lib.s3enc_op_gn1_apply(_ptr(dx), _ptr(dg) if affine else None, _ptr(db) if affine else None,
                                          _ptr(dres) if use_res else None, scale, log, B, T, C_, pad, pad_zero, _ptr(dst), _ptr(state),
                                          _ptr(acc), aw, int(accm == 2), init, None), "s3enc_op_gn1_apply")
        torch.cuda.synchronize()
        d = dst.cpu().numpy()
        worst = max(worst, O.rel_err(state.cpu().numpy(), y), O.rel_err(d[:, pad:], y))
        if pad:
            want = np.zeros((B, pad, C_)) if pad_zero else np.repeat(y[:, :1], pad, axis=1)
            assert np.array_equal(d[:, :pad], np.repeat(d[:, pad:pad + 1], pad, axis=1) if not pad_zero else want)
            assert np.abs(d[:, :pad] - want).max() <= OP_TOL * max(1.0, np.abs(want).max())
        if accm:
            yn = (y - y.mean(-1, keepdims=True)) / np.sqrt(y.var(-1, keepdims=True) + 1e-5) if accm == 2 else y
            want = (0.0 if init else acc0.astype(np.float64)) + aw * yn
            worst = max(worst, O.rel_err(acc.cpu().numpy(), want))
    print(f"gn1_apply T={T} C={C_}: worst rel-err {worst:.2e}")
    assert worst < OP_TOL


@pytest.mark.parametrize("rows", [1, 63, 65, 998])
@pytest.mark.parametrize("G", [1, 2])
@pytest.mark.parametrize("V", [32, 320])
def test_argmax_gather_op(V, G, rows):
    """int64 index of the largest score per (row, group), ties to the lowest index (torch.max), and the gathered codeword."""
    Dv = 24
    rng = np.random.default_rng(V * 7 + G * 3 + rows)
    sc = rng.standard_normal((rows, G, V)).astype(np.float32)
    # planted exact ties of the maximum: two (three) equal largest values, the lowest index must win — also across the lanes'
    # strided walk (indices 64 apart land in the same lane for V = 320)
    for r in range(0, rows, 3):
        g = r % G
        a, b = sorted(rng.choice(V, size=2, replace=False))
        sc[r, g, a] = sc[r, g, b] = 10.0
        if V > 64 and r % 2 == 0:
            sc[r, g, (a + 64) % V] = 10.0
    _check_argmax_gather(sc, Dv, rng)


def _check_argmax_gather(sc, Dv, rng):
    from s3prl_amd import _lib

    torch = _torch()
    lib = _lib.load()
    rows, G, V = sc.shape
    for shared in (0, 1):
        table = rng.standard_normal((1 if shared else G, V, Dv)).astype(np.float32)
        ids = torch.full((rows, G), -1, dtype=torch.int64, device="cuda")
        out = torch.full((rows, G * Dv), float("nan"), device="cuda")
        dsc, dtab = _dev(sc), _dev(table)
        _lib.check(lib.s3enc_op_argmax_gather(_ptr(dsc), _ptr(dtab), shared, rows, G, V, Dv, _ptr(ids), _ptr(out), None),
                   "s3enc_op_argmax_gather")
        torch.cuda.synchronize()
        want = sc.argmax(-1)  # numpy: the first occurrence
        assert np.array_equal(ids.cpu().numpy(), want)
        cw = np.stack([table[0 if shared else g][want[:, g]] for g in range(G)], axis=1).reshape(rows, G * Dv)
        assert np.array_equal(out.cpu().numpy(), cw)  # a gather: exact


@pytest.mark.parametrize("rows", [2, 7])
@pytest.mark.parametrize("Dv", [4, 64, 200])
@pytest.mark.parametrize("G", [4, 16])
@pytest.mark.parametrize("V", [1, 5, 63, 64, 65])
def test_argmax_gather_op_lane_edges(V, G, Dv, rows):
    """V below, at and just past one wave (idle lanes carry the INT_MAX sentinel through the shuffle reduction; V = 1: all but
    lane 0), more groups than a workgroup's four waves, codewords of less than, exactly and more than one pass of the gather loop.
    Planted in every case: a tie between index 0 and the last index (0 wins), a row of all-equal scores (0 wins), a largest value
    at the last index alone, and all scores -inf but one."""
    rng = np.random.default_rng(((V * 17 + G) * 201 + Dv) * 8 + rows)
    sc = rng.standard_normal((rows, G, V)).astype(np.float32)
    want = {}
    sc[0, 0, 0] = sc[0, 0, V - 1] = 10.0            # first and last index tie (V = 1: the only one)
    want[(0, 0)] = 0
    sc[1, G - 1, :] = -0.75                          # all equal
    want[(1, G - 1)] = 0
    sc[rows - 1, 1, V - 1] = 11.0                    # the last index alone: the last lane that holds a value
    want[(rows - 1, 1)] = V - 1
    sc[0, 2, :] = -np.inf                            # every score -inf but one: the initial best value is -inf too
    sc[0, 2, V // 2] = -3.0
    want[(0, 2)] = V // 2
    sc[1, 0, :] = 5.0                                # all equal but a smaller first entry: the second index wins
    sc[1, 0, 0] = 4.0
    want[(1, 0)] = min(1, V - 1)
    ref = sc.argmax(-1)
    for (r, g), v in want.items():
        assert ref[r, g] == v
    _check_argmax_gather(sc, Dv, rng)


@pytest.mark.parametrize("cfg_name", ["tiny_wav2vec", "tiny_vq_wav2vec_kmeans"])
def test_permutation_and_shard_are_bit_exact(cfg_name):
    torch = _torch()
    from s3prl_amd.synth import named_config, synth_wavs, synth_weights

    cfg = named_config(cfg_name)
    enc = _encoder(cfg, synth_weights(cfg, 3))
    vq = cfg.vq_type != "none"
    lengths = [4000, 2345, 800, 3111, 1999]
    wavs = [torch.from_numpy(w).cuda() for w in synth_wavs(lengths, 5)]

    def run(ws, n_max=None):
        aux = {} if vq else None
        hs = enc.forward(ws, n_max=n_max, aux=aux).clone()
        return hs, (aux["codeids"].clone(), aux["codewords"].clone()) if vq else None

    full, fa = run(wavs)
    perm = [3, 0, 4, 2, 1]
    permuted, pa = run([wavs[i] for i in perm])
    shard, sa = run(wavs[2:4], n_max=max(lengths))
    torch.cuda.synchronize()
    for j, i in enumerate(perm):
        assert torch.equal(permuted[:, j], full[:, i])
        if vq:
            assert torch.equal(pa[0][j], fa[0][i]) and torch.equal(pa[1][j], fa[1][i])
    assert torch.equal(shard, full[:, 2:4])
    if vq:
        assert torch.equal(sa[0], fa[0][2:4]) and torch.equal(sa[1], fa[1][2:4])
    # the batch's longest utterance is part of the result (GroupNorm over the padded time): alone, the utterance differs
    alone, _ = run(wavs[1:2])
    assert not torch.equal(alone[-1, 0, :alone.shape[2]], full[-1, 1, :alone.shape[2]])
    assert enc.status() == 0


@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("cfg_name", ["tiny_wav2vec", "tiny_vq_wav2vec_gumbel"])
def test_featurize_is_the_weighted_sum_of_the_states(cfg_name, normalize):
    torch = _torch()
    from s3prl_amd.synth import named_config, synth_wavs, synth_weights

    cfg = named_config(cfg_name)
    enc = _encoder(cfg, synth_weights(cfg, 4))
    wavs = [torch.from_numpy(w).cuda() for w in synth_wavs([4000, 2345, 3111], 6)]
    hs = enc.forward(wavs).clone()
    w = np.random.default_rng(7).standard_normal(hs.shape[0]).astype(np.float32)
    w = np.exp(w) / np.exp(w).sum()
    w[1] = 0.0  # an unselected state
    feat = enc.forward_featurized(wavs, list(w), normalize=normalize)
    torch.cuda.synchronize()
    h = hs.cpu().numpy().astype(np.float64)
    if normalize:
        h = (h - h.mean(-1, keepdims=True)) / np.sqrt(h.var(-1, keepdims=True) + 1e-5)
    ref = np.tensordot(w.astype(np.float64), h, axes=1)
    assert O.rel_err(feat.cpu().numpy(), ref) < 1e-5
    assert enc.status() == 0


def test_expert_returns_the_reference_keys(tmp_path, golden_loader):
    """hub entry -> checkpoint -> expert forward: z, c, default, codewords, codeids and the hook-added entries."""
    torch = _torch()
    import s3prl_amd.hub as amd
    from s3prl_amd.ckpt import save_checkpoint

    meta, cfg, weights, wavs, hs, norms = golden_loader("wav2vec/vq_gumbel_tiny_pad")
    path = str(tmp_path / "c.pt")
    save_checkpoint(path, cfg, weights)
    expert = amd.vq_wav2vec_custom(ckpt=path)
    with torch.no_grad():
        out = expert([torch.from_numpy(w) for w in wavs])  # CPU waveforms: encoded on the GPU, returned on the CPU
    assert set(out) >= {"z", "c", "default", "codewords", "codeids", "hidden_states", "last_hidden_state", "hidden_state_0",
                        "hidden_state_4", "_hidden_states_info"}
    assert len(out["hidden_states"]) == 5 and out["c"] is out["default"]
    assert torch.equal(out["z"], out["hidden_states"][0]) and torch.equal(out["c"], out["hidden_states"][-1])
    z = np.load(os.path.join(ROOT, "tests", "golden", "wav2vec", "vq_gumbel_tiny_pad.npz"))
    assert out["codeids"].dtype == torch.int64 and np.array_equal(out["codeids"].numpy(), z["codeids"])
    assert O.rel_err(out["last_hidden_state"].numpy(), hs[-1]) < FP32_TOL
    assert out["codewords"].device.type == "cpu" and tuple(out["codewords"].shape) == (3, 23, 64)
    plain = amd.wav2vec_local(ckpt=path)  # the same checkpoint through the wav2vec names
    assert plain.get_downsample_rates("c") == 160


@pytest.mark.parametrize("dtype", ["bf16", "fp16", "fp16x2", "fp32x3"])
def test_non_fp32_modes_are_refused(dtype):
    from s3prl_amd import _lib
    from s3prl_amd.synth import named_config, synth_weights

    cfg = named_config("tiny_wav2vec")
    with pytest.raises(ValueError, match=dtype):
        _encoder(cfg, synth_weights(cfg, 0), dtype)
    lib = _lib.load()
    ccfg, w2v = _lib.make_config(cfg, dtype), _lib.make_wav2vec_config(cfg)
    h = C.c_void_p()
    tensors = (_lib.S3Tensor * 1)()
    assert lib.s3enc_create_ex(C.byref(ccfg), C.byref(w2v), tensors, 0, 0, C.byref(h)) != 0
    err = lib.s3enc_last_error()
    assert b"fp32 only" in err and dtype.encode() in err


def test_feature_selection_and_stray_aux_are_refused():
    from s3prl_amd._lib import S3EncError
    from s3prl_amd.synth import named_config, synth_wavs, synth_weights

    torch = _torch()
    cfg = named_config("tiny_wav2vec")
    enc = _encoder(cfg, synth_weights(cfg, 0))
    wavs = [torch.from_numpy(w).cuda() for w in synth_wavs([3000], 1)]
    with pytest.raises(S3EncError, match="feature_selection"):
        enc.forward(wavs, selection="fairseq_layers")
    with pytest.raises(ValueError, match="vq-wav2vec"):
        enc.forward(wavs, aux={})
    with pytest.raises(ValueError, match="receptive field"):
        enc.forward([wavs[0][:464]])
