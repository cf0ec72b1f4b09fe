"""wav2vec 2.0 Conformer encoders (rel_pos / rope) on the MI355X: the reference's own outputs (tests/golden/make_golden_conformer.py),
the two new kernels through the C ABI against float64, batch invariances, featurize, and the refusal of the modes not built."""

import ctypes as C

import numpy as np
import pytest

from oracle import encoder_oracle as O

import conformer_ref as R

pytestmark = pytest.mark.gpu

FP32_TOL = 1e-4
OP_TOL = 2e-5

FIXTURES = ["conformer/" + n for n in ["conformer_relpos_tiny_pad", "conformer_rope_tiny_pad", "conformer_rope_postln_tiny_pad", "conformer_relpos_tiny_eq",
            "conformer_relpos_tiny_t49", "conformer_relpos_large_pseudo", "conformer_rope_large_pseudo"]]


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
    out = enc.forward([torch.from_numpy(w).cuda() for w in wavs])
    torch.cuda.synchronize()
    ts, cs = meta["t_stride"], meta["c_stride"]
    errs = [O.rel_err(out[l].cpu().numpy()[:, ::ts, ::cs], hs[l]) for l in range(len(hs))]
    assert max(errs) < FP32_TOL, f"{name}: per-state rel-err {['%.2e' % e for e in errs]}"
    for l in range(len(hs)):
        n = np.linalg.norm(out[l].cpu().numpy().astype(np.float64))
        assert abs(n - norms[l]) / norms[l] < FP32_TOL
    assert enc.status() == 0


@pytest.mark.parametrize("T", [1, 17, 31, 49, 499, 749])
def test_conv_module_op(T):
    """GLU -> depthwise conv (zero outside each utterance's T rows) -> folded BatchNorm -> swish, against float64."""
    B, D, K = (3, 128, 31) if T < 499 else (2, 256, 31)
    _check_conv_module(B, T, D, K, np.random.default_rng(T))


@pytest.mark.parametrize("T", [1, 7, 8, 9, 127, 128, 129, 136])
@pytest.mark.parametrize("D", [64, 192])
@pytest.mark.parametrize("K", [1, 3, 7, 15, 63])
def test_conv_module_op_kernel_and_tile_edges(K, D, T):
    """Every kernel width class (1: no window; 63: the largest, 63.25 KiB of LDS) at one and three channel blocks, with T around
    the 8 frames of a thread and the 128 frames of a workgroup: the window's zero rows on both sides of every utterance."""
    _check_conv_module(3, T, D, K, np.random.default_rng((K * 1000 + D) * 1000 + T))


def _check_conv_module(B, T, D, K, rng):
    from s3prl_amd import _lib

    torch = _torch()
    lib = _lib.load()
    x = rng.standard_normal((B, T, 2 * D)).astype(np.float32)
    dw = (rng.standard_normal((D, K)) / np.sqrt(K)).astype(np.float32)
    bn = dict(weight=1 + 0.1 * rng.standard_normal(D), bias=0.05 * rng.standard_normal(D), running_mean=0.2 * rng.standard_normal(D),
              running_var=rng.uniform(0.5, 2.0, D))
    sc = bn["weight"] / np.sqrt(bn["running_var"] + 1e-5)
    taps = (dw * sc[:, None]).astype(np.float32)
    shift = (bn["bias"] - bn["running_mean"] * sc).astype(np.float32)
    out = torch.full((B * T, D), float("nan"), device="cuda")
    dx, dtaps, dshift = _dev(x), _dev(taps), _dev(shift)  # (held: a temporary's memory would be reused by the next argument)
    _lib.check(lib.s3enc_op_conformer_conv(_ptr(dx), _ptr(dtaps), _ptr(dshift), B, T, D, K, _ptr(out), None),
               "s3enc_op_conformer_conv")
    torch.cuda.synchronize()
    ref = R.glu_dw_bn_swish(x.astype(np.float64), dw.astype(np.float64), bn)
    got = out.cpu().numpy().reshape(B, T, D)
    assert O.rel_err(got, ref) < OP_TOL
    assert max(O.rel_err(got[b], ref[b]) for b in range(B)) < OP_TOL  # per utterance


@pytest.mark.parametrize("T", [1, 17, 31, 49, 499, 749])
def test_relpos_attention_op(T):
    """score = q.k + (q + qadd).P[(j - i) + T - 1], masked softmax, ragged valid — against float64."""
    B, H = (3, 2) if T < 499 else (2, 4)
    _check_relpos_attention(B, T, H, np.random.default_rng(100 + T))


@pytest.mark.parametrize("T", [63, 64, 65])
@pytest.mark.parametrize("H", [1, 3])
def test_relpos_attention_op_row_tile_edges(H, T):
    """One head and an odd head count (D = 64, 192) with T one short of, at and one past two 32-key tiles."""
    _check_relpos_attention(3, T, H, np.random.default_rng(7000 + 10 * T + H))


def _check_relpos_attention(B, T, H, rng):
    from s3prl_amd import _lib

    torch = _torch()
    lib = _lib.load()
    D = 64 * H
    qkv = rng.standard_normal((B, T, 3 * D)).astype(np.float32)
    qkv[..., :D] *= 0.3
    P = (0.5 * rng.standard_normal((2 * T - 1, D))).astype(np.float32)
    qadd = (0.1 * rng.standard_normal((H, 64))).astype(np.float32)
    valid = [T] + [max(1, (T * (b + 1)) // (B + 1)) for b in range(1, B)]
    out = torch.empty((B * T, D), device="cuda")
    dvalid = _dev(np.array(valid, dtype=np.int32), np.int32)
    dqkv, dP, dqadd = _dev(qkv), _dev(P), _dev(qadd)
    _lib.check(lib.s3enc_op_relpos_attention(_ptr(dqkv), _ptr(out), _ptr(dvalid), B, T, H, _ptr(dP), _ptr(dqadd), None),
               "s3enc_op_relpos_attention")
    torch.cuda.synchronize()
    x = qkv.astype(np.float64)
    sh = lambda t: t.reshape(B, T, H, 64).transpose(0, 2, 1, 3)  # noqa: E731
    q, k, v = sh(x[..., :D]), sh(x[..., D:2 * D]), sh(x[..., 2 * D:])
    s = R.relpos_scores(q, k, P.astype(np.float64).reshape(2 * T - 1, H, 64), qadd.astype(np.float64))
    ref = (R.softmax_masked(s, valid) @ v).transpose(0, 2, 1, 3).reshape(B, T, D)
    assert O.rel_err(out.cpu().numpy().reshape(B, T, D), ref) < OP_TOL


@pytest.mark.parametrize("dtype", ["bf16", "fp16", "fp16x2", "fp32x3"])
@pytest.mark.parametrize("cfg_name", ["tiny_conformer_rope", "tiny_conformer_relpos"])
def test_non_fp32_modes_are_refused(cfg_name, dtype):
    """Only the exact-fp32 Conformer is built: the other modes are a ValueError naming the mode, and the library refuses them too."""
    from s3prl_amd import _lib
    from s3prl_amd.synth import named_config, synth_weights

    cfg = named_config(cfg_name)
    weights = synth_weights(cfg, 0)
    with pytest.raises(ValueError, match=dtype):
        _encoder(cfg, weights, dtype)
    lib = _lib.load()
    ccfg = _lib.make_config(cfg, dtype)
    h = C.c_void_p()
    tensors = (_lib.S3Tensor * 1)()
    assert lib.s3enc_create(C.byref(ccfg), tensors, 0, 0, C.byref(h)) != 0
    assert b"fp32 only" in lib.s3enc_last_error()


@pytest.mark.parametrize("cfg_name", ["tiny_conformer_relpos", "tiny_conformer_rope_postln"])
def test_permutation_and_shard_are_bit_exact(cfg_name):
    torch = _torch()
    from s3prl_amd.synth import named_config, synth_wavs, synth_weights

    cfg = named_config(cfg_name)
    enc = _encoder(cfg, synth_weights(cfg, 3))
    lengths = [4000, 2345, 800, 3111, 1999]
    wavs = [torch.from_numpy(w).cuda() for w in synth_wavs(lengths, 5)]
    full = enc.forward(wavs).clone()
    perm = [3, 0, 4, 2, 1]
    permuted = enc.forward([wavs[i] for i in perm]).clone()
    shard = enc.forward(wavs[2:4], n_max=max(lengths)).clone()
    torch.cuda.synchronize()
    for j, i in enumerate(perm):
        assert torch.equal(permuted[:, j], full[:, i])
    assert torch.equal(shard, full[:, 2:4])
    assert enc.status() == 0


@pytest.mark.parametrize("normalize", [False, True])
def test_featurize_is_the_weighted_sum_of_the_states(normalize):
    torch = _torch()
    from s3prl_amd.synth import named_config, synth_wavs, synth_weights

    cfg = named_config("tiny_conformer_rope")
    enc = _encoder(cfg, synth_weights(cfg, 4))
    wavs = [torch.from_numpy(w).cuda() for w in synth_wavs([4000, 2345, 3111], 6)]
    hs = enc.forward(wavs).clone()
    w = np.random.default_rng(7).standard_normal(hs.shape[0]).astype(np.float32)
    w = np.exp(w) / np.exp(w).sum()
    feat = enc.forward_featurized(wavs, list(w), normalize=normalize)
    torch.cuda.synchronize()
    h = hs.cpu().numpy().astype(np.float64)
    if normalize:
        h = (h - h.mean(-1, keepdims=True)) / np.sqrt(h.var(-1, keepdims=True) + 1e-5)
    ref = np.tensordot(w.astype(np.float64), h, axes=1)
    assert O.rel_err(feat.cpu().numpy(), ref) < 1e-5
    assert enc.status() == 0


def test_feature_selection_is_refused():
    from s3prl_amd.synth import named_config, synth_wavs, synth_weights

    torch = _torch()
    cfg = named_config("tiny_conformer_rope")
    enc = _encoder(cfg, synth_weights(cfg, 0))
    wavs = [torch.from_numpy(w).cuda() for w in synth_wavs([3000], 1)]
    from s3prl_amd._lib import S3EncError

    with pytest.raises(S3EncError, match="feature_selection"):
        enc.forward(wavs, selection="fairseq_layers")
