"""modified CPC on the MI355X, every test through the C ABI: the reference's own outputs (tests/golden/make_golden_cpc.py), the
channel-norm and the recurrent kernels against float64, the recurrence's bit-exact invariances (batch position, causality,
repeatability, row gaps), the family against its own ops, featurize, workspace regrowth and the refusals."""

import ctypes as C
import itertools
import os

import numpy as np
import pytest

from oracle import encoder_oracle as O

import cpc_ref as R

pytestmark = pytest.mark.gpu

FP32_TOL = 1e-4  # the project's fixture bound (tests/test_wav2vec_gpu.py)
OP_TOL = 2e-5    # the project's op bound
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = ["cpc/" + n for n in ["cpc_tiny_pad", "cpc_tiny_eq", "cpc_tiny_t1", "cpc_tiny_gru_pad", "cpc_tiny_lstm1_pad",
                                 "cpc_base_pseudo", "cpc_base_10s"]]


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


@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_fp32(name, golden_loader):
    torch = _torch()
    meta, cfg, weights, wavs, hs, norms = golden_loader(name)
    enc = _encoder(cfg, weights)
    assert enc.num_states() == len(hs) == 2
    out = enc.forward([torch.from_numpy(w).cuda() for w in wavs])
    torch.cuda.synchronize()
    assert list(out.shape[1:]) == meta["shape"]
    ts, cs = meta["t_stride"], meta["c_stride"]
    errs = [O.rel_err(out[l].cpu().numpy()[:, ::ts, ::cs], hs[l]) for l in range(2)]
    print(f"{name}: per-state rel-err {['%.2e' % e for e in errs]}")
    assert max(errs) < FP32_TOL, f"{name}: per-state rel-err {['%.2e' % e for e in errs]}"
    for l in range(2):
        n = np.linalg.norm(out[l].cpu().numpy().astype(np.float64))
        assert abs(n - norms[l]) / norms[l] < FP32_TOL
    assert enc.status() == 0


def test_frame_arithmetic_of_the_library():
    from s3prl_amd.synth import named_config, synth_weights

    cfg = named_config("tiny_cpc")
    enc = _encoder(cfg, synth_weights(cfg, 0))
    assert [enc.num_frames(n) for n in (160000, 16000, 4000, 159, 158, 1)] == [1000, 100, 25, 1, 0, 0]
    assert [enc.num_output_frames(n) for n in (160000, 159, 158)] == [1000, 1, 0]
    assert [enc.valid_frames(n, 160000) for n in (160000, 16000, 4000, 159, 158)] == [1000, 100, 25, 1, 0]
    assert enc.valid_frames(2345, 4000) == cfg.valid_frames(2345, 4000) == 14
    assert enc.downsample_rate() == 160 and enc.num_states() == 2


# ---- s3enc_op_channelnorm_relu -------------------------------------------------------------------------------------------
GUARD = 3  # NaN rows in front of and behind every output buffer: nothing outside (pad + rows + pad) rows may be written


@pytest.mark.parametrize("rows", [1, 3, 17, 31])
@pytest.mark.parametrize("C_", [64, 128, 192, 256, 512])
def test_channelnorm_relu_op(C_, rows):
    """Per-frame channel norm (unbiased variance) + ReLU into the zero-bordered operand and the state slot, against float64: border
    rows 0 / 1 / 2, with and without affine, with and without the state output; a frame of equal channels (variance 0)."""
    from s3prl_amd import _lib

    torch = _torch()
    lib = _lib.load()
    B = 3
    rng = np.random.default_rng(1000 * C_ + rows)
    x = (rng.standard_normal((B, rows, C_)) * rng.uniform(0.5, 2.0, (B, rows, 1)) + rng.uniform(-1, 1, (B, rows, 1))).astype(np.float32)
    x[1, rows // 2, :] = 0.75  # all channels equal: variance 0, the output is relu(beta)
    gamma = (1 + 0.1 * rng.standard_normal(C_)).astype(np.float32)
    beta = (0.05 * rng.standard_normal(C_)).astype(np.float32)
    dx, dg, db = _dev(x), _dev(gamma), _dev(beta)
    refs = {a: R.channelnorm_relu(x.astype(np.float64), gamma.astype(np.float64) if a else None, beta.astype(np.float64) if a else None)
            for a in (False, True)}
    assert np.array_equal(refs[True][1, rows // 2], np.maximum(beta.astype(np.float64), 0.0))
    worst = 0.0
    for pad, affine, with_state, with_dst in itertools.product([0, 1, 2], [False, True], [False, True], [False, True]):
        if not with_state and not with_dst or (pad and not with_dst):
            continue
        y = refs[affine]
        Rr = pad + rows + pad
        dst = torch.full((GUARD + B * Rr + GUARD, C_), float("nan"), device="cuda") if with_dst else None
        state = torch.full((GUARD + B * rows + GUARD, C_), float("nan"), device="cuda") if with_state else None
        _lib.check(lib.s3enc_op_channelnorm_relu(_ptr(dx), _ptr(dg) if affine else None, _ptr(db) if affine else None, B, rows, C_, pad,
                                                 _ptr(dst, GUARD * C_), _ptr(state, GUARD * C_), None), "s3enc_op_channelnorm_relu")
        torch.cuda.synchronize()
        for buf, r, p in ((dst, Rr, pad), (state, rows, 0)):
            if buf is None:
                continue
            h = buf.cpu().numpy()
            assert np.isnan(h[:GUARD]).all() and np.isnan(h[-GUARD:]).all(), "a guard row was written"
            body = h[GUARD:-GUARD].reshape(B, r, C_)
            worst = max(worst, O.rel_err(body[:, p:p + rows], y))
            assert np.abs(body[1, p + rows // 2] - y[1, rows // 2]).max() <= OP_TOL  # the variance-0 frame
            if p:
                assert np.array_equal(body[:, :p], np.zeros((B, p, C_))) and np.array_equal(body[:, p + rows:], np.zeros((B, p, C_)))
    print(f"channelnorm_relu rows={rows} C={C_}: worst rel-err {worst:.2e}")
    assert worst < OP_TOL


# ---- s3enc_op_rnn --------------------------------------------------------------------------------------------------------
GATES = {0: 4, 1: 3}


def _rnn_inputs(cell, B, T, H, seed):
    """pre with a standard deviation of 2 (gates far outside their linear range), recurrent weights 1.5 / sqrt(H), b_hn 0.1."""
    rng = np.random.default_rng(seed)
    G = GATES[cell]
    pre = (2.0 * rng.standard_normal((B, T, G * H))).astype(np.float32)
    w_hh = (rng.standard_normal((G * H, H)) * (1.5 / np.sqrt(H))).astype(np.float32)
    b_hn = (0.1 * rng.standard_normal(H)).astype(np.float32) if cell == 1 else None
    return pre, w_hh, b_hn


def _rnn_op(cell, pre_dev, w_hh, b_hn_dev, B, T, H, ld_pre=None, out=None, ldo=None):
    from s3prl_amd import _lib

    torch = _torch()
    lib = _lib.load()
    G = GATES[cell]
    ld_pre, ldo = ld_pre or G * H, ldo or H
    if out is None:
        out = torch.full((B, T, ldo), float("nan"), device="cuda")
    w = np.ascontiguousarray(w_hh, dtype=np.float32)
    _lib.check(lib.s3enc_op_rnn(cell, _ptr(pre_dev), C.c_void_p(w.ctypes.data), _ptr(b_hn_dev), B, T, H, ld_pre, _ptr(out), ldo, None),
               "s3enc_op_rnn")
    torch.cuda.synchronize()
    return out


def _rnn_ref64(cell, pre, w_hh, b_hn):
    p, w = pre.astype(np.float64), w_hh.astype(np.float64)
    return R.lstm_from_pre(p, w) if cell == 0 else R.gru_from_pre(p, w, b_hn.astype(np.float64))


def _torch_cpu_fp32(cell, pre, w_hh, b_hn):
    """torch's own CPU fp32 nn.LSTM / nn.GRU on the same weights and inputs: the input projection is the identity (exact in fp32),
    so its arithmetic sees exactly `pre`, and b_hn sits where nn.GRU keeps it."""
    import torch

    B, T, GH = pre.shape
    H = w_hh.shape[1]
    net = (torch.nn.LSTM if cell == 0 else torch.nn.GRU)(GH, H, num_layers=1, batch_first=True)
    with torch.no_grad():
        net.weight_ih_l0.copy_(torch.eye(GH))
        net.weight_hh_l0.copy_(torch.from_numpy(w_hh))
        net.bias_ih_l0.zero_()
        net.bias_hh_l0.zero_()
        if cell == 1:
            net.bias_hh_l0[2 * H:].copy_(torch.from_numpy(b_hn))
        return net(torch.from_numpy(pre))[0].numpy()


def _check_rnn(cell, B, T, H, seed):
    pre, w_hh, b_hn = _rnn_inputs(cell, B, T, H, seed)
    got = _rnn_op(cell, _dev(pre), w_hh, _dev(b_hn) if cell else None, B, T, H).cpu().numpy()
    ref = _rnn_ref64(cell, pre, w_hh, b_hn)
    ours, theirs = O.rel_err(got, ref), O.rel_err(_torch_cpu_fp32(cell, pre, w_hh, b_hn), ref)
    print(f"rnn {'LSTM' if cell == 0 else 'GRU'} H={H} T={T} B={B}: ours {ours:.2e}, torch CPU fp32 {theirs:.2e} (against float64)")
    # OP_TOL is the target; an error that compounds over T steps in another summation order may differ from the reference's own
    # by a small factor, not by an order of magnitude
    assert ours < max(OP_TOL, 8 * theirs), (cell, B, T, H, ours, theirs)
    return ours, theirs


@pytest.mark.parametrize("H", [64, 128, 256, 320, 512])
@pytest.mark.parametrize("cell", [0, 1])
def test_rnn_op(cell, H):
    """Both cells at every width class (one row per thread up to 1024 gate rows; two rows per thread above: LSTM from H = 320, GRU
    at H = 512), T in 1, 2, 3, 17 and B in 1, 3, 5, against float64."""
    for T, B in itertools.product([1, 2, 3, 17], [1, 3, 5]):
        _check_rnn(cell, B, T, H, seed=((cell * 600 + H) * 20 + T) * 8 + B)


@pytest.mark.parametrize("cell", [0, 1])
def test_rnn_op_long_recurrence(cell):
    _check_rnn(cell, 2, 1000, 256, seed=77 + cell)


@pytest.mark.parametrize("cell", [0, 1])
def test_rnn_op_is_bit_exact_where_it_must_be(cell):
    torch = _torch()
    H, T, B = 128, 17, 5
    G = GATES[cell]
    pre, w_hh, b_hn = _rnn_inputs(cell, B, T, H, 31 + cell)
    dpre, dbh = _dev(pre), (_dev(b_hn) if cell else None)
    full = _rnn_op(cell, dpre, w_hh, dbh, B, T, H)
    assert torch.isfinite(full).all()
    # two runs of the same input
    assert torch.equal(_rnn_op(cell, dpre, w_hh, dbh, B, T, H), full)
    # row b of the batch equals the same utterance run alone
    for b in range(B):
        alone = _rnn_op(cell, dpre[b:b + 1].contiguous(), w_hh, dbh, 1, T, H)
        assert torch.equal(alone[0], full[b]), b
    # causality: replacing pre at frames >= t leaves the output at frames < t unchanged
    for t in (1, 9, 16):
        changed = dpre.clone()
        changed[:, t:] = torch.from_numpy(np.random.default_rng(t).standard_normal((B, T - t, G * H)).astype(np.float32)).cuda()
        out = _rnn_op(cell, changed, w_hh, dbh, B, T, H)
        assert torch.equal(out[:, :t], full[:, :t]) and not torch.equal(out[:, t:], full[:, t:]), t
    # row strides larger than the rows: the gap bytes stay untouched, the rows are the same bits
    ld_pre, ldo = G * H + 24, H + 8
    wide = torch.full((B, T, ld_pre), float("nan"), device="cuda")
    wide[:, :, :G * H] = dpre
    out = torch.full((B, T, ldo), -7.0, device="cuda")
    _rnn_op(cell, wide, w_hh, dbh, B, T, H, ld_pre=ld_pre, out=out, ldo=ldo)
    assert torch.equal(out[:, :, :H], full) and bool((out[:, :, H:] == -7.0).all())


# ---- the family ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg_name", ["tiny_cpc", "tiny_cpc_gru"])
def test_recurrent_state_is_the_ops_applied_to_state_zero(cfg_name):
    """State 1 of a handle equals, per recurrent layer, s3enc_op_gemm (the input projection with the folded biases) followed by
    s3enc_op_rnn, applied to the handle's own state 0 — BIT FOR BIT: the engine issues exactly these two kernels on operands of the
    same shapes and strides, and folds b_ih + b_hh with the same single fp32 addition on the host."""
    from s3prl_amd import _lib
    from s3prl_amd.synth import named_config, synth_wavs, synth_weights

    torch = _torch()
    lib = _lib.load()
    cfg = named_config(cfg_name)
    weights = synth_weights(cfg, 8)
    enc = _encoder(cfg, weights)
    hs = enc.forward([torch.from_numpy(w).cuda() for w in synth_wavs([4000, 2345, 3111], 9)]).clone()
    torch.cuda.synchronize()
    _, B, T, H = hs.shape
    cell = 0 if cfg.ar_mode == "LSTM" else 1
    G = GATES[cell]
    x = hs[0].reshape(B * T, H).contiguous()
    for l in range(cfg.ar_layers):
        g = lambda n: weights[f"gAR.baseNet.{n}_l{l}"]  # noqa: E731
        bias = g("bias_ih").copy()
        fold = G * H if cell == 0 else 2 * H
        bias[:fold] = bias[:fold] + g("bias_hh")[:fold]
        dw, dbias = _dev(g("weight_ih")), _dev(bias)
        pre = torch.empty((B * T, G * H), device="cuda")
        _lib.check(lib.s3enc_op_gemm(_lib.F32, _ptr(x), H, 0, _ptr(dw), _ptr(dbias), B * T, G * H, H, 1, 0, None, None, _ptr(pre), None,
                                     G * H, 0, None), "s3enc_op_gemm")
        dbh = _dev(g("bias_hh")[2 * H:]) if cell else None
        x = _rnn_op(cell, pre, g("weight_hh"), dbh, B, T, H).reshape(B * T, H)
    assert torch.equal(x.reshape(B, T, H), hs[1])
    assert enc.status() == 0


@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("cfg_name", ["tiny_cpc", "tiny_cpc_gru"])
def test_featurize_is_the_weighted_sum_of_the_states(cfg_name, normalize):
    from s3prl_amd import _lib
    from s3prl_amd.synth import named_config, synth_wavs, synth_weights

    torch = _torch()
    lib = _lib.load()
    cfg = named_config(cfg_name)
    enc = _encoder(cfg, synth_weights(cfg, 4))
    wavs = [torch.from_numpy(w).cuda() for w in synth_wavs([4000, 2345, 3111], 6)]
    hs = enc.forward(wavs).clone()
    _, B, T, D = hs.shape
    for w in ([0.3, 0.7], [0.0, 1.0], [1.0, 0.0]):
        feat = enc.forward_featurized(wavs, w, normalize=normalize)
        want = torch.empty((B, T, D), device="cuda")
        wp = (C.c_float * 2)(*w)
        _lib.check(lib.s3enc_weighted_sum(_ptr(hs), B * T * D, 2, wp, int(normalize), B * T, D, _ptr(want), None), "s3enc_weighted_sum")
        torch.cuda.synchronize()
        assert O.rel_err(feat.cpu().numpy(), want.cpu().numpy()) < OP_TOL, w
    assert enc.status() == 0


def test_workspace_regrowth_keeps_the_bits():
    """One handle forwarded at 4000, 159 and 16000 samples in turn (the workspace grows, is reused smaller, grows again) equals
    fresh handles bit for bit."""
    from s3prl_amd.synth import named_config, synth_wavs, synth_weights

    torch = _torch()
    cfg = named_config("tiny_cpc")
    weights = synth_weights(cfg, 2)
    enc = _encoder(cfg, weights)
    for n in (4000, 159, 16000):
        wavs = [torch.from_numpy(w).cuda() for w in synth_wavs([n, max(159, n // 2)], n)]
        got = enc.forward(wavs).clone()
        fresh = _encoder(cfg, weights)
        want = fresh.forward(wavs).clone()
        torch.cuda.synchronize()
        assert got.shape[2] == cfg.num_frames(n) and torch.isfinite(got).all()
        assert torch.equal(got, want), n
        fresh.close()
    assert enc.status() == 0


def test_permutation_and_shard_are_bit_exact():
    from s3prl_amd.synth import named_config, synth_wavs, synth_weights

    torch = _torch()
    cfg = named_config("tiny_cpc")
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


REFUSALS = [("norm_mode", 3, 'normMode="batchNorm"'), ("ar_mode", 2, 'arMode="RNN"'), ("ar_mode", 3, 'arMode="transformer"'),
            ("ar_mode", 4, 'arMode="no_ar"'), ("reverse", 1, 'cpc_mode="reverse"'), ("keep_hidden", 1, 'samplingType="sequential"'),
            ("ar_hidden", 128, "hiddenGar != hiddenEncoder"), ("ar_layers", 5, "nLevelsGRU"), ("width", 96, "multiple of 64"),
            ("width", 576, "at most 512"), ("dtype", "bf16", "fp32 only")]


@pytest.mark.parametrize("field, value, match", REFUSALS)
def test_create_refusals_are_error_codes_with_a_message(field, value, match):
    from s3prl_amd import _lib
    from s3prl_amd.synth import named_config, synth_weights

    _torch()
    lib = _lib.load()
    cfg = named_config("tiny_cpc")
    ccfg, cpc = _lib.make_config(cfg, value if field == "dtype" else "fp32"), _lib.make_cpc_config(cfg)
    if field == "width":
        ccfg.conv_dim = ccfg.embed_dim = cpc.ar_hidden = value
    elif field != "dtype":
        setattr(cpc, field, value)
    h = C.c_void_p()
    tensors = (_lib.S3Tensor * 1)()
    assert lib.s3enc_create_cpc(C.byref(ccfg), C.byref(cpc), tensors, 0, 0, C.byref(h)) != 0 and not h.value
    assert match in lib.s3enc_last_error().decode()
    # with a valid configuration a missing hot-path tensor is named
    weights = synth_weights(cfg, 0)
    del weights["gAR.baseNet.weight_hh_l1"]
    with pytest.raises(_lib.S3EncError, match="gAR.baseNet.weight_hh_l1"):
        _encoder(cfg, weights)


def test_forward_refusals():
    from s3prl_amd import _lib
    from s3prl_amd._lib import S3EncError
    from s3prl_amd.synth import named_config, synth_wavs, synth_weights

    torch = _torch()
    cfg = named_config("tiny_cpc")
    enc = _encoder(cfg, synth_weights(cfg, 0))
    wavs = [torch.from_numpy(w).cuda() for w in synth_wavs([3000], 1)]
    with pytest.raises(S3EncError, match="feature_selection"):
        enc.forward(wavs, selection="fairseq_layers")
    with pytest.raises(S3EncError, match="feature_selection"):
        enc.num_states("fairseq_layers_before_residual")
    with pytest.raises(ValueError, match="receptive field"):
        enc.forward([wavs[0][:158]])
    with pytest.raises(ValueError, match="vq-wav2vec"):
        enc.forward(wavs, aux={})
    # the C entry itself: 158 samples are refused with a message, nothing is launched
    lib = _lib.load()
    out = torch.full((2, 1, 1, 64), float("nan"), device="cuda")
    ptrs = (C.c_void_p * 1)(wavs[0].data_ptr())
    lens = (C.c_int64 * 1)(158)
    assert lib.s3enc_forward(enc._h, ptrs, lens, 1, 0, _ptr(out), 64, None) != 0
    assert b"receptive field" in lib.s3enc_last_error()
    opts = _lib.S3ForwardOpts(_lib.SEL_HIDDEN, _lib.F16, 0, 0, None)
    lens = (C.c_int64 * 1)(3000)
    assert lib.s3enc_forward_ex(enc._h, ptrs, lens, 1, 0, C.byref(opts), _ptr(out), 64, None) != 0
    assert b"S3ENC_F32" in lib.s3enc_last_error()
    torch.cuda.synchronize()
    assert torch.isnan(out).all()


def test_expert_returns_the_fixture_states(tmp_path, golden_loader):
    """hub entry -> checkpoint written from synth_weights -> expert forward, CPU waveforms in, CPU states out."""
    torch = _torch()
    import s3prl_amd.hub as amd
    from s3prl_amd.ckpt import save_checkpoint

    meta, cfg, weights, wavs, hs, norms = golden_loader("cpc/cpc_tiny_pad")
    path = str(tmp_path / "c.pt")
    save_checkpoint(path, cfg, weights)
    expert = amd.cpc_local(path)
    with torch.no_grad():
        out = expert([torch.from_numpy(w) for w in wavs])
    assert set(out) == {"hidden_states", "last_hidden_state", "hidden_state_0", "hidden_state_1", "_hidden_states_info"}
    assert out["_hidden_states_info"] == ("self.model.gEncoder", "self.model.gAR")
    assert len(out["hidden_states"]) == 2 and out["last_hidden_state"] is out["hidden_states"][1]
    for l in range(2):
        assert out["hidden_states"][l].device.type == "cpu" and list(out["hidden_states"][l].shape) == meta["shape"]
        assert O.rel_err(out["hidden_states"][l].numpy(), hs[l]) < FP32_TOL
    assert expert.get_downsample_rates("hidden_states") == 160
