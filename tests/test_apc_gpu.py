"""APC / VQ-APC on the MI355X, every test through the C ABI: the front end with both windows against float64, the length-aware
recurrence against float64 (live rows, zero tails, guard bytes) and bit for bit where it must be, the model pinned to the
reference's own outputs (tests/golden/make_golden_apc.py), the family against its own ops, featurize, shards, handle reuse and
the refusals."""

import ctypes as C

import numpy as np
import pytest

from oracle import encoder_oracle as O

import apc_ref as R
import cpc_ref

pytestmark = pytest.mark.gpu

FP32_TOL = 1e-4  # the project's fixture bound
OP_TOL = 2e-5    # the project's op bound
FBANK_TOL_CMVN, FBANK_TOL_RAW = 5e-4, 2e-4  # tests/test_fbank_gpu.py: the 80 log-mel bins behind / without CMVN, absolute
FIXTURES = ["apc/" + n for n in ["apc_tiny_pad", "apc_tiny_eq", "apc_tiny_nores", "apc_tiny_t1", "apc_tiny_l4", "vq_apc_tiny_pad",
                                 "apc_360hr_pseudo"]]
GATES = {0: 4, 1: 3}
GUARD = 3  # NaN rows in front of and behind an output buffer: nothing outside the B * T rows may be written


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


# ---- the front end: s3enc_fbank_forward_ex ---------------------------------------------------------------------------------
def _fbank_config(cmvn=True, nmel=80):
    from s3prl_amd import _lib

    c = _lib.S3FbankConfig()
    c.sample_rate, c.num_mel_bins, c.frame_length_ms, c.frame_shift_ms, c.preemphasis = 16000, nmel, 25.0, 10.0, 0.97
    c.delta_order, c.delta_win_length, c.use_cmvn, c.cmvn_eps = 0, 5, int(cmvn), 1e-10
    return c


def _fbank(wavs_dev, window, cmvn=True, ex=True):
    from s3prl_amd import _lib

    torch = _torch()
    lib = _lib.load()
    c = _fbank_config(cmvn)
    lengths = [int(w.numel()) for w in wavs_dev]
    B, T = len(wavs_dev), max((n - 400) // 160 + 1 for n in lengths)
    out = torch.full((B, T, 80), float("nan"), device="cuda")
    ptrs = (C.c_void_p * B)(*[w.data_ptr() for w in wavs_dev])
    lens = (C.c_int64 * B)(*lengths)
    if ex:
        rc = lib.s3enc_fbank_forward_ex(C.byref(c), window, ptrs, lens, B, _ptr(out), T, 0, None)
    else:
        rc = lib.s3enc_fbank_forward(C.byref(c), ptrs, lens, B, _ptr(out), T, 0, None)
    _lib.check(rc, "s3enc_fbank_forward")
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("cmvn", [True, False])
@pytest.mark.parametrize("window", ["hamming", "povey"])
def test_front_end_against_float64(window, cmvn):
    from s3prl_amd.synth import synth_wavs

    lengths = [4000, 2345, 16000, 560]
    wavs = synth_wavs(lengths, 77)
    got = _fbank([_dev(w) for w in wavs], {"povey": 0, "hamming": 1}[window], cmvn).cpu().numpy()
    tol = FBANK_TOL_CMVN if cmvn else FBANK_TOL_RAW
    for b, w in enumerate(wavs):
        ref = R.kaldi_fbank(w.astype(np.float64), window_type=window)
        ref = R.cmvn(ref) if cmvn else ref
        n = ref.shape[0]
        err = np.abs(got[b, :n] - ref).max()
        print(f"fbank {window} cmvn={cmvn} utt {b} ({n} frames): max abs err {err:.2e}")
        assert err < tol, (window, cmvn, b, err)
        assert not got[b, n:].any()  # pad_sequence


def test_povey_through_ex_keeps_its_bits():
    from s3prl_amd.synth import synth_wavs

    torch = _torch()
    wavs = [_dev(w) for w in synth_wavs([4000, 2345, 16000], 78)]
    for cmvn in (True, False):
        assert torch.equal(_fbank(wavs, 0, cmvn, ex=True), _fbank(wavs, 0, cmvn, ex=False))
    assert not torch.equal(_fbank(wavs, 1), _fbank(wavs, 0))


# ---- s3enc_op_rnn_len ------------------------------------------------------------------------------------------------------
def _rnn_inputs(cell, B, T, H, seed):
    """pre with a standard deviation of 2 (gates far outside their linear range), recurrent weights 1.5 / sqrt(H), b_hn 0.1."""
    rng = np.random.default_rng(seed)
    G = GATES[cell]
    pre = (2.0 * rng.standard_normal((B, T, G * H))).astype(np.float32)
    w_hh = (rng.standard_normal((G * H, H)) * (1.5 / np.sqrt(H))).astype(np.float32)
    b_hn = (0.1 * rng.standard_normal(H)).astype(np.float32) if cell == 1 else None
    res = rng.standard_normal((B, T, H)).astype(np.float32)
    return pre, w_hh, b_hn, res


def _rnn_len_op(cell, pre_dev, w_hh, b_hn_dev, lens, B, T, H, res_dev=None, ld_res=None, ld_pre=None, out=None, ldo=None):
    from s3prl_amd import _lib

    torch = _torch()
    lib = _lib.load()
    G = GATES[cell]
    ld_pre, ldo = ld_pre or G * H, ldo or H
    if out is None:
        out = torch.full((B, T, ldo), float("nan"), device="cuda")
    w = np.ascontiguousarray(w_hh, dtype=np.float32)
    ln = (C.c_int32 * B)(*lens)
    _lib.check(lib.s3enc_op_rnn_len(cell, _ptr(pre_dev), C.c_void_p(w.ctypes.data), _ptr(b_hn_dev), C.cast(ln, C.c_void_p),
                                    _ptr(res_dev), (ld_res or H) if res_dev is not None else 0, B, T, H, ld_pre, _ptr(out), ldo, None),
               "s3enc_op_rnn_len")
    torch.cuda.synchronize()
    return out


def _rnn_op(cell, pre_dev, w_hh, b_hn_dev, B, T, H):
    from s3prl_amd import _lib

    torch = _torch()
    lib = _lib.load()
    out = torch.full((B, T, H), float("nan"), device="cuda")
    w = np.ascontiguousarray(w_hh, dtype=np.float32)
    _lib.check(lib.s3enc_op_rnn(cell, _ptr(pre_dev), C.c_void_p(w.ctypes.data), _ptr(b_hn_dev), B, T, H, GATES[cell] * H, _ptr(out), H,
                                None), "s3enc_op_rnn")
    torch.cuda.synchronize()
    return out


def _ref64(cell, pre, w_hh, b_hn, lens, res=None):
    """float64, per utterance over its own length; the rows behind it are zeros; res added to the row, not to the carried state"""
    B, T, _ = pre.shape
    H = w_hh.shape[1]
    out = np.zeros((B, T, H))
    for b, n in enumerate(lens):
        p, w = pre[b:b + 1, :n].astype(np.float64), w_hh.astype(np.float64)
        out[b, :n] = (cpc_ref.lstm_from_pre(p, w) if cell == 0 else cpc_ref.gru_from_pre(p, w, b_hn.astype(np.float64)))[0]
        if res is not None:
            out[b, :n] += res[b, :n].astype(np.float64)
    return out


def _torch_cpu_fp32(cell, pre, w_hh, b_hn, lens, res=None):
    """torch's own CPU fp32 nn.LSTM / nn.GRU on packed sequences of the same inputs (the input projection is the identity)"""
    import torch
    from torch.nn.utils.rnn import pack_padded_sequence, pad_packed_sequence

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
        packed = pack_padded_sequence(torch.from_numpy(pre), torch.LongTensor(lens), batch_first=True, enforce_sorted=False)
        out = pad_packed_sequence(net(packed)[0], batch_first=True, total_length=T)[0]
        if res is not None:
            for b, n in enumerate(lens):
                out[b, :n] += torch.from_numpy(res[b, :n])
        return out.numpy()


@pytest.mark.parametrize("with_res", [False, True])
@pytest.mark.parametrize("H", [64, 384, 512])  # 384: the smallest width with two gate rows per thread (GRU: 1152 rows)
@pytest.mark.parametrize("cell", [0, 1])
def test_rnn_len_op(cell, H, with_res):
    """T = 7, B = 3, lengths (7, 3, 1), row strides larger than the rows: live rows against float64 per utterance, tail rows exactly
    0, the gap and guard bytes untouched."""
    torch = _torch()
    B, T, lens = 3, 7, (7, 3, 1)
    pre, w_hh, b_hn, res = _rnn_inputs(cell, B, T, H, 4000 + 10 * H + cell)
    if not with_res:
        res = None
    ldo, ld_res = H + 8, H + 4
    out = torch.full((GUARD + B * T + GUARD, ldo), float("nan"), device="cuda")
    body = out[GUARD:GUARD + B * T].view(B, T, ldo)
    body[:, :, H:] = -7.0
    dres = None
    if with_res:
        dres = torch.full((B, T, ld_res), float("nan"), device="cuda")
        dres[:, :, :H] = _dev(res)
    _rnn_len_op(cell, _dev(pre), w_hh, _dev(b_hn) if cell else None, lens, B, T, H, res_dev=dres, ld_res=ld_res, out=body, ldo=ldo)
    h = out.cpu().numpy()
    assert np.isnan(h[:GUARD]).all() and np.isnan(h[-GUARD:]).all(), "a guard row was written"
    got = h[GUARD:-GUARD].reshape(B, T, ldo)
    assert (got[:, :, H:] == -7.0).all(), "the gap behind a row was written"
    got = got[:, :, :H]
    ref = _ref64(cell, pre, w_hh, b_hn, lens, res)
    theirs_all = _torch_cpu_fp32(cell, pre, w_hh, b_hn, lens, res)
    for b, n in enumerate(lens):
        assert np.array_equal(got[b, n:], np.zeros((T - n, H), dtype=np.float32)), (b, "tail rows must be exactly 0")
        ours, theirs = O.rel_err(got[b, :n], ref[b, :n]), O.rel_err(theirs_all[b, :n], ref[b, :n])
        print(f"rnn_len {'LSTM' if cell == 0 else 'GRU'} H={H} res={with_res} utt {b} ({n} steps): ours {ours:.2e}, torch CPU fp32 {theirs:.2e}")
        assert ours < max(OP_TOL, 8 * theirs), (cell, H, with_res, b, ours, theirs)


@pytest.mark.parametrize("H", [64, 384, 512])
@pytest.mark.parametrize("cell", [0, 1])
def test_full_lengths_without_res_are_the_plain_recurrence_bit_for_bit(cell, H):
    torch = _torch()
    B, T = 3, 7
    pre, w_hh, b_hn, _ = _rnn_inputs(cell, B, T, H, 5000 + 10 * H + cell)
    dpre, dbh = _dev(pre), (_dev(b_hn) if cell else None)
    plain = _rnn_op(cell, dpre, w_hh, dbh, B, T, H)
    assert torch.isfinite(plain).all()
    assert torch.equal(_rnn_len_op(cell, dpre, w_hh, dbh, (T,) * B, B, T, H), plain)


@pytest.mark.parametrize("H", [128, 512])
def test_an_utterances_rows_depend_on_nothing_but_the_utterance(H):
    """Bit for bit: the batch size, the place in the batch, the other lengths and T do not reach an utterance's rows; two runs agree."""
    torch = _torch()
    cell, B, T = 1, 4, 9
    lens = (9, 4, 1, 6)
    pre, w_hh, b_hn, res = _rnn_inputs(cell, B, T, H, 6000 + H)
    dpre, dbh, dres = _dev(pre), _dev(b_hn), _dev(res)
    full = _rnn_len_op(cell, dpre, w_hh, dbh, lens, B, T, H, res_dev=dres)
    assert torch.isfinite(full).all()
    assert torch.equal(_rnn_len_op(cell, dpre, w_hh, dbh, lens, B, T, H, res_dev=dres), full)  # run twice
    for b, n in enumerate(lens):
        alone = _rnn_len_op(cell, dpre[b:b + 1].contiguous(), w_hh, dbh, (n,), 1, T, H, res_dev=dres[b:b + 1].contiguous())
        assert torch.equal(alone[0], full[b]), ("alone", b)
        short = _rnn_len_op(cell, dpre[b:b + 1, :n].contiguous(), w_hh, dbh, (n,), 1, n, H, res_dev=dres[b:b + 1, :n].contiguous())
        assert torch.equal(short[0], full[b, :n]), ("T = its own length", b)
    perm = [2, 0, 3, 1]
    idx = torch.tensor(perm, device="cuda")
    permuted = _rnn_len_op(cell, dpre[idx].contiguous(), w_hh, dbh, [lens[i] for i in perm], B, T, H, res_dev=dres[idx].contiguous())
    for j, i in enumerate(perm):
        assert torch.equal(permuted[j], full[i]), ("permuted", j, i)
    other = _rnn_len_op(cell, dpre, w_hh, dbh, (4, 4, 9, 6), B, T, H, res_dev=dres)  # the other lengths change
    assert torch.equal(other[1], full[1]) and torch.equal(other[3], full[3])
    assert torch.equal(other[0, :4], full[0, :4]) and torch.equal(other[2, :1], full[2, :1])


class _split:
    """the tuning key rnn_split for the calling thread's op entries, restored on exit"""

    def __init__(self, S):
        self.S = S

    def __enter__(self):
        from s3prl_amd import _lib

        _lib.check(_lib.load().s3enc_set_tuning(b"rnn_split", self.S), "s3enc_set_tuning")

    def __exit__(self, *exc):
        from s3prl_amd import _lib

        _lib.check(_lib.load().s3enc_set_tuning(b"rnn_split", -1), "s3enc_set_tuning")  # the default rule


@pytest.mark.parametrize("H, splits", [(128, (1, 2)), (512, (1, 2, 4, 8))])
@pytest.mark.parametrize("cell", [0, 1])
def test_step_form_is_the_one_launch_form_bit_for_bit(cell, H, splits):
    """T = 5, B = 2, lengths (5, 2), with and without res: every S gives the one-launch form's bits, zero tail included (the
    output buffers start as NaN)."""
    torch = _torch()
    B, T, lens = 2, 5, (5, 2)
    pre, w_hh, b_hn, res = _rnn_inputs(cell, B, T, H, 7000 + 10 * H + cell)
    dpre, dbh = _dev(pre), (_dev(b_hn) if cell else None)
    for dres in (None, _dev(res)):
        with _split(0):
            one = _rnn_len_op(cell, dpre, w_hh, dbh, lens, B, T, H, res_dev=dres)
        assert torch.isfinite(one).all() and not one[1, 2:].any()
        assert torch.equal(_rnn_len_op(cell, dpre, w_hh, dbh, lens, B, T, H, res_dev=dres), one)  # whatever the default picks
        for S in splits:
            with _split(S):
                got = _rnn_len_op(cell, dpre, w_hh, dbh, lens, B, T, H, res_dev=dres)
            assert torch.equal(got, one), (cell, H, S, dres is not None)


def test_step_form_refuses_what_it_cannot_split():
    from s3prl_amd import _lib

    _torch()
    lib = _lib.load()
    pre, w_hh, b_hn, _ = _rnn_inputs(1, 1, 2, 64, 1)
    with _split(2):  # H / S = 32 is no multiple of 64
        with pytest.raises(_lib.S3EncError, match="rnn_split"):
            _rnn_len_op(1, _dev(pre), w_hh, _dev(b_hn), (2,), 1, 2, 64)
    assert lib.s3enc_set_tuning(b"rnn_split", 9) != 0 and lib.s3enc_set_tuning(b"rnn_split", -2) != 0


def test_family_in_the_step_form_keeps_its_bits(golden_loader):
    """apc_360hr_pseudo (H = 512, ragged): the handle's rnn_split = 8 / 4 / -1 (the default rule: the step form with S = 8 at this width)
    against the one-launch form (0), bit for bit."""
    from s3prl_amd import _lib

    torch = _torch()
    meta, cfg, weights, wavs, hs, norms = golden_loader("apc/apc_360hr_pseudo")
    dev = [torch.from_numpy(w).cuda() for w in wavs]
    one = _encoder(cfg, weights)
    _lib.check(_lib.load().s3enc_set_handle_tuning(one._h, b"rnn_split", 0), "s3enc_set_handle_tuning")
    want = one.forward(dev).clone()
    for S in (8, 4, -1):
        enc = _encoder(cfg, weights)
        _lib.check(_lib.load().s3enc_set_handle_tuning(enc._h, b"rnn_split", S), "s3enc_set_handle_tuning")
        got = enc.forward(dev).clone()
        torch.cuda.synchronize()
        assert torch.equal(got, want), S
        assert enc.status() == 0


# ---- the model, pinned to the reference ------------------------------------------------------------------------------------
def _op_chain(cfg, weights, feats_dev, lens):
    """The three states from (B, T, F) features through s3enc_op_gemm + s3enc_op_rnn_len, as the engine issues them."""
    from s3prl_amd import _lib

    torch = _torch()
    lib = _lib.load()
    B, T, F = feats_dev.shape
    H = cfg.conv_dim
    x, I, outs = feats_dev.reshape(B * T, F).contiguous(), F, []
    for l in range(cfg.apc_layers):
        g = lambda n: weights[f"rnn_layers.{l}.{n}_l0"]  # noqa: E731
        bias = g("bias_ih").copy()
        bias[:2 * H] = bias[:2 * H] + g("bias_hh")[:2 * H]
        dw, dbias = _dev(g("weight_ih")), _dev(bias)
        pre = torch.empty((B * T, 3 * H), device="cuda")
        _lib.check(lib.s3enc_op_gemm(_lib.F32, _ptr(x), I, 0, _ptr(dw), _ptr(dbias), B * T, 3 * H, I, 1, 0, None, None, _ptr(pre), None,
                                     3 * H, 0, None), "s3enc_op_gemm")
        res = x if (cfg.apc_residual and l > 0) else None
        y = _rnn_len_op(1, pre, g("weight_hh"), _dev(g("bias_hh")[2 * H:]), lens, B, T, H, res_dev=res)
        outs.append(y)
        x, I = y.reshape(B * T, H), H
    return [outs[0], outs[1], outs[-1]]


def _score_per_utterance(got, hs, lens, meta, what):
    ts, cs = meta["t_stride"], meta["c_stride"]
    worst = 0.0
    for l in range(3):
        g = got[l].cpu().numpy()
        for b, n in enumerate(lens):
            assert not g[b, n:].any(), (what, l, b, "rows behind the length must be exactly 0")
            worst = max(worst, O.rel_err(g[b, :n:ts, ::cs], hs[l][b, :-(-n // ts)]))
    return worst


@pytest.mark.parametrize("name", FIXTURES)
def test_model_from_the_fixture_features(name, golden_loader):
    """The features the reference was fed (apc_ref's front end, rounded to fp32) through the op chain: every state per utterance."""
    meta, cfg, weights, wavs, hs, norms = golden_loader(name)
    feats, lens = R.features(cfg, wavs)
    got = _op_chain(cfg, weights, _dev(feats.astype(np.float32)), lens)
    err = _score_per_utterance(got, hs, lens, meta, name)
    print(f"{name}: model from the fixture's features, worst per-(state, utterance) rel-err {err:.2e}")
    assert err < FP32_TOL, (name, err)


# ---- the family ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_fp32_from_waveforms(name, golden_loader):
    torch = _torch()
    meta, cfg, weights, wavs, hs, norms = golden_loader(name)
    enc = _encoder(cfg, weights)
    assert enc.num_states() == len(hs) == 3
    out = enc.forward([torch.from_numpy(w).cuda() for w in wavs])
    torch.cuda.synchronize()
    assert list(out.shape[1:]) == meta["shape"]
    err = _score_per_utterance(out, hs, meta["frames"], meta, name)
    print(f"{name}: from waveforms, worst per-(state, utterance) rel-err {err:.2e}")
    assert err < FP32_TOL, (name, err)
    for l in range(3):
        n = np.linalg.norm(out[l].cpu().numpy().astype(np.float64))
        assert abs(n - norms[l]) / norms[l] < FP32_TOL
    assert enc.status() == 0


@pytest.mark.parametrize("cfg_name", ["tiny_apc", "tiny_apc_nores", "tiny_apc_nocmvn", "tiny_apc_l4", "tiny_vq_apc"])
def test_family_is_its_own_ops_bit_for_bit(cfg_name):
    """A handle's states equal s3enc_fbank_forward_ex -> (s3enc_op_gemm -> s3enc_op_rnn_len) per layer BIT FOR BIT."""
    from s3prl_amd.synth import named_config, synth_wavs, synth_weights

    torch = _torch()
    cfg = named_config(cfg_name)
    weights = synth_weights(cfg, 8)
    lengths = [4000, 2345, 3111, 400 if not cfg.apc_cmvn else 560]
    wavs = [torch.from_numpy(w).cuda() for w in synth_wavs(lengths, 9)]
    enc = _encoder(cfg, weights)
    hs = enc.forward(wavs).clone()
    torch.cuda.synchronize()
    feats = _fbank(wavs, 1, cfg.apc_cmvn)
    want = _op_chain(cfg, weights, feats, [cfg.num_frames(n) for n in lengths])
    for l in range(3):
        assert torch.equal(hs[l], want[l]), (cfg_name, l)
    assert enc.status() == 0


def test_frame_arithmetic_of_the_library():
    from s3prl_amd.synth import named_config, synth_weights

    cfg = named_config("tiny_apc")
    enc = _encoder(cfg, synth_weights(cfg, 0))
    assert [enc.num_frames(n) for n in (160000, 16000, 4000, 400, 399, 1)] == [998, 98, 23, 1, 0, 0]
    assert [enc.num_output_frames(n) for n in (160000, 400, 399)] == [998, 1, 0]
    assert [enc.valid_frames(n, 160000) for n in (160000, 16000, 4000, 400, 399)] == [998, 98, 23, 1, 0]
    assert enc.valid_frames(2345, 4000) == cfg.valid_frames(2345, 4000) == 13
    assert enc.downsample_rate() == 160 and enc.num_states() == 3


@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("cfg_name", ["tiny_apc", "tiny_apc_l4"])
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
    for w in ([0.2, 0.3, 0.5], [0.0, 0.0, 1.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]):
        feat = enc.forward_featurized(wavs, w, normalize=normalize)
        want = torch.empty((B, T, D), device="cuda")
        wp = (C.c_float * 3)(*w)
        _lib.check(lib.s3enc_weighted_sum(_ptr(hs), B * T * D, 3, wp, int(normalize), B * T, D, _ptr(want), None), "s3enc_weighted_sum")
        torch.cuda.synchronize()
        assert O.rel_err(feat.cpu().numpy(), want.cpu().numpy()) < OP_TOL, w
    assert enc.status() == 0


def test_permutation_and_shard_are_bit_exact():
    from s3prl_amd.synth import named_config, synth_wavs, synth_weights

    torch = _torch()
    cfg = named_config("tiny_apc")
    enc = _encoder(cfg, synth_weights(cfg, 3))
    lengths = [4000, 2345, 800, 3111, 1999]
    wavs = [torch.from_numpy(w).cuda() for w in synth_wavs(lengths, 5)]
    full = enc.forward(wavs).clone()
    perm = [3, 0, 4, 2, 1]
    permuted = enc.forward([wavs[i] for i in perm]).clone()
    shard = enc.forward(wavs[2:4], n_max=max(lengths)).clone()  # padded to the global length: the full batch's rows
    torch.cuda.synchronize()
    for j, i in enumerate(perm):
        assert torch.equal(permuted[:, j], full[:, i])
    assert torch.equal(shard, full[:, 2:4])


def test_one_handle_at_several_lengths_equals_fresh_handles():
    from s3prl_amd.synth import named_config, synth_wavs, synth_weights

    torch = _torch()
    cfg = named_config("tiny_apc")
    weights = synth_weights(cfg, 2)
    enc = _encoder(cfg, weights)
    for n in (4000, 560, 16000, 2345):
        wavs = [torch.from_numpy(w).cuda() for w in synth_wavs([n, max(560, n // 2)], n)]
        got = enc.forward(wavs).clone()
        fresh = _encoder(cfg, weights)
        want = fresh.forward(wavs).clone()
        torch.cuda.synchronize()
        assert got.shape[2] == cfg.num_frames(n) and torch.isfinite(got).all()
        assert torch.equal(got, want), n
        fresh.close()
    assert enc.status() == 0


REFUSALS = [("num_layers", 2, "at least 3"), ("num_layers", 5, "above 4"), ("width", 96, "multiple of 64"), ("width", 576, "at most 512"),
            ("frame_length_ms", 25.1, "multiple of 4 samples"), ("dtype", "bf16", "fp32 only")]


@pytest.mark.parametrize("field, value, match", REFUSALS)
def test_create_refusals_are_error_codes_with_a_message(field, value, match):
    from s3prl_amd import _lib
    from s3prl_amd.synth import named_config, synth_weights

    _torch()
    lib = _lib.load()
    cfg = named_config("tiny_apc")
    ccfg, apc = _lib.make_config(cfg, value if field == "dtype" else "fp32"), _lib.make_apc_config(cfg)
    if field == "width":
        ccfg.conv_dim = ccfg.embed_dim = apc.hidden = value
    elif field != "dtype":
        setattr(apc, field, value)
    h = C.c_void_p()
    tensors = (_lib.S3Tensor * 1)()
    assert lib.s3enc_create_apc(C.byref(ccfg), C.byref(apc), tensors, 0, 0, C.byref(h)) != 0 and not h.value
    assert match in lib.s3enc_last_error().decode()
    # with a valid configuration a missing GRU tensor is named
    weights = synth_weights(cfg, 0)
    del weights["rnn_layers.1.weight_hh_l0"]
    with pytest.raises(_lib.S3EncError, match="rnn_layers.1.weight_hh_l0"):
        _encoder(cfg, weights)


def test_forward_refusals():
    from s3prl_amd import _lib
    from s3prl_amd._lib import S3EncError
    from s3prl_amd.synth import named_config, synth_wavs, synth_weights

    torch = _torch()
    cfg = named_config("tiny_apc")
    enc = _encoder(cfg, synth_weights(cfg, 0))
    wavs = [torch.from_numpy(w).cuda() for w in synth_wavs([3000, 399], 1)]
    with pytest.raises(S3EncError, match="feature_selection"):
        enc.forward(wavs[:1], selection="fairseq_layers")
    with pytest.raises(S3EncError, match="feature_selection"):
        enc.num_states("fairseq_layers_before_residual")
    with pytest.raises(ValueError, match="shorter than one analysis window"):
        enc.forward(wavs)  # the SHORT one of the batch, not only the longest, must hold a window
    with pytest.raises(ValueError, match="vq-wav2vec"):
        enc.forward(wavs[:1], aux={})
    # the C entry itself: 399 samples beside a longer utterance are refused with a message, nothing is launched
    lib = _lib.load()
    T = cfg.num_frames(3000)
    out = torch.full((3, 2, T, 64), float("nan"), device="cuda")
    ptrs = (C.c_void_p * 2)(wavs[0].data_ptr(), wavs[1].data_ptr())
    lens = (C.c_int64 * 2)(3000, 399)
    assert lib.s3enc_forward(enc._h, ptrs, lens, 2, 0, _ptr(out), 2 * T * 64, None) != 0
    assert b"shorter than one analysis window" in lib.s3enc_last_error()
    opts = _lib.S3ForwardOpts(_lib.SEL_HIDDEN, _lib.F16, 0, 0, None)
    assert lib.s3enc_forward_ex(enc._h, ptrs, lens, 1, 0, C.byref(opts), _ptr(out), 2 * T * 64, None) != 0
    assert b"S3ENC_F32" in lib.s3enc_last_error()
    torch.cuda.synchronize()
    assert torch.isnan(out).all()


def test_expert_returns_the_fixture_states(tmp_path, golden_loader):
    """hub entry -> checkpoint written from synth_weights -> expert forward, CPU waveforms in, CPU states out."""
    torch = _torch()
    import s3prl_amd.hub as amd
    from s3prl_amd.ckpt import save_checkpoint

    for name, entry in (("apc/apc_tiny_pad", amd.apc_local), ("apc/vq_apc_tiny_pad", amd.apc_local)):
        meta, cfg, weights, wavs, hs, norms = golden_loader(name)
        path = str(tmp_path / "c.pt")
        save_checkpoint(path, cfg, weights)
        expert = entry(path)
        with torch.no_grad():
            out = expert([torch.from_numpy(w) for w in wavs])
        assert set(out) == {"hidden_states", "last_hidden_state", "hidden_state_0", "hidden_state_1", "hidden_state_2",
                            "_hidden_states_info"}
        assert out["_hidden_states_info"] == ("self.model.rnn_layers[1]", "self.model.rnn_layers[2]", "self.model")
        assert len(out["hidden_states"]) == 3 and out["last_hidden_state"] is out["hidden_states"][2]
        for l in range(3):
            assert out["hidden_states"][l].device.type == "cpu" and list(out["hidden_states"][l].shape) == meta["shape"]
            assert O.rel_err(out["hidden_states"][l].numpy(), hs[l]) < FP32_TOL
        assert expert.get_downsample_rates("hidden_states") == 160
