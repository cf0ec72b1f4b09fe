"""NPC on the MI355X, every test through the C ABI: the model pinned to the reference's own outputs on ALL rows
(tests/golden/make_golden_npc.py), every frame against float64 on the GPU front end's own features, the family against its own
ops bit for bit, the two-run form against the dense form, an utterance alone against its rows in the batch, shards, handle reuse,
featurize, the status word and the refusals."""

import ctypes as C

import numpy as np
import pytest

from oracle import encoder_oracle as O

import npc_ref as R
import posconv_ref as PR

pytestmark = pytest.mark.gpu

FP32_TOL = 1e-4  # the project's fixture bound
OP_TOL = 2e-5    # the project's op bound
FIXTURES = ["npc/" + n for n in ["npc_tiny_pad", "npc_tiny_eq", "npc_tiny_plain", "npc_tiny_t1", "npc_tiny_last", "npc_tiny_k9",
                                 "npc_360hr_pseudo"]]
CONFIGS = ["tiny_npc", "tiny_npc_plain", "tiny_npc_nocmvn", "tiny_npc_last", "tiny_npc_k9", "tiny_npc_h192"]


def _torch():
    import torch

    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _dev(x, dtype=np.float32):
    return _torch().from_numpy(np.ascontiguousarray(x, dtype=dtype)).cuda()


def _encoder(cfg, weights, dtype="fp32"):
    from s3prl_amd.encoder import HipEncoder

    return HipEncoder(cfg, weights, dtype=dtype)


def _wavs(lengths, seed):
    from s3prl_amd.synth import synth_wavs

    torch = _torch()
    return [torch.from_numpy(w).cuda() for w in synth_wavs(lengths, seed)]


def _fbank(cfg, wavs_dev, n_max=None):
    """The front end's own output, (B, T, F) with zeros behind every utterance's frames: s3enc_fbank_forward_ex, hamming"""
    from s3prl_amd import _lib

    torch = _torch()
    lib = _lib.load()
    c = _lib.S3FbankConfig()
    c.sample_rate, c.num_mel_bins, c.frame_length_ms, c.frame_shift_ms, c.preemphasis = 16000, cfg.apc_feat_dim, 25.0, 10.0, 0.97
    c.delta_order, c.delta_win_length, c.use_cmvn, c.cmvn_eps = 0, 5, int(cfg.apc_cmvn), 1e-10
    lengths = [int(w.numel()) for w in wavs_dev]
    B, T = len(wavs_dev), cfg.num_frames(n_max or max(lengths))
    out = torch.full((B, T, cfg.apc_feat_dim), float("nan"), device="cuda")
    ptrs = (C.c_void_p * B)(*[w.data_ptr() for w in wavs_dev])
    lens = (C.c_int64 * B)(*lengths)
    _lib.check(lib.s3enc_fbank_forward_ex(C.byref(c), 1, ptrs, lens, B, _ptr(out), T, 0, None), "s3enc_fbank_forward_ex")
    torch.cuda.synchronize()
    return out


def _folded(cfg, weights, i):
    """block i's two convolutions with their BatchNorms folded in, as the library does it: float64, rounded to fp32 once"""
    p = f"blocks.{i}."
    out = []
    for conv, bn in (("conv", "bn1"), ("linear", "bn2")):
        w, b = weights[p + conv + ".weight"].astype(np.float64), weights[p + conv + ".bias"].astype(np.float64)
        if cfg.npc_batch_norm:
            g, beta, mean, var = (weights[p + bn + "." + n].astype(np.float64) for n in ("weight", "bias", "running_mean", "running_var"))
            s = g / np.sqrt(var + 1e-5)
            w, b = w * s[:, None, None], (b - mean) * s + beta
        out += [w.astype(np.float32), b.astype(np.float32)]
    return out


def _conv_taps(x, w, bias, T, k, mask=0, act=0, res=None, dst=None, dst_pad=0, state=None, sm=None, sum_init=1, dense=0):
    from s3prl_amd import _lib

    lib = _lib.load()
    N, Cin, _ = w.shape
    wh = np.ascontiguousarray(w, dtype=np.float32)
    _lib.check(lib.s3enc_op_conv_taps(_ptr(x), C.c_void_p(wh.ctypes.data), _ptr(bias), x.shape[0], T, Cin, N, k, mask, act, _ptr(res),
                                      N if res is not None else 0, _ptr(dst), dst_pad, N if dst is not None else 0, _ptr(state),
                                      _ptr(sm), sum_init, dense, None), "s3enc_op_conv_taps")


def _op_chain(cfg, weights, feats):
    """The states from (B, T, F) features through s3enc_op_conv_taps, three calls per block as the engine issues them"""
    torch = _torch()
    B, T, F = feats.shape
    H, k, P = cfg.conv_dim, cfg.npc_kernel_size, (cfg.npc_kernel_size - 1) // 2
    act = 1 if cfg.npc_activate == "relu" else 2
    x, states, total = feats, [], None
    for i in range(cfg.npc_blocks):
        w3, b3, w1, b1 = _folded(cfg, weights, i)
        x1 = torch.zeros((B, T + 2, x.shape[2]), device="cuda")
        x1[:, 1:T + 1] = x
        h = torch.empty((B, T, H), device="cuda")
        _conv_taps(x1, w3, _dev(b3), T, 3, act=act, dst=h)
        xb = torch.zeros((B, T + 2 * P, H), device="cuda")
        s = torch.empty((B, T, H), device="cuda")
        _conv_taps(h, w1, _dev(b1), T, 1, act=act, res=x if (cfg.npc_residual and i > 0) else None, dst=xb, dst_pad=P, state=s)
        states.append(s)
        x = s
        if not cfg.npc_has_mask(i):
            continue
        m = torch.empty((B, T, H), device="cuda")
        if total is None:
            total = torch.full((B, T, H), float("nan"), device="cuda")
            init = 1
        else:
            init = 0
        _conv_taps(xb, weights[f"masked_convs.{i}.conv.weight"], _dev(weights[f"masked_convs.{i}.conv.bias"]), T, k,
                   mask=cfg.npc_mask(i), act=2, state=m, sm=total, sum_init=init)
        states.append(m)
    torch.cuda.synchronize()
    return states + [total]


def _torch_fp32(cfg, weights, feats):
    """the same modules in torch CPU fp32 (conv1d, batch_norm in eval mode, the activations), on (B, T, F) features"""
    torch = _torch()
    F_ = torch.nn.functional
    g = lambda n: torch.from_numpy(np.ascontiguousarray(weights[n], dtype=np.float32))  # noqa: E731
    act = torch.relu if cfg.npc_activate == "relu" else torch.tanh
    x = feats.transpose(1, 2)
    hs, feat = [], None
    for i in range(cfg.npc_blocks):
        p = f"blocks.{i}."
        y = F_.conv1d(x, g(p + "conv.weight"), g(p + "conv.bias"), padding=1)
        if cfg.npc_batch_norm:
            y = F_.batch_norm(y, g(p + "bn1.running_mean"), g(p + "bn1.running_var"), g(p + "bn1.weight"), g(p + "bn1.bias"), False, 0.1, 1e-5)
        y = F_.conv1d(act(y), g(p + "linear.weight"), g(p + "linear.bias"))
        if cfg.npc_batch_norm:
            y = F_.batch_norm(y, g(p + "bn2.running_mean"), g(p + "bn2.running_var"), g(p + "bn2.weight"), g(p + "bn2.bias"), False, 0.1, 1e-5)
        if cfg.npc_residual and i > 0:
            y = y + x
        x = act(y)
        hs.append(x.transpose(1, 2))
        if not cfg.npc_has_mask(i):
            continue
        k, m = cfg.npc_kernel_size, cfg.npc_mask(i)
        w = g(f"masked_convs.{i}.conv.weight").clone()
        w[:, :, (k - m) // 2:(k - m) // 2 + m] = 0
        mk = torch.tanh(F_.conv1d(x, w, g(f"masked_convs.{i}.conv.bias"), padding=(k - 1) // 2)).transpose(1, 2)
        hs.append(mk)
        feat = mk if feat is None else feat + mk
    return hs + [feat]


# ---- pinned to the reference -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_fp32_from_waveforms(name, golden_loader):
    """every state within FP32_TOL of the reference's, whole, per utterance (padded rows included) and on the padded rows alone"""
    torch = _torch()
    meta, cfg, weights, wavs, hs, norms = golden_loader(name)
    enc = _encoder(cfg, weights)
    assert enc.num_states() == len(hs) == meta["n_states"]
    out = enc.forward([torch.from_numpy(w).cuda() for w in wavs])
    torch.cuda.synchronize()
    assert list(out.shape[1:]) == meta["shape"]
    ts, cs = meta["t_stride"], meta["c_stride"]
    worst = 0.0
    for l in range(len(hs)):
        g = out[l].cpu().numpy()
        errs = [O.rel_err(g[:, ::ts, ::cs], hs[l])] + [O.rel_err(g[b, ::ts, ::cs], hs[l][b]) for b in range(len(wavs))]
        errs += [O.rel_err(g[b, n::ts, ::cs], hs[l][b, -(-n // ts):]) for b, n in enumerate(meta["frames"]) if n < g.shape[1]]
        worst = max(worst, max(errs))
        assert max(errs) < FP32_TOL, (name, l, errs)
        n = np.linalg.norm(g.astype(np.float64))
        assert abs(n - norms[l]) / norms[l] < FP32_TOL
    print(f"{name}: from waveforms, worst per-(state, utterance | padded rows) rel-err {worst:.2e}")
    if cfg.npc_disable_cross_layer:
        assert torch.equal(out[-1], out[-2])
    assert enc.status() == 0


@pytest.mark.parametrize("cfg_name, lengths", [("tiny_npc", [4000, 2345, 3111, 560]), ("tiny_npc_plain", [4000, 2345, 3111]),
                                               ("tiny_npc_nocmvn", [400, 2000]), ("tiny_npc", [1200]), ("tiny_npc_last", [4000, 2345]),
                                               ("tiny_npc_k9", [4000, 2345, 3111]), ("tiny_npc_h192", [11000, 2345]),
                                               ("npc_360hr", [16000, 12345])])
def test_every_frame_against_float64_on_the_front_ends_own_features(cfg_name, lengths):
    """All T rows of every state, frame by frame, against npc_ref in float64 on the GPU front end's output; the op rule with
    `theirs` = the same modules in torch CPU fp32 on the same features.  [1200] is T = 6 < P: every masked window hangs over both
    ends."""
    from s3prl_amd.synth import named_config, synth_weights

    torch = _torch()
    cfg = named_config(cfg_name)
    weights = synth_weights(cfg, 21)
    wavs = _wavs(lengths, 22)
    enc = _encoder(cfg, weights)
    out = enc.forward(wavs).clone()
    torch.cuda.synchronize()
    feats = _fbank(cfg, wavs).cpu()
    ref = R.model(cfg, weights, feats.numpy().astype(np.float64))["hidden_states"]
    theirs = _torch_fp32(cfg, weights, feats)
    assert out.shape[0] == len(ref) == len(theirs) == cfg.num_hidden_states
    for l, r in enumerate(ref):
        r = torch.from_numpy(r)
        a = PR.frame_scores(out[l].cpu(), r, OP_TOL).numpy()
        b = PR.frame_scores(theirs[l], r, OP_TOL).numpy()
        print(f"{cfg_name} {lengths} state {l}: worst frame ours {a[1]:.2e} (frame {int(a[2])}) theirs {b[1]:.2e}, whole {a[0]:.2e}, "
              f"elements off {int(a[3])}")
        assert a[1] < max(OP_TOL, 8 * b[1]), (cfg_name, l, a, b)
        assert a[3] == 0, (cfg_name, l, a)
    assert enc.status() == 0


@pytest.mark.parametrize("cfg_name", CONFIGS)
def test_family_is_its_own_ops_bit_for_bit(cfg_name):
    """A handle's states equal s3enc_fbank_forward_ex -> three s3enc_op_conv_taps per block BIT FOR BIT"""
    from s3prl_amd.synth import named_config, synth_weights

    torch = _torch()
    cfg = named_config(cfg_name)
    weights = synth_weights(cfg, 8)
    wavs = _wavs([4000, 2345, 3111, 400 if not cfg.apc_cmvn else 560, 11000], 9)  # T = 67: two 64-row tiles
    enc = _encoder(cfg, weights)
    hs = enc.forward(wavs).clone()
    torch.cuda.synchronize()
    want = _op_chain(cfg, weights, _fbank(cfg, wavs))
    assert len(want) == hs.shape[0]
    for l in range(hs.shape[0]):
        assert torch.equal(hs[l], want[l]), (cfg_name, l)
    assert enc.status() == 0


@pytest.mark.parametrize("cfg_name", ["tiny_npc", "tiny_npc_k9", "tiny_npc_last", "npc_360hr"])
def test_skipping_the_masked_taps_changes_no_value(cfg_name):
    from s3prl_amd import _lib
    from s3prl_amd.synth import named_config, synth_weights

    torch = _torch()
    cfg = named_config(cfg_name)
    weights = synth_weights(cfg, 12)
    wavs = _wavs([16000, 2345, 3111], 13)
    outs = []
    for skip in (1, 0):
        enc = _encoder(cfg, weights)
        _lib.check(_lib.load().s3enc_set_handle_tuning(enc._h, b"npc_skip_taps", skip), "s3enc_set_handle_tuning")
        outs.append(enc.forward(wavs).clone())
        torch.cuda.synchronize()
        assert enc.status() == 0
    assert torch.isfinite(outs[0]).all() and np.array_equal(outs[0].cpu().numpy(), outs[1].cpu().numpy())
    assert _lib.load().s3enc_set_tuning(b"npc_skip_taps", 2) != 0 and b"0..1" in _lib.load().s3enc_last_error()


def test_an_utterance_alone_at_the_batchs_n_max_is_its_rows_in_the_batch():
    """Bit for bit, padded rows included: an utterance's rows depend on T and on nothing else of the batch.  Shards, permutations."""
    from s3prl_amd.synth import named_config, synth_weights

    torch = _torch()
    cfg = named_config("tiny_npc")
    enc = _encoder(cfg, synth_weights(cfg, 3))
    lengths = [4000, 2345, 800, 3111, 1999]
    wavs = _wavs(lengths, 5)
    full = enc.forward(wavs).clone()
    for b in range(len(wavs)):
        alone = enc.forward(wavs[b:b + 1], n_max=max(lengths)).clone()
        assert torch.equal(alone[:, 0], full[:, b]), b
    own = enc.forward(wavs[1:2]).clone()  # at its own T the last valid frames see a zero border instead of loud padded rows
    n = cfg.num_frames(lengths[1])
    assert own.shape[2] == n and torch.equal(own[0, 0], full[0, 1, :n]) and not torch.equal(own[1, 0], full[1, 1, :n])
    perm = [3, 0, 4, 2, 1]
    permuted = enc.forward([wavs[i] for i in perm]).clone()
    shard = enc.forward(wavs[2:4], n_max=max(lengths)).clone()  # padded to the global length: the full batch's rows
    torch.cuda.synchronize()
    for j, i in enumerate(perm):
        assert torch.equal(permuted[:, j], full[:, i])
    assert torch.equal(shard, full[:, 2:4])
    for b, n in enumerate(cfg.num_frames(v) for v in lengths):  # the rows behind an utterance's frames are loud in every state
        if n < full.shape[2]:
            assert (full[:, b, n:].abs().amax(dim=(1, 2)) > 0.05).all(), b
    assert enc.status() == 0


def test_one_handle_at_several_lengths_equals_fresh_handles():
    from s3prl_amd.synth import named_config, synth_weights

    torch = _torch()
    cfg = named_config("tiny_npc")
    weights = synth_weights(cfg, 2)
    enc = _encoder(cfg, weights)
    for n in (4000, 560, 16000, 2345):  # growing and shrinking: stale rows of a longer batch must not show as borders
        wavs = _wavs([n, max(560, n // 2)], n)
        got = enc.forward(wavs).clone()
        fresh = _encoder(cfg, weights)
        want = fresh.forward(wavs).clone()
        torch.cuda.synchronize()
        assert got.shape[2] == cfg.num_frames(n) and torch.isfinite(got).all()
        assert torch.equal(got, want), n
        fresh.close()
    assert enc.status() == 0


def test_frame_arithmetic_of_the_library():
    from s3prl_amd.synth import named_config, synth_weights

    cfg = named_config("tiny_npc")
    enc = _encoder(cfg, synth_weights(cfg, 0))
    assert [enc.num_frames(n) for n in (160000, 16000, 4000, 400, 399, 1)] == [998, 98, 23, 1, 0, 0]
    assert [enc.num_output_frames(n) for n in (160000, 400, 399)] == [998, 1, 0]
    assert [enc.valid_frames(n, 160000) for n in (160000, 16000, 4000, 400, 399)] == [998, 98, 23, 1, 0]
    assert enc.valid_frames(2345, 4000) == cfg.valid_frames(2345, 4000) == 13
    assert enc.downsample_rate() == 160 and enc.num_states() == 9
    last = named_config("tiny_npc_last")
    assert _encoder(last, synth_weights(last, 0)).num_states() == 6


@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("cfg_name", ["tiny_npc", "tiny_npc_last"])
def test_featurize_is_the_weighted_sum_of_the_states(cfg_name, normalize):
    from s3prl_amd import _lib
    from s3prl_amd.synth import named_config, synth_weights

    torch = _torch()
    lib = _lib.load()
    cfg = named_config(cfg_name)
    enc = _encoder(cfg, synth_weights(cfg, 4))
    wavs = _wavs([4000, 2345, 3111], 6)
    hs = enc.forward(wavs).clone()
    NS, B, T, D = hs.shape
    rng = np.random.default_rng(0)
    onehots = [[1.0 if i == j else 0.0 for i in range(NS)] for j in (0, 1, NS - 2, NS - 1)]
    for w in [list(rng.dirichlet(np.ones(NS)))] + onehots + [[0.0] * NS]:
        feat = enc.forward_featurized(wavs, w, normalize=normalize)
        want = torch.empty((B, T, D), device="cuda")
        wp = (C.c_float * NS)(*w)
        _lib.check(lib.s3enc_weighted_sum(_ptr(hs), B * T * D, NS, wp, int(normalize), B * T, D, _ptr(want), None), "s3enc_weighted_sum")
        torch.cuda.synchronize()
        if any(w):
            assert O.rel_err(feat.cpu().numpy(), want.cpu().numpy()) < OP_TOL, w
        else:
            assert not feat.any()
    assert enc.status() == 0


REFUSALS = [("dim_bottleneck", 32, "dim_bottleneck"), ("kernel_size", 14, "kernel_size must be odd"), ("mask_size", 7, "leaves no tap"),
            ("n_blocks", 9, "n_blocks must be 1..8"), ("width", 96, "multiple of 64"), ("width", 1088, "at most 1024"),
            ("num_mel_bins", 40, "multiple of 16"), ("dtype", "bf16", "fp32 only")]


@pytest.mark.parametrize("field, value, match", REFUSALS)
def test_create_refusals_are_error_codes_with_a_message(field, value, match):
    from s3prl_amd import _lib
    from s3prl_amd.synth import named_config, synth_weights

    _torch()
    lib = _lib.load()
    cfg = named_config("tiny_npc")
    ccfg, npc = _lib.make_config(cfg, value if field == "dtype" else "fp32"), _lib.make_npc_config(cfg)
    if field == "width":
        ccfg.conv_dim = ccfg.embed_dim = npc.hidden = value
    elif field != "dtype":
        setattr(npc, field, value)
    h = C.c_void_p()
    tensors = (_lib.S3Tensor * 1)()
    assert lib.s3enc_create_npc(C.byref(ccfg), C.byref(npc), tensors, 0, 0, C.byref(h)) != 0 and not h.value
    assert match in lib.s3enc_last_error().decode()


def test_missing_tensors_and_a_wrong_mask_are_named():
    from s3prl_amd import _lib
    from s3prl_amd.synth import named_config, synth_weights

    _torch()
    cfg = named_config("tiny_npc")
    for drop in ("blocks.1.bn2.running_var", "masked_convs.2.conv.weight", "blocks.0.conv.bias"):
        weights = synth_weights(cfg, 0)
        del weights[drop]
        with pytest.raises(_lib.S3EncError, match=drop):
            _encoder(cfg, weights)
    weights = synth_weights(cfg, 0)
    mask = np.ones((64, 64, 15), np.float32)
    mask[:, :, 3:12] = 0  # block 1's mask
    _encoder(cfg, dict(weights, **{"masked_convs.1.conv_mask": mask})).close()
    with pytest.raises(_lib.S3EncError, match="masked_convs.2.conv_mask"):
        _encoder(cfg, dict(weights, **{"masked_convs.2.conv_mask": mask}))


def test_forward_refusals():
    from s3prl_amd import _lib
    from s3prl_amd._lib import S3EncError
    from s3prl_amd.synth import named_config, synth_weights

    torch = _torch()
    cfg = named_config("tiny_npc")
    enc = _encoder(cfg, synth_weights(cfg, 0))
    wavs = _wavs([3000, 399], 1)
    with pytest.raises(S3EncError, match="feature_selection"):
        enc.forward(wavs[:1], selection="fairseq_layers")
    with pytest.raises(S3EncError, match="feature_selection"):
        enc.num_states("fairseq_layers_before_residual")
    with pytest.raises(ValueError, match="shorter than one analysis window"):
        enc.forward(wavs)  # the SHORT one of the batch, not only the longest, must hold a window
    with pytest.raises(ValueError, match="vq-wav2vec"):
        enc.forward(wavs[:1], aux={})
    lib = _lib.load()
    T = cfg.num_frames(3000)
    out = torch.full((9, 2, T, 64), float("nan"), device="cuda")
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
    """hub entry -> checkpoint written from synth_weights -> expert forward, CPU waveforms in, CPU states out, in hook order"""
    torch = _torch()
    import s3prl_amd.hub as amd
    from s3prl_amd.ckpt import save_checkpoint

    for name in ("npc/npc_tiny_pad", "npc/npc_tiny_last"):
        meta, cfg, weights, wavs, hs, norms = golden_loader(name)
        path = str(tmp_path / "c.pt")
        save_checkpoint(path, cfg, weights)
        expert = amd.npc_local(path)
        with torch.no_grad():
            out = expert([torch.from_numpy(w) for w in wavs])
        n = len(hs)
        assert set(out) == {"hidden_states", "last_hidden_state", "_hidden_states_info"} | {f"hidden_state_{i}" for i in range(n)}
        assert list(out["_hidden_states_info"]) == R.state_names(cfg)
        assert len(out["hidden_states"]) == n and out["last_hidden_state"] is out["hidden_states"][n - 1]
        for l in range(n):
            assert out["hidden_states"][l].device.type == "cpu" and list(out["hidden_states"][l].shape) == meta["shape"]
            assert O.rel_err(out["hidden_states"][l].numpy(), hs[l]) < FP32_TOL
