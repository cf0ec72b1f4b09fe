"""DeCoAR / DeCoAR-layers on the MI355X, every test through the C ABI: the model pinned to the reference's own outputs
(tests/golden/make_golden_decoar.py) per utterance, both experts by hub name, the subsampled front end against float64, featurize,
shards, handle reuse and the refusals.  The recurrent op itself: tests/test_lstm_bidir_gpu.py."""

import ctypes as C

import numpy as np
import pytest

from oracle import encoder_oracle as O

import decoar_ref as R

pytestmark = pytest.mark.gpu

FP32_TOL = 1e-4  # the project's fixture bound (tests/test_apc_gpu.py)
OP_TOL = 2e-5    # the project's op bound
FIXTURES = ["decoar/" + n for n in ["decoar_tiny_pad", "decoar_tiny_eq", "decoar_tiny_t2", "decoar_tiny_l1", "decoar_layers_tiny_pad",
                                    "decoar_layers_tiny_h192"]]


def _torch():
    import torch

    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _encoder(cfg, weights, dtype="fp32"):
    from s3prl_amd.encoder import HipEncoder

    return HipEncoder(cfg, weights, dtype=dtype)


def _score_per_utterance(got, hs, lens, meta, what):
    ts, cs = meta["t_stride"], meta["c_stride"]
    worst = 0.0
    for l in range(len(hs)):
        g = got[l].cpu().numpy()
        for b, n in enumerate(lens):
            assert not g[b, n:].any(), (what, l, b, "rows behind the length must be exactly 0")
            worst = max(worst, O.rel_err(g[b, :n:ts, ::cs], hs[l][b, :-(-n // ts)]))
    return worst


@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_fp32_from_waveforms(name, golden_loader):
    """s3enc_create_decoar + forward on the fixture's waveforms: every state per utterance, and the full-tensor norms."""
    torch = _torch()
    meta, cfg, weights, wavs, hs, norms = golden_loader(name)
    enc = _encoder(cfg, weights)
    assert enc.num_states() == len(hs) == meta["n_states"]
    out = enc.forward([torch.from_numpy(w).cuda() for w in wavs])
    torch.cuda.synchronize()
    assert list(out.shape[1:]) == meta["shape"]
    err = _score_per_utterance(out, hs, meta["frames"], meta, name)
    print(f"{name}: from waveforms, worst per-(state, utterance) rel-err {err:.2e}")
    assert err < FP32_TOL, (name, err)
    for l in range(len(hs)):
        n = np.linalg.norm(out[l].cpu().numpy().astype(np.float64))
        assert abs(n - norms[l]) / norms[l] < FP32_TOL
    assert enc.status() == 0


@pytest.mark.parametrize("cfg_name, lengths", [("tiny_decoar_sub2", [4000, 2345, 3111, 560]), ("tiny_decoar_layers", [4000, 560, 720]),
                                               ("tiny_decoar_h192", [1999, 4000])])
def test_family_against_float64_per_utterance_and_per_frame(cfg_name, lengths):
    """Shapes no fixture holds — every second frame (2 fbank frames = ONE model frame next to longer utterances), a two-frame
    utterance in the middle of a batch — against decoar_ref from the waveforms: every state per utterance and per frame."""
    from s3prl_amd.synth import named_config, synth_wavs, synth_weights

    torch = _torch()
    cfg = named_config(cfg_name)
    weights = synth_weights(cfg, 21)
    wavs = synth_wavs(lengths, 22)
    ref = R.forward(cfg, weights, wavs)
    enc = _encoder(cfg, weights)
    out = enc.forward([torch.from_numpy(w).cuda() for w in wavs]).cpu().numpy()
    assert ref["lengths"] == [enc.num_frames(n) for n in lengths] == [enc.valid_frames(n, max(lengths)) for n in lengths]
    assert out.shape == (cfg.num_hidden_states, len(lengths), max(ref["lengths"]), 2 * cfg.decoar_hidden)
    worst_u = worst_f = 0.0
    for l, want in enumerate(ref["hidden_states"]):
        for b, n in enumerate(ref["lengths"]):
            assert not out[l, b, n:].any()
            worst_u = max(worst_u, O.rel_err(out[l, b, :n], want[b, :n]))
            worst_f = max(worst_f, max(O.rel_err(out[l, b, t], want[b, t]) for t in range(n)))
    print(f"{cfg_name}: worst per utterance {worst_u:.2e}, worst per frame {worst_f:.2e}")
    assert worst_u < FP32_TOL and worst_f < FP32_TOL
    assert enc.status() == 0


def test_released_shape_against_float64():
    """80 / 1024 / 4 on two short ragged utterances (48 and 33 frames) against decoar_ref from the waveforms: the four states of
    decoar_layers per utterance and per frame, and decoar's single state = the last of them, bit for bit.  (No reference-generated
    fixture exists at this shape: tests/golden/make_golden_decoar.py says why.)"""
    from s3prl_amd.synth import named_config, synth_wavs, synth_weights

    torch = _torch()
    per, one = named_config("decoar_layers"), named_config("decoar")
    weights = synth_weights(per, 607)
    lengths = [8000, 5555]
    wavs = synth_wavs(lengths, 707)
    ref = R.forward(per, weights, wavs)
    assert ref["lengths"] == [48, 33] and min(ref["gate_std"]) >= 1.0
    dev = [torch.from_numpy(w).cuda() for w in wavs]
    enc = _encoder(per, weights)
    hs = enc.forward(dev).clone()
    out = hs.cpu().numpy()
    assert out.shape == (4, 2, 48, 2048)
    worst_u = worst_f = 0.0
    for l, want in enumerate(ref["hidden_states"]):
        for b, n in enumerate(ref["lengths"]):
            assert not out[l, b, n:].any()
            worst_u = max(worst_u, O.rel_err(out[l, b, :n], want[b, :n]))
            worst_f = max(worst_f, max(O.rel_err(out[l, b, t], want[b, t]) for t in range(n)))
    print(f"released shape: worst per utterance {worst_u:.2e}, worst per frame {worst_f:.2e}")
    assert worst_u < FP32_TOL and worst_f < FP32_TOL
    last = _encoder(one, weights).forward(dev)
    assert last.shape[0] == 1 and torch.equal(last[0], hs[3])
    assert enc.status() == 0


def test_frame_arithmetic_of_the_library():
    from s3prl_amd.synth import named_config, synth_weights

    cfg = named_config("tiny_decoar")
    enc = _encoder(cfg, synth_weights(cfg, 0))
    assert [enc.num_frames(n) for n in (160000, 16000, 8000, 5555, 560, 400, 399, 1)] == [998, 98, 48, 33, 2, 1, 0, 0]
    assert [enc.num_output_frames(n) for n in (160000, 560, 399)] == [998, 2, 0]
    assert enc.valid_frames(2345, 4000) == cfg.valid_frames(2345, 4000) == 13
    assert enc.downsample_rate() == 160 and enc.num_states() == 1
    sub = named_config("tiny_decoar_sub2")
    enc2 = _encoder(sub, synth_weights(sub, 0))
    assert [enc2.num_frames(n) for n in (8000, 5555, 560, 400, 399)] == [24, 17, 1, 1, 0]  # the true frame count: ceil(f / 2)
    assert enc2.downsample_rate() == 160 and enc2.num_states() == 2 and enc2.valid_frames(5555, 8000) == 17


def test_both_experts_by_hub_name_on_one_checkpoint(tmp_path, golden_loader):
    """hub entry -> ONE checkpoint written from synth_weights -> both experts' forward, CPU waveforms in, CPU states out: the
    reference's dict, the fixture's states, and decoar's state = the last of decoar_layers'."""
    torch = _torch()
    import s3prl_amd.hub as amd
    from s3prl_amd.ckpt import save_checkpoint

    meta, cfg, weights, wavs, hs, norms = golden_loader("decoar/decoar_layers_tiny_pad")
    path = str(tmp_path / "c.pt")
    save_checkpoint(path, cfg, weights)
    one, per = getattr(amd, "decoar_local")(path), getattr(amd, "decoar_layers_local")(path)
    cpu = [torch.from_numpy(w) for w in wavs]
    with torch.no_grad():
        a, b = one(cpu), per(cpu)
    assert set(a) == set(b) == {"hidden_states", "last_hidden_state"}  # the reference's experts are plain modules: no hook keys
    assert isinstance(a["hidden_states"], list) and len(a["hidden_states"]) == 1 and len(b["hidden_states"]) == cfg.decoar_layers == 3
    assert a["last_hidden_state"] is a["hidden_states"][-1] and b["last_hidden_state"] is b["hidden_states"][-1]
    assert all(h.device.type == "cpu" and h.dtype == torch.float32 for h in b["hidden_states"])
    assert torch.equal(a["hidden_states"][0], b["hidden_states"][-1])
    err = _score_per_utterance(torch.stack(b["hidden_states"]), hs, meta["frames"], meta, "expert")
    print(f"decoar_layers expert: worst per-(state, utterance) rel-err {err:.2e}")
    assert err < FP32_TOL


@pytest.mark.parametrize("normalize", [False, True])
def test_featurize_is_the_weighted_sum_of_the_states(normalize):
    from s3prl_amd import _lib
    from s3prl_amd.synth import named_config, synth_wavs, synth_weights

    torch = _torch()
    lib = _lib.load()
    cfg = named_config("tiny_decoar_layers")
    enc = _encoder(cfg, synth_weights(cfg, 4))
    wavs = [torch.from_numpy(w).cuda() for w in synth_wavs([4000, 2345, 3111], 6)]
    hs = enc.forward(wavs).clone()
    NS, B, T, D = hs.shape
    assert NS == 3
    for w in ([0.2, 0.3, 0.5], [0.0, 0.0, 1.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 0.0]):
        feat = enc.forward_featurized(wavs, w, normalize=normalize)
        want = torch.empty((B, T, D), device="cuda")
        wp = (C.c_float * 3)(*w)
        _lib.check(lib.s3enc_weighted_sum(_ptr(hs), B * T * D, 3, wp, int(normalize), B * T, D, _ptr(want), None), "s3enc_weighted_sum")
        torch.cuda.synchronize()
        if any(w):
            assert O.rel_err(feat.cpu().numpy(), want.cpu().numpy()) < OP_TOL, w
        else:
            assert not feat.any()
    one = named_config("tiny_decoar")
    enc1 = _encoder(one, synth_weights(one, 4))
    assert torch.equal(enc1.forward_featurized(wavs, [1.0]), enc1.forward(wavs)[0])
    assert enc.status() == 0


def test_permutation_and_shard_are_bit_exact():
    from s3prl_amd.synth import named_config, synth_wavs, synth_weights

    torch = _torch()
    cfg = named_config("tiny_decoar_layers")
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


def test_one_handle_at_three_batch_shapes_equals_fresh_handles():
    from s3prl_amd.synth import named_config, synth_wavs, synth_weights

    torch = _torch()
    cfg = named_config("tiny_decoar_layers")
    weights = synth_weights(cfg, 2)
    enc = _encoder(cfg, weights)
    for lengths in ([4000, 2000], [560], [16000, 2345, 8000, 3111, 720]):
        wavs = [torch.from_numpy(w).cuda() for w in synth_wavs(lengths, sum(lengths))]
        got = enc.forward(wavs).clone()
        fresh = _encoder(cfg, weights)
        want = fresh.forward(wavs).clone()
        torch.cuda.synchronize()
        assert got.shape[1:3] == (len(lengths), cfg.num_frames(max(lengths))) and torch.isfinite(got).all()
        assert torch.equal(got, want), lengths
        fresh.close()
    assert enc.status() == 0


def test_create_refusals_are_error_codes_with_a_message():
    from s3prl_amd import _lib
    from s3prl_amd.synth import named_config, synth_weights

    _torch()
    lib = _lib.load()
    cfg = named_config("tiny_decoar")
    h = C.c_void_p()
    tensors = (_lib.S3Tensor * 1)()
    for dtype, field, value, match in (("bf16", None, None, "fp32 only"), ("fp32", "num_layers", 5, "num_layers must be 1..4"),
                                       ("fp32", "subsample", 3, "subsample must be 1 or 2")):
        ccfg, dc = _lib.make_config(cfg, dtype), _lib.make_decoar_config(cfg)
        if field:
            setattr(dc, field, value)
        assert lib.s3enc_create_decoar(C.byref(ccfg), C.byref(dc), tensors, 0, 0, C.byref(h)) != 0 and not h.value
        assert match in lib.s3enc_last_error().decode()
    # the wrong create entry, in both directions
    ccfg, apc = _lib.make_config(cfg, "fp32"), _lib.make_apc_config(named_config("tiny_apc"))
    assert lib.s3enc_create_apc(C.byref(ccfg), C.byref(apc), tensors, 0, 0, C.byref(h)) != 0 and b"s3enc_create_decoar" in lib.s3enc_last_error()
    assert lib.s3enc_create(C.byref(ccfg), tensors, 0, 0, C.byref(h)) != 0 and b"s3enc_create_decoar" in lib.s3enc_last_error()
    acfg = _lib.make_config(named_config("tiny_apc"), "fp32")
    assert lib.s3enc_create_decoar(C.byref(acfg), C.byref(_lib.make_decoar_config(cfg)), tensors, 0, 0, C.byref(h)) != 0
    assert b"S3ENC_DECOAR only" in lib.s3enc_last_error()
    # with a valid configuration a missing tensor is named
    weights = synth_weights(cfg, 0)
    del weights["backward_lstm.weight_hh_l1"]
    with pytest.raises(_lib.S3EncError, match="backward_lstm.weight_hh_l1"):
        _encoder(cfg, weights)


def test_forward_refusals():
    from s3prl_amd import _lib
    from s3prl_amd._lib import S3EncError
    from s3prl_amd.synth import named_config, synth_wavs, synth_weights

    torch = _torch()
    cfg = named_config("tiny_decoar")
    enc = _encoder(cfg, synth_weights(cfg, 0))
    wavs = [torch.from_numpy(w).cuda() for w in synth_wavs([3000, 400], 1)]  # 400 samples: ONE fbank frame
    with pytest.raises(S3EncError, match="feature_selection"):
        enc.forward(wavs[:1], selection="fairseq_layers")
    with pytest.raises(S3EncError, match="feature_selection"):
        enc.num_states("fairseq_layers_before_residual")
    with pytest.raises(ValueError, match="fewer than 2 analysis windows"):
        enc.forward(wavs)  # the SHORT one of the batch
    with pytest.raises(ValueError, match="vq-wav2vec"):
        enc.forward(wavs[:1], aux={})
    with pytest.raises(ValueError, match="at most 128 utterances"):
        enc.forward([wavs[0]] * 129)
    # the C entry itself: one frame beside a longer utterance is refused with a message, nothing is launched
    lib = _lib.load()
    T = cfg.num_frames(3000)
    out = torch.full((1, 2, T, 128), float("nan"), device="cuda")
    ptrs = (C.c_void_p * 2)(wavs[0].data_ptr(), wavs[1].data_ptr())
    lens = (C.c_int64 * 2)(3000, 400)
    assert lib.s3enc_forward(enc._h, ptrs, lens, 2, 0, _ptr(out), 2 * T * 128, None) != 0
    assert b"fewer than 2 analysis windows" in lib.s3enc_last_error()
    opts = _lib.S3ForwardOpts(_lib.SEL_HIDDEN, _lib.F16, 0, 0, None)
    assert lib.s3enc_forward_ex(enc._h, ptrs, lens, 1, 0, C.byref(opts), _ptr(out), 2 * T * 128, None) != 0
    assert b"S3ENC_F32" in lib.s3enc_last_error()
    opts = _lib.S3ForwardOpts(_lib.SEL_LAYER_OUT, _lib.F32, 0, 0, None)
    assert lib.s3enc_forward_ex(enc._h, ptrs, lens, 1, 0, C.byref(opts), _ptr(out), 2 * T * 128, None) != 0
    assert b"feature_selection" in lib.s3enc_last_error()
    torch.cuda.synchronize()
    assert torch.isnan(out).all()
