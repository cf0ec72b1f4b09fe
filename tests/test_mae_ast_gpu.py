"""MAE-AST on the MI355X: the family pinned to the reference model's own outputs (tests/golden/make_golden_mae_ast.py) to FP32_TOL,
whole and per (utterance, time step) row — the rows behind an utterance's valid count included: they are the reference's values —
through the C ABI and through the hub names on a written checkpoint file; float64 per row on fresh waveforms; an utterance alone
against the same utterance inside a ragged batch; handle reuse; both forms of the patch embedding; status; the refusals."""

import dataclasses

import numpy as np
import pytest

from oracle import encoder_oracle as O

import mae_ast_ref as R

pytestmark = pytest.mark.gpu

FP32_TOL = 1e-4  # the project's fixture bound
TINY = ["mae_ast/" + n for n in ["tiny_patch_eq", "tiny_patch_pad", "tiny_frame_pad", "tiny_preln_pad", "tiny_k3x32_pad"]]
FULL = {"mae_ast_patch": "mae_ast/mae_ast_patch_pseudo", "mae_ast_frame": "mae_ast/mae_ast_frame_pseudo"}
URLS = {"mae_ast_patch": "https://www.cs.utexas.edu/~harwath/model_checkpoints/mae_ast/chunk_patch_75_12LayerEncoder.pt",
        "mae_ast_frame": "https://www.cs.utexas.edu/~harwath/model_checkpoints/mae_ast/random_frame_75_12LayerEncoder.pt"}


def _torch():
    import torch

    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def _encoder(cfg, weights, dtype="fp32"):
    from s3prl_amd.encoder import HipEncoder

    return HipEncoder(cfg, weights, dtype=dtype)


def _forward(enc, wavs, **kw):
    torch = _torch()
    out = enc.forward([torch.from_numpy(np.asarray(w, np.float32)).cuda() for w in wavs], **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _row_errs(g, h):
    return [O.rel_err(g[b, t], h[b, t]) for b in range(h.shape[0]) for t in range(h.shape[1])]


def _check_fixture(name, g, meta, hs, norms):
    """g: (NS, B, Tt, V * D) as the handle wrote it; hs: the reference's states, sub-sampled by (t_stride, c_stride)"""
    ts, cs = meta["t_stride"], meta["c_stride"]
    assert list(g.shape[1:]) == meta["shape"] and g.shape[0] == meta["n_states"] == len(hs)
    worst = 0.0
    for l, h in enumerate(hs):
        sub = g[l][:, ::ts, ::cs]
        assert sub.shape == h.shape
        whole, rows = O.rel_err(sub, h), _row_errs(sub, h)
        worst = max(worst, whole, max(rows))
        assert np.isfinite(g[l]).all() and whole < FP32_TOL and max(rows) < FP32_TOL, (name, l, whole, max(rows))
        assert abs(np.linalg.norm(g[l].astype(np.float64)) - norms[l]) / norms[l] < FP32_TOL, (name, l)
    print(f"{name}: worst of whole / (utterance, time step) row over {len(hs)} states {worst:.2e}")
    return [(b, t) for b, own in enumerate(meta["frames"]) for t in range(own, meta["steps"])]


@pytest.mark.parametrize("name", TINY)
def test_tiny_fixture_through_the_c_abi(name, golden_loader):
    meta, cfg, weights, wavs, hs, norms = golden_loader(name)
    enc = _encoder(cfg, weights)
    try:
        nmax = max(meta["lengths"])
        assert enc.num_states() == cfg.encoder_layers == meta["n_states"] and enc.downsample_rate() == meta["downsample"] == cfg.ma_kt * 160
        assert enc.num_frames(nmax) == meta["steps"] and [enc.valid_frames(n, nmax) for n in meta["lengths"]] == meta["frames"]
        assert [enc.num_frames(n) for n in meta["lengths"]] == [f // cfg.ma_kt for f in meta["fbank_frames"]]
        g = _forward(enc, wavs)
        pad = _check_fixture(name, g, meta, hs, norms)
        assert bool(pad) == (len(set(meta["frames"])) > 1)
        for b, t in pad:  # padded rows are the reference's values (checked per row above), not zeros
            assert np.abs(g[-1][b, t]).max() > 0
        assert enc.status() == 0
    finally:
        enc.close()


def test_padded_rows_exist_in_the_fixtures(golden_loader):
    assert sum(m["steps"] * len(m["frames"]) - sum(m["frames"]) for m in (golden_loader(n)[0] for n in TINY)) >= 8


def _hub_expert(tmp_path, cfg, weights, name):
    """the hub name served from the cache directory: a written checkpoint file under the released file's cache name"""
    import s3prl_amd.hub as amd
    from s3prl_amd import download
    from s3prl_amd.ckpt import save_checkpoint

    old = download.get_dir()
    download.set_dir(tmp_path)
    try:
        save_checkpoint(str(download.cache_path(URLS[name])), cfg, weights)
        return getattr(amd, name)()
    finally:
        download.set_dir(old)


@pytest.mark.parametrize("hub", sorted(FULL))
def test_full_size_fixture_through_the_hub_name(hub, golden_loader, tmp_path):
    torch = _torch()
    meta, cfg, weights, wavs, hs, norms = golden_loader(FULL[hub])
    expert = _hub_expert(tmp_path, cfg, weights, hub)
    assert expert.cfg == cfg and (cfg.encoder_embed_dim, cfg.encoder_layers, cfg.encoder_attention_heads) == (768, 12, 12)
    assert expert.get_downsample_rates("hidden_states") == meta["downsample"] == {"mae_ast_patch": 2560, "mae_ast_frame": 320}[hub]
    out = expert([torch.from_numpy(w).cuda() for w in wavs])
    torch.cuda.synchronize()
    assert len(out["hidden_states"]) == 12 and out["last_hidden_state"] is out["hidden_states"][-1]
    assert out["_hidden_states_info"] == tuple(f"state_{i}" for i in range(12))
    g = np.stack([h.cpu().numpy() for h in out["hidden_states"]])
    assert g.shape[-1] == {"mae_ast_patch": 6144, "mae_ast_frame": 768}[hub] == expert.hidden_sizes[0]
    _check_fixture(FULL[hub], g, meta, hs, norms)
    assert expert._encoder_for(torch.device("cuda", torch.cuda.current_device())).status() == 0


@pytest.mark.parametrize("config, lengths", [("tiny_mae_ast", [9300, 3000, 6100]), ("tiny_mae_ast_frame", [3333, 1000]),
                                             ("tiny_mae_ast_preln", [7000]), ("tiny_mae_ast_k3x32", [4000, 4400, 1500])])
def test_against_float64_per_row_on_fresh_waveforms(config, lengths):
    from s3prl_amd.synth import named_config, synth_wavs, synth_weights

    cfg = named_config(config)
    weights = synth_weights(cfg, 91)
    wavs = synth_wavs(lengths, 92)
    enc = _encoder(cfg, weights)
    try:
        g = _forward(enc, wavs)
        assert enc.status() == 0
    finally:
        enc.close()
    want = R.forward(cfg, weights, wavs)["states"]
    assert g.shape == (cfg.encoder_layers,) + want[0].shape
    rows = [e for l in range(cfg.encoder_layers) for e in _row_errs(g[l], want[l])]
    print(f"{config} {lengths}: worst row {max(rows):.2e}")
    assert max(rows) < FP32_TOL


@pytest.mark.parametrize("config, kt", [("tiny_mae_ast", 16), ("tiny_mae_ast_frame", 2)])
def test_an_utterance_alone_against_inside_a_ragged_batch(config, kt):
    """utterances whose frame count is a whole number of patches: alone, their tokens and keys are the ones they have inside a
    longer batch, so their valid rows agree to FP32_TOL (the batch only changes tile placement and the number of masked keys)"""
    from s3prl_amd.synth import named_config, synth_wavs, synth_weights

    cfg = named_config(config)
    weights = synth_weights(cfg, 93)
    frames = [2 * kt, 3 * kt]
    lengths = [400 + 160 * (f - 1) for f in frames] + [400 + 160 * (5 * kt + 1)]
    wavs = synth_wavs(lengths, 94)
    enc = _encoder(cfg, weights)
    try:
        full = _forward(enc, wavs)
        for b in range(2):
            alone = _forward(enc, [wavs[b]])
            own = frames[b] // kt
            assert alone.shape[2] == own == enc.valid_frames(lengths[b], max(lengths))
            for l in range(cfg.encoder_layers):
                assert max(_row_errs(alone[l], full[l][b:b + 1, :own])) < FP32_TOL, (b, l)
        assert enc.status() == 0
    finally:
        enc.close()


def test_one_handle_at_many_lengths_equals_fresh_handles(golden_loader):
    from s3prl_amd.synth import synth_wavs

    _, cfg, weights, _, _, _ = golden_loader("mae_ast/tiny_patch_pad")
    batches = [synth_wavs(lens, 40 + i) for i, lens in enumerate([[3000], [20000, 400 + 160 * 15], [2960, 8000, 12000], [5000, 5000]])]
    batches.append(batches[0])  # the first batch again behind longer and wider ones
    enc = _encoder(cfg, weights)
    try:
        reused = [_forward(enc, b) for b in batches]
        assert enc.status() == 0
    finally:
        enc.close()
    for b, want in zip(batches, reused):
        fresh = _encoder(cfg, weights)
        try:
            assert np.array_equal(_forward(fresh, b), want)
        finally:
            fresh.close()
    assert np.array_equal(reused[0], reused[-1])


@pytest.mark.parametrize("name", ["mae_ast/tiny_patch_pad", "mae_ast/tiny_k3x32_pad"])
def test_both_forms_of_the_patch_embedding_in_the_forward(name, golden_loader):
    from s3prl_amd import _lib

    meta, cfg, weights, wavs, hs, norms = golden_loader(name)
    enc = _encoder(cfg, weights)
    try:
        fused = _forward(enc, wavs)
        _lib.check(_lib.load().s3enc_set_handle_tuning(enc._h, b"patch_embed_fused", 0), "s3enc_set_handle_tuning")
        two = _forward(enc, wavs)
        _check_fixture(name + " (two-step form)", two, meta, hs, norms)
        assert max(_row_errs(two[-1], fused[-1])) < FP32_TOL
        enc.profile_enable(True)
        _forward(enc, wavs)
        assert "patch_embed_two_step" in {p["name"] for p in enc.profile_read()}
        assert enc.status() == 0
    finally:
        enc.close()


def test_featurized_sum_is_the_weighted_sum_of_the_states(golden_loader):
    torch = _torch()
    _, cfg, weights, wavs, _, _ = golden_loader("mae_ast/tiny_preln_pad")
    enc = _encoder(cfg, weights)
    try:
        g = _forward(enc, wavs).astype(np.float64)
        w = [0.5, 0.0, 0.25]
        f = enc.forward_featurized([torch.from_numpy(x).cuda() for x in wavs], w)
        torch.cuda.synchronize()
        want = sum(wi * g[i] for i, wi in enumerate(w))
        assert max(_row_errs(f.cpu().numpy(), want)) < FP32_TOL
        from s3prl_amd import _lib

        with pytest.raises(_lib.S3EncError, match="feat_normalize is not built for an MAE-AST handle"):
            enc.forward_featurized([torch.from_numpy(x).cuda() for x in wavs], w, normalize=True)
    finally:
        enc.close()


def test_refusals_by_name(golden_loader):
    from s3prl_amd import _lib
    from s3prl_amd.config import mae_ast_config

    _, cfg, weights, wavs, _, _ = golden_loader("mae_ast/tiny_patch_eq")
    for dtype in ("bf16", "fp16", "fp32x3", "fp16x2"):
        with pytest.raises(ValueError, match=f"MAE-AST is built for compute dtype fp32 only; {dtype} is not built"):
            _encoder(cfg, weights, dtype=dtype)
    enc = _encoder(cfg, weights)
    try:
        with pytest.raises(ValueError, match="utterance 1 has 399 samples, fewer than one 400-sample analysis window"):
            _forward(enc, [np.zeros(5000, np.float32), np.zeros(399, np.float32)])
        with pytest.raises(ValueError, match="the batch has 15 frames, fewer than one patch of 16 frames"):
            _forward(enc, [np.zeros(400 + 160 * 14, np.float32)])
        with pytest.raises(ValueError, match="the batch needs 648 position rows, the handle holds 640"):
            _forward(enc, [np.zeros(400 + 160 * (81 * 16 - 1), np.float32)])
        with pytest.raises(_lib.S3EncError, match="feature_selection is not defined for MAE-AST"):
            enc.num_states("fairseq_layers")
        # the C ABI repeats the forward's refusals: the Python checks bypassed
        import ctypes as C

        torch = _torch()
        lib = _lib.load()

        def raw(lengths):
            held = [torch.zeros(n, device="cuda") for n in lengths]
            B = len(held)
            out = torch.empty(cfg.encoder_layers * B * 200 * 1024, device="cuda")
            ptrs = (C.c_void_p * B)(*[w.data_ptr() for w in held])
            opts = _lib.S3ForwardOpts(_lib.SEL_HIDDEN, _lib.F32, 0, 0, None)
            return lib.s3enc_forward_ex(enc._h, ptrs, (C.c_int64 * B)(*lengths), B, max(lengths), C.byref(opts), C.c_void_p(out.data_ptr()),
                                        B * 200 * 1024, None)

        for lengths, msg in (([5000, 399], "utterance 1 has 399 samples, fewer than one 400-sample analysis window"),
                             ([400 + 160 * 14], "fewer than one patch of 16 frames"),
                             ([400 + 160 * (81 * 16 - 1)], "needs 648 position rows, the handle holds 640")):
            with pytest.raises(_lib.S3EncError, match=msg):
                _lib.check(raw(lengths), "s3enc_forward")
    finally:
        enc.close()
    # the create entry repeats what it can see of the configuration: the Python check bypassed
    for field, value, msg in (("ma_feature_dim", 80, "feature_dim must be 128"), ("ma_kc", 8, "ast_kernel_size_chan must be 16, 32, 64 or 128"),
                              ("ma_kt", 40, "ast_kernel_size_time must be 1..32"), ("encoder_attention_heads", 4, "must be 64")):
        bad = dataclasses.replace(cfg, **{field: value})
        bad.validate = lambda: None
        w = dict(weights)
        if field in ("ma_kc", "ma_kt"):
            w["post_extract_proj.weight"] = np.zeros((128, bad.ma_kt * bad.ma_kc), np.float32)
        with pytest.raises(_lib.S3EncError, match=msg):
            _encoder(bad, w)
    # the other create entries refuse the family by name
    import ctypes as C

    ccfg = _lib.make_config(cfg, "fp32")
    h = C.c_void_p()
    tensors = (_lib.S3Tensor * 1)()
    rc = _lib.load().s3enc_create(C.byref(ccfg), tensors, 0, 0, C.byref(h))
    with pytest.raises(_lib.S3EncError, match="s3enc_create_mae_ast"):
        _lib.check(rc, "s3enc_create")
    with pytest.raises(ValueError, match="enc_conv_pos=True is not built"):
        mae_ast_config(ma_enc_conv_pos=True)
