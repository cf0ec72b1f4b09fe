"""SSAST on the MI355X: the family against the fixtures of tests/golden/ssast/ (the float64 restatement on a synthetic checkpoint in
the released key layout: no run of the reference stands behind them, see make_golden_ssast.py) to FP32_TOL, whole and per (utterance,
state row) — the rows behind an utterance's own length included: they are the reference's values; float64 per row on fresh waveforms;
an utterance alone against the same utterance in a ragged batch of equal max_len, bit for bit; chunked against unchunked workspace,
bit for bit; both forms of the embedding; handle reuse; the featurized sum; the blocks' LayerNorm eps; the hub name on a written
full-width checkpoint file; the refusals."""

import ctypes as C
import dataclasses

import numpy as np
import pytest

from oracle import encoder_oracle as O

import ssast_ref as R

pytestmark = pytest.mark.gpu

FP32_TOL = 1e-4  # the project's fixture bound
TINY = ["ssast/" + n for n in ["tiny_patch_cut", "tiny_frame_cut", "tiny_patch_short", "tiny_patch_eq", "tiny_patch_interp",
                               "tiny_frame_interp", "tiny_patch_d192"]]
URLS = {"ssast_patch_base": "https://www.dropbox.com/s/ewrzpco95n9jdz6/SSAST-Base-Patch-400.pth?dl=1",
        "ssast_frame_base": "https://www.dropbox.com/s/nx6nl4d4bl71sm8/SSAST-Base-Frame-400.pth?dl=1"}


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


def _tune(enc, key, value):
    from s3prl_amd import _lib

    _lib.check(_lib.load().s3enc_set_handle_tuning(enc._h, key.encode(), int(value)), "s3enc_set_handle_tuning")


def _row_errs(g, h):
    return [O.rel_err(g[b, t], h[b, t]) for b in range(h.shape[0]) for t in range(h.shape[1])]


def _check_fixture(name, g, meta, hs, norms):
    """g: (NS, B, T_out, f_dim * D) as the handle wrote it; hs: the fixture's states, sub-sampled by (t_stride, c_stride)"""
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
    print(f"{name}: worst of whole / (utterance, state row) over {len(hs)} states {worst:.2e}")


@pytest.mark.parametrize("name", TINY)
def test_tiny_fixture_through_the_c_abi(name, golden_loader):
    meta, cfg, weights, wavs, hs, norms = golden_loader(name)
    enc = _encoder(cfg, weights)
    try:
        nmax = max(meta["lengths"])
        assert enc.num_states() == cfg.encoder_layers == meta["n_states"] and enc.downsample_rate() == meta["downsample"] == cfg.ss_tstride * 160
        assert enc.num_frames(nmax) == meta["steps"] == cfg.num_frames(nmax) <= meta["uncut_steps"]
        assert [enc.valid_frames(n, nmax) for n in meta["lengths"]] == meta["frames"]
        g = _forward(enc, wavs)
        _check_fixture(name, g, meta, hs, norms)
        for b, own in enumerate(meta["frames"]):  # rows behind an utterance's own length are the reference's values, not zeros
            for t in range(own, meta["steps"]):
                assert np.abs(g[-1][b, t]).max() > 0
    finally:
        enc.close()


def test_the_fixtures_cover_the_cut_the_silent_window_and_the_short_utterance(golden_loader):
    metas = {n: golden_loader(n)[0] for n in TINY}
    assert sum(m["steps"] < m["uncut_steps"] for m in metas.values()) >= 3
    assert any(any(row) and not all(row) for m in metas.values() for row in m["silent_windows"])  # a wholly silent window behind a live one
    assert min(min(m["lengths"]) for m in metas.values()) < 400
    assert {m["tokens"] for m in metas.values()} == {50, 51}


@pytest.mark.parametrize("config, lengths", [("tiny_ssast_patch", [8000 * 2 + 1, 300, 11111]), ("tiny_ssast_frame", [7999, 12001]),
                                             ("tiny_ssast_patch_w1", [16001, 5000]), ("tiny_ssast_frame_interp", [1])])
def test_against_float64_per_row_on_fresh_waveforms(config, lengths):
    from s3prl_amd.synth import named_config, synth_wavs, synth_weights

    cfg = named_config(config)
    weights = synth_weights(cfg, 191)
    wavs = synth_wavs(lengths, 192)
    enc = _encoder(cfg, weights)
    try:
        g = _forward(enc, wavs)
    finally:
        enc.close()
    want = R.forward(cfg, weights, wavs)["states"]
    assert g.shape == (cfg.encoder_layers,) + want[0].shape
    rows = [e for l in range(cfg.encoder_layers) for e in _row_errs(g[l], want[l])]
    print(f"{config} {lengths}: worst row {max(rows):.2e}")
    assert np.isfinite(g).all() and max(rows) < FP32_TOL


@pytest.mark.parametrize("config", ["tiny_ssast_patch", "tiny_ssast_frame"])
def test_an_utterance_alone_against_inside_a_ragged_batch_of_equal_max_len(config):
    """windows are independent sequences and nothing is masked: with n_max the same, an utterance's rows are its bits anywhere"""
    from s3prl_amd.synth import named_config, synth_wavs, synth_weights

    cfg = named_config(config)
    weights = synth_weights(cfg, 193)
    lengths = [20001, 9000, 350]
    wavs = synth_wavs(lengths, 194)
    enc = _encoder(cfg, weights)
    try:
        full = _forward(enc, wavs)
        for b in (1, 2, 0):
            alone = _forward(enc, [wavs[b]], n_max=max(lengths))
            assert alone.shape[1:] == (1,) + full.shape[2:]
            assert np.array_equal(alone[:, 0], full[:, b]), b
    finally:
        enc.close()


@pytest.mark.parametrize("config", ["tiny_ssast_patch", "tiny_ssast_frame"])
def test_chunked_against_unchunked_workspace_bit_for_bit(config):
    from s3prl_amd.synth import named_config, synth_wavs, synth_weights

    cfg = named_config(config)
    weights = synth_weights(cfg, 195)
    wavs = synth_wavs([24001, 8000, 17000], 196)  # 3 x 4 windows
    enc = _encoder(cfg, weights)
    try:
        whole = _forward(enc, wavs)
        for tokens in (1, 5 * 51, 7 * 51):  # one window per pass; 5 and 7 windows per pass: a ragged last chunk
            _tune(enc, "ssast_chunk", tokens)
            assert np.array_equal(_forward(enc, wavs), whole), tokens
    finally:
        enc.close()


@pytest.mark.parametrize("name", ["ssast/tiny_patch_cut", "ssast/tiny_frame_cut"])
def test_both_forms_of_the_patch_embedding_in_the_forward(name, golden_loader):
    meta, cfg, weights, wavs, hs, norms = golden_loader(name)
    enc = _encoder(cfg, weights)
    try:
        fused = _forward(enc, wavs)
        _tune(enc, "patch_strided_fused", 0)
        two = _forward(enc, wavs)
        _check_fixture(name + " (two-step form)", two, meta, hs, norms)
        assert max(_row_errs(two[-1], fused[-1])) < FP32_TOL
        enc.profile_enable(True)
        _forward(enc, wavs)
        names = {p["name"] for p in enc.profile_read()}
        assert "patch_strided_two_step" in names and "ssast_emit" in names and "ssast_fbank" in names
    finally:
        enc.close()


def test_one_handle_at_many_lengths_equals_fresh_handles(golden_loader):
    from s3prl_amd.synth import synth_wavs

    _, cfg, weights, _, _, _ = golden_loader("ssast/tiny_patch_cut")
    batches = [synth_wavs(lens, 140 + i) for i, lens in enumerate([[3000], [20000, 9000], [100, 8000, 12000], [8001, 8001]])]
    batches.append(batches[0])  # the first batch again behind longer and wider ones
    enc = _encoder(cfg, weights)
    try:
        reused = [_forward(enc, b) for b in batches]
    finally:
        enc.close()
    for b, want in zip(batches, reused):
        fresh = _encoder(cfg, weights)
        try:
            assert np.array_equal(_forward(fresh, b), want)
        finally:
            fresh.close()
    assert np.array_equal(reused[0], reused[-1])


def test_featurized_sum_is_the_weighted_sum_of_the_states(golden_loader):
    torch = _torch()
    from s3prl_amd import _lib

    _, cfg, weights, wavs, _, _ = golden_loader("ssast/tiny_patch_cut")
    enc = _encoder(cfg, weights)
    try:
        g = _forward(enc, wavs).astype(np.float64)
        dev = [torch.from_numpy(x).cuda() for x in wavs]
        for w in ([0.25, 0.75], [0.0, 2.0], [1.5, 0.0], [0.0, 0.0]):
            f = enc.forward_featurized(dev, w)
            torch.cuda.synchronize()
            want = sum(wi * g[i] for i, wi in enumerate(w))
            if any(w):
                assert max(_row_errs(f.cpu().numpy(), want)) < FP32_TOL, w
            else:
                assert not f.cpu().numpy().any()
        with pytest.raises(_lib.S3EncError, match="feat_normalize is not built for an SSAST handle"):
            enc.forward_featurized(dev, [0.5, 0.5], normalize=True)
    finally:
        enc.close()


def test_the_blocks_layernorm_runs_at_the_checkpoints_eps():
    """Patch tokens, prefix and position rows scaled down so that the residual stream entering block 0 has a variance near 1e-4: there
    1e-6 against the engine's fixed 1e-5 moves LayerNorm 1's output by about 4 %, far above the bound.  The float64 restatement at 1e-5
    must sit outside the bound of the one at 1e-6 (the test can tell them apart), and the handle inside the bound of the latter."""
    from s3prl_amd.synth import named_config, synth_wavs, synth_weights

    cfg = named_config("tiny_ssast_patch")
    weights = dict(synth_weights(cfg, 197))
    for k in ("module.v.patch_embed.proj.weight", "module.v.patch_embed.proj.bias", "module.v.cls_token", "module.v.dist_token",
              "module.v.pos_embed"):
        weights[k] = (weights[k] * np.float32(0.01)).astype(np.float32)
    wavs = synth_wavs([8000, 5000], 198)
    want = R.forward(cfg, weights, wavs)["states"]
    wrong = R.forward(cfg, weights, wavs, eps=1e-5)["states"]
    apart = min(_row_errs(wrong[0], want[0]))
    assert apart > 10 * FP32_TOL, apart
    enc = _encoder(cfg, weights)
    try:
        g = _forward(enc, wavs)
    finally:
        enc.close()
    rows = [e for l in range(cfg.encoder_layers) for e in _row_errs(g[l], want[l])]
    print(f"eps 1e-6: worst row {max(rows):.2e}; eps 1e-5 would be at least {apart:.2e} away in every row of state 0")
    assert max(rows) < FP32_TOL


@pytest.mark.parametrize("hub", sorted(URLS))
def test_by_hub_name_from_a_full_width_checkpoint_file(hub, tmp_path):
    """the released widths (D = 768, 12 heads, FFN 3072) with depth cut to 2, served from the cache directory at window_secs = 1.0"""
    torch = _torch()
    import s3prl_amd.hub as amd
    from s3prl_amd import download
    from s3prl_amd.ckpt import save_checkpoint
    from s3prl_amd.synth import named_config, synth_wavs, synth_weights

    cfg = named_config(hub + "_l2")
    weights = synth_weights(cfg, 199)
    old = download.get_dir()
    download.set_dir(tmp_path)
    try:
        save_checkpoint(str(download.cache_path(URLS[hub])), cfg, weights)
        expert = getattr(amd, hub)(window_secs=1.0)
    finally:
        download.set_dir(old)
    assert expert.cfg == cfg and (cfg.encoder_embed_dim, cfg.encoder_layers, cfg.encoder_attention_heads) == (768, 2, 12)
    rate = {"ssast_patch_base": 1600, "ssast_frame_base": 160}[hub]
    assert expert.get_downsample_rates("hidden_states") == rate
    wavs = synth_wavs([16001, 9000], 200)
    out = expert([torch.from_numpy(w).cuda() for w in wavs])
    torch.cuda.synchronize()
    T, width = {"ssast_patch_base": (11, 9216), "ssast_frame_base": (101, 768)}[hub]  # 18 and 198 rows before the cut
    assert len(out["hidden_states"]) == 2 and out["last_hidden_state"] is out["hidden_states"][-1]
    g = np.stack([h.cpu().numpy() for h in out["hidden_states"]])
    assert g.shape == (2, 2, T, width) and expert.hidden_sizes == [width, width]
    want = R.forward(cfg, weights, wavs)["states"]
    rows = [e for l in range(2) for e in _row_errs(g[l], want[l])]
    print(f"{hub}: worst row {max(rows):.2e}")
    assert max(rows) < FP32_TOL


def test_refusals_by_name(golden_loader):
    from s3prl_amd import _lib

    _, cfg, weights, wavs, _, _ = golden_loader("ssast/tiny_patch_eq")
    for dtype in ("bf16", "fp16", "fp32x3", "fp16x2"):
        with pytest.raises(ValueError, match=f"SSAST is built for compute dtype fp32 only; {dtype} is not built"):
            _encoder(cfg, weights, dtype=dtype)
    enc = _encoder(cfg, weights)
    try:
        with pytest.raises(_lib.S3EncError, match="feature_selection is not defined for SSAST"):
            enc.num_states("fairseq_layers")
    finally:
        enc.close()
    # the create entry repeats what it can see of the configuration: the Python check bypassed
    from s3prl_amd.ckpt import ssast_hot_path

    ready = ssast_hot_path("w", cfg, weights)
    for field, value, msg in (("encoder_attention_heads", 4, "embed_dim / heads must be 64"), ("ss_fstride", 9, "fstride must be even"),
                              ("ss_fshape", 48, "fshape must be 16, 32, 64 or 128"), ("ss_tshape", 40, "tshape must be 1..32"),
                              ("layer_norm_first", False, "ssast blocks are pre-LN"), ("ss_window_secs", 0.01, "window_samples must be")):
        bad = dataclasses.replace(cfg, **{field: value})
        bad.validate = lambda: None
        with pytest.raises(_lib.S3EncError, match=msg):
            _encoder(bad, ready)
    for dtype, word in ((1, "bf16"), (4, "fp16x2")):  # the operand modes by name, the Python check bypassed
        ccfg = _lib.make_config(cfg, "fp32")
        ccfg.compute_dtype = dtype
        block = _lib.make_ssast_config(cfg)
        h = C.c_void_p()
        tensors = (_lib.S3Tensor * 1)()
        rc = _lib.load().s3enc_create_ssast(C.byref(ccfg), C.byref(block), tensors, 0, 0, C.byref(h))
        with pytest.raises(_lib.S3EncError, match=f"SSAST is built for compute dtype fp32 only; {word} is not built"):
            _lib.check(rc, "s3enc_create_ssast")
    # the other create entries refuse the family by name
    ccfg = _lib.make_config(cfg, "fp32")
    h = C.c_void_p()
    tensors = (_lib.S3Tensor * 1)()
    rc = _lib.load().s3enc_create(C.byref(ccfg), tensors, 0, 0, C.byref(h))
    with pytest.raises(_lib.S3EncError, match="s3enc_create_ssast"):
        _lib.check(rc, "s3enc_create")
    block = _lib.S3MaeAstConfig()
    rc = _lib.load().s3enc_create_mae_ast(C.byref(ccfg), C.byref(block), tensors, 0, 0, C.byref(h))
    with pytest.raises(_lib.S3EncError, match="the SSAST family needs its window / patch block: use s3enc_create_ssast"):
        _lib.check(rc, "s3enc_create_mae_ast")
