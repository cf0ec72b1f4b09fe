"""BYOL-S on the MI355X: the family pinned to the reference's own outputs (tests/golden/make_golden_byol_s.py) at the bound each
fixture records (FP32_TOL, or four times the reference's own fp32 rounding where that was measured larger), whole and per
(utterance, window) row, through the C ABI and through both hub names; the rows behind a short utterance equal to the reference's
values (they are not zeros); one handle at several (B, n_max) against fresh handles; the chunk size and the stem's two forms bit for
bit; the refusals; the shape entry points against config.py."""

import numpy as np
import pytest

from oracle import encoder_oracle as O

pytestmark = pytest.mark.gpu

FP32_TOL = 1e-4  # the project's fixture bound
TINY = ["byol_s/" + n for n in ["byol_s_tiny_eq", "byol_s_tiny_pad", "byol_s_tiny_win025", "byol_s_tiny_hop02", "byol_s_tiny_default"]]
FULL = {"byol_s_resnetish34": "byol_s/byol_s_resnetish34_pseudo", "byol_s_default": "byol_s/byol_s_default_pseudo"}
FILES = {"byol_s_default": "default2048_BYOLAs64x96-2105311814-e100-bs256-lr0003-rs42.pth",
         "byol_s_resnetish34": "resnetish34_BYOLAs64x96-2105271915-e100-bs256-lr0003-rs42.pth"}


def _torch():
    import torch

    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def _encoder(cfg, weights, dtype="fp32"):
    from s3prl_amd.encoder import HipEncoder

    return HipEncoder(cfg, weights, dtype=dtype)


def _forward(enc, wavs, **kw):
    torch = _torch()
    out = enc.forward([torch.from_numpy(w).cuda() for w in wavs], **kw)
    torch.cuda.synchronize()
    return out


def _tune(enc, key, value):
    from s3prl_amd import _lib

    _lib.check(_lib.load().s3enc_set_handle_tuning(enc._h, key, value), "s3enc_set_handle_tuning")


def _row_errs(g, h):
    return [O.rel_err(g[b, s], h[b, s]) for b in range(h.shape[0]) for s in range(h.shape[1])]


def _check_fixture(name, g, meta, hs, norms):
    h = hs[0]
    bound = meta["bound"]
    assert list(g.shape) == meta["shape"] and bound >= FP32_TOL
    whole, rows = O.rel_err(g, h), _row_errs(g, h)
    print(f"{name}: whole {whole:.2e}, worst (utterance, window) row {max(rows):.2e}, bound {bound:.1e}")
    assert np.isfinite(g).all() and whole < bound and max(rows) < bound, (name, whole, max(rows))
    assert abs(np.linalg.norm(g.astype(np.float64)) - norms[0]) / norms[0] < bound
    pad = [(b, s) for b, own in enumerate(meta["frames"]) for s in range(own, meta["windows"])]
    for b, s in pad:  # the reference's values for the windows behind the utterance, not zeros
        assert np.abs(g[b, s]).max() > 0 and O.rel_err(g[b, s], h[b, s]) < bound, (name, b, s)
    return pad


@pytest.mark.parametrize("name", TINY)
def test_tiny_fixture_through_the_c_abi(name, golden_loader):
    meta, cfg, weights, wavs, hs, norms = golden_loader(name)
    enc = _encoder(cfg, weights)
    try:
        assert enc.num_states() == 1 == meta["n_states"] and enc.downsample_rate() == meta["step"] == cfg.downsample_rate
        assert [enc.num_frames(n) for n in meta["lengths"]] == meta["frames"]
        g = _forward(enc, wavs)[0].cpu().numpy()
        pad = _check_fixture(name, g, meta, hs, norms)
        assert bool(pad) == (len(set(meta["frames"])) > 1)
        assert enc.status() == 0
    finally:
        enc.close()


def test_pad_rows_exist_in_the_fixtures(golden_loader):
    metas = [golden_loader(n)[0] for n in TINY + list(FULL.values())]
    assert sum(m["windows"] * len(m["frames"]) - sum(m["frames"]) for m in metas) >= 8


@pytest.mark.parametrize("hub", sorted(FULL))
def test_full_size_fixture_through_the_hub_name_and_the_c_abi(hub, golden_loader, tmp_path):
    """the released shapes once: the hub name, served from the cache directory, on a list of ragged waveforms returns the reference's
    hidden_states; the same weights through the C ABI give the same bits"""
    import s3prl_amd.hub as amd
    from s3prl_amd import download

    torch = _torch()
    meta, cfg, weights, wavs, hs, norms = golden_loader(FULL[hub])
    old = download.get_dir()
    download.set_dir(tmp_path)
    try:
        url = "https://github.com/GasserElbanna/serab-byols/raw/main/checkpoints/" + FILES[hub]
        torch.save({k: torch.from_numpy(v) for k, v in weights.items()}, str(download.cache_path(url)))
        expert = getattr(amd, hub)()
    finally:
        download.set_dir(old)
    assert expert.cfg == cfg and expert.get_downsample_rates("hidden_states") == 800
    out = expert([torch.from_numpy(w).cuda() for w in wavs])
    torch.cuda.synchronize()
    assert len(out["hidden_states"]) == 1 and out["last_hidden_state"] is out["hidden_states"][0]
    g = out["hidden_states"][0].cpu().numpy()
    pad = _check_fixture(FULL[hub], g, meta, hs, norms)
    assert len(pad) >= 4
    enc = expert._encoder_for(torch.device("cuda", torch.cuda.current_device()))
    assert enc.status() == 0
    assert np.array_equal(_forward(enc, wavs)[0].cpu().numpy(), g)


def test_hub_keywords_reach_the_windows(golden_loader):
    torch = _torch()
    from s3prl_amd.upstream.byol_s.expert import UpstreamExpert

    name = "byol_s/byol_s_tiny_hop02"
    meta, cfg, weights, wavs, hs, norms = golden_loader(name)
    sd = {k: torch.from_numpy(v) for k, v in weights.items()}
    with pytest.raises(ValueError, match=r"resnetish34 has \(3, 4, 6, 3\) blocks"):
        UpstreamExpert(sd, "resnetish34", window_secs=0.5, hop_secs=0.2)
    expert = UpstreamExpert(sd, "resnetish10", window_secs=0.5, hop_secs=0.2)
    assert expert.get_downsample_rates() == 3200 and expert.cfg == cfg
    g = expert([torch.from_numpy(w).cuda() for w in wavs])["hidden_states"][0].cpu().numpy()
    _check_fixture(name, g, meta, hs, norms)


@pytest.mark.parametrize("name", ["byol_s/byol_s_tiny_win025", "byol_s/byol_s_tiny_default"])
def test_chunk_size_and_stem_form_do_not_change_a_bit(name, golden_loader):
    """the network over the windows in chunks of 1, 2, 5 and the default; the fused stem against the split one"""
    meta, cfg, weights, wavs, _, _ = golden_loader(name)
    enc = _encoder(cfg, weights)
    try:
        base = _forward(enc, wavs)[0].cpu().numpy()
        assert np.isfinite(base).all()
        for chunk in (1, 2, 5):
            _tune(enc, b"byol_s_chunk", chunk)
            assert np.array_equal(_forward(enc, wavs)[0].cpu().numpy(), base), (name, chunk)
        _tune(enc, b"stem_fused", 1)
        assert np.array_equal(_forward(enc, wavs)[0].cpu().numpy(), base), (name, "fused stem, chunk 5")
        _tune(enc, b"byol_s_chunk", 1024)
        assert np.array_equal(_forward(enc, wavs)[0].cpu().numpy(), base), (name, "fused stem")
        _tune(enc, b"conv2d_n64", 0)
        assert np.array_equal(_forward(enc, wavs)[0].cpu().numpy(), base), (name, "128-wide n-tile")
        assert enc.status() == 0
    finally:
        enc.close()


def test_a_row_depends_on_the_batch_only_through_the_statistics(golden_loader):
    """a permuted batch gives permuted rows bit for bit (the statistics are sums over a fixed partition of the same N windows in
    another order: equal to rounding, so the rows agree to the bound, and where the two statistics come out equal in bits, in bits)"""
    name = "byol_s/byol_s_tiny_pad"
    meta, cfg, weights, wavs, _, _ = golden_loader(name)
    enc = _encoder(cfg, weights)
    try:
        full = _forward(enc, wavs)[0].cpu().numpy()
        stats = enc.debug_tap("stats").copy()
        perm = [2, 0, 1]
        permuted = _forward(enc, [wavs[i] for i in perm])[0].cpu().numpy()
        pstats = enc.debug_tap("stats").copy()
        assert np.abs(pstats - stats).max() <= 1e-6 * np.abs(stats).min()
        for j, i in enumerate(perm):
            assert O.rel_err(permuted[j], full[i]) < FP32_TOL
            if np.array_equal(pstats, stats):
                assert np.array_equal(permuted[j], full[i]), (j, i)
        # an utterance alone sees other statistics: its rows differ (that is the reference's behaviour, and why shards are refused)
        alone = _forward(enc, [wavs[1]])[0].cpu().numpy()
        assert alone.shape == full[1:2].shape and not np.array_equal(alone[0], full[1])
    finally:
        enc.close()


def test_one_handle_at_many_shapes_equals_fresh_handles(golden_loader):
    from s3prl_amd.synth import synth_wavs

    _, cfg, weights, _, _, _ = golden_loader("byol_s/byol_s_tiny_win025")
    batches = [synth_wavs(lens, 40 + i) for i, lens in enumerate([[4000], [9000, 7], [1, 4801, 8000], [3200, 3200]])]
    batches.append(batches[0])  # the first batch again behind longer and wider ones
    n_maxes = [None, 12000, None, None, None]
    enc = _encoder(cfg, weights)
    try:
        reused = [_forward(enc, b, n_max=nm)[0].cpu().numpy() for b, nm in zip(batches, n_maxes)]
        assert enc.status() == 0 and reused[1].shape[1] == 12000 // 1600 + 1
    finally:
        enc.close()
    for b, nm, want in zip(batches, n_maxes, reused):
        fresh = _encoder(cfg, weights)
        try:
            assert np.array_equal(_forward(fresh, b, n_max=nm)[0].cpu().numpy(), want)
        finally:
            fresh.close()
    assert np.array_equal(reused[0], reused[-1])


def test_shape_entry_points_against_config(golden_loader):
    for name in ("byol_s/byol_s_tiny_win025", "byol_s/byol_s_tiny_eq"):
        _, cfg, weights, _, _, _ = golden_loader(name)
        step = cfg.conv_layers[0][2]
        enc = _encoder(cfg, weights)
        try:
            assert enc.downsample_rate() == cfg.downsample_rate == step and enc.num_states() == cfg.num_hidden_states == 1
            for n in (1, step - 1, step, step + 1, 5 * step, 160000):
                assert enc.num_frames(n) == enc.num_output_frames(n) == cfg.num_frames(n) == n // step + 1, n
                for n_max in (n, n + step, 3 * n + 7):
                    assert enc.valid_frames(n, n_max) == cfg.valid_frames(n, n_max) == min(n // step + 1, n_max // step + 1)
            assert enc.embed_dim == 2048
        finally:
            enc.close()


def test_forward_refusals_by_name(golden_loader):
    from s3prl_amd import _lib

    torch = _torch()
    meta, cfg, weights, wavs, _, _ = golden_loader("byol_s/byol_s_tiny_win025")
    for dtype in ("bf16", "fp16", "fp32x3", "fp16x2"):
        with pytest.raises(ValueError, match=f"BYOL-S is built for compute dtype fp32 only; {dtype} is not built"):
            _encoder(cfg, weights, dtype=dtype)
    enc = _encoder(cfg, weights)
    try:
        dev = [torch.from_numpy(w).cuda() for w in wavs]
        for selection in ("fairseq_layers", "fairseq_layers_before_residual"):
            with pytest.raises(_lib.S3EncError, match="feature_selection is not defined for BYOL-S"):
                enc.num_states(selection)
        # featurize: one state, one weight; the weighted sum of one state at weight 1 is the state
        base = _forward(enc, wavs)[0]
        feat = enc.forward_featurized(dev, [1.0])
        torch.cuda.synchronize()
        assert torch.equal(feat, base)
        with pytest.raises(ValueError, match="one weight per state"):
            enc.forward_featurized(dev, [0.5, 0.5])
        B, T = base.shape[:2]
        opts = _lib.S3ForwardOpts(0, _lib.BF16, 0, 0, None)
        import ctypes as C

        ptrs = (C.c_void_p * B)(*[w.data_ptr() for w in dev])
        lens = (C.c_int64 * B)(*[w.numel() for w in dev])
        out = torch.empty((B, T, 2048), device="cuda")
        rc = _lib.load().s3enc_forward_ex(enc._h, ptrs, lens, B, 0, C.byref(opts), C.c_void_p(out.data_ptr()), B * T * 2048, None)
        assert rc != 0 and _lib.load().s3enc_last_error().decode() == "s3enc_forward: out_dtype must be S3ENC_F32 for a BYOL-S handle"
        opts = _lib.S3ForwardOpts(0, _lib.F32, 1, 0, None)
        rc = _lib.load().s3enc_forward_ex(enc._h, ptrs, lens, B, 0, C.byref(opts), C.c_void_p(out.data_ptr()), 0, None)
        assert rc != 0 and _lib.load().s3enc_last_error().decode() == "s3enc_forward: featurize needs feat_w"
    finally:
        enc.close()
