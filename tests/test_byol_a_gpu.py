"""BYOL-A on the MI355X: the family pinned to the reference's own outputs (tests/golden/make_golden_byol_a.py) to FP32_TOL, whole
and per (utterance, segment) row, through the hub name's expert and through the C ABI; pad rows equal to the reference's values
(they are not zeros); a segment's row bit for bit whatever the batch around it; handle reuse; status; the refusals."""

import numpy as np
import pytest

from oracle import encoder_oracle as O

import byol_a_ref as R

pytestmark = pytest.mark.gpu

FP32_TOL = 1e-4  # the project's fixture bound
TINY = ["byol_a/" + n for n in ["byol_a_tiny_eq", "byol_a_tiny_pad", "byol_a_tiny_overlap", "byol_a_tiny_win025"]]
FULL = "byol_a/byol_a_2048_pseudo"


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


def _row_errs(g, h):
    return [O.rel_err(g[b, s], h[b, s]) for b in range(h.shape[0]) for s in range(h.shape[1])]


def _check_fixture(name, g, meta, hs, norms):
    h = hs[0]
    assert list(g.shape) == meta["shape"]
    whole, rows = O.rel_err(g, h), _row_errs(g, h)
    print(f"{name}: whole {whole:.2e}, worst (utterance, segment) row {max(rows):.2e}")
    assert np.isfinite(g).all() and whole < FP32_TOL and max(rows) < FP32_TOL, (name, whole, max(rows))
    assert abs(np.linalg.norm(g.astype(np.float64)) - norms[0]) / norms[0] < FP32_TOL
    pad = [(b, s) for b, own in enumerate(meta["frames"]) for s in range(own, meta["segments"])]
    for b, s in pad:  # the reference's values for the zero-padded segments, not zeros
        assert np.abs(g[b, s]).max() > 0 and O.rel_err(g[b, s], h[b, s]) < FP32_TOL, (name, b, s)
    return pad


@pytest.mark.parametrize("name", TINY)
def test_tiny_fixture_through_the_c_abi(name, golden_loader):
    meta, cfg, weights, wavs, hs, norms = golden_loader(name)
    enc = _encoder(cfg, weights)
    try:
        assert enc.num_states() == 1 == meta["n_states"] and enc.downsample_rate() == meta["stride"]
        assert [enc.num_frames(n) for n in meta["lengths"]] == meta["frames"]
        g = _forward(enc, wavs)[0].cpu().numpy()
        pad = _check_fixture(name, g, meta, hs, norms)
        assert bool(pad) == (len(set(meta["frames"])) > 1)
        assert enc.status() == 0
    finally:
        enc.close()


def test_pad_rows_exist_in_the_fixtures(golden_loader):
    assert sum(golden_loader(n)[0]["segments"] * len(golden_loader(n)[0]["frames"]) - sum(golden_loader(n)[0]["frames"])
               for n in TINY + [FULL]) >= 8


def _hub_expert(tmp_path, cfg, weights, name, **kwds):
    """the hub name served from the cache directory: a synthetic file under the released file's cache name, key prefixes as a
    training wrapper leaves them"""
    import torch

    import s3prl_amd.hub as amd
    from s3prl_amd import download

    d = cfg.conv_layers[0][0]
    url = f"https://github.com/nttcslab/byol-a/raw/master/pretrained_weights/AudioNTT2020-BYOLA-64x96d{d}.pth"
    old = download.get_dir()
    download.set_dir(tmp_path)
    try:
        sd = {"model." + k: torch.from_numpy(v) for k, v in weights.items()}
        sd["model.features.1.num_batches_tracked"] = torch.tensor(7)
        torch.save({"state_dict": sd}, str(download.cache_path(url)))
        return getattr(amd, name)(**kwds)
    finally:
        download.set_dir(old)


def test_full_size_fixture_through_the_hub_name_and_the_c_abi(golden_loader, tmp_path):
    """the released size once: hub.byol_a_2048 on a list of ragged waveforms returns the reference's hidden_states; the same
    weights through the C ABI give the same bits"""
    torch = _torch()
    meta, cfg, weights, wavs, hs, norms = golden_loader(FULL)
    expert = _hub_expert(tmp_path, cfg, weights, "byol_a_2048")
    assert expert.cfg == cfg and expert.get_downsample_rates("hidden_states") == 16000
    out = expert([torch.from_numpy(w).cuda() for w in wavs])
    torch.cuda.synchronize()
    assert len(out["hidden_states"]) == 1 and out["last_hidden_state"] is out["hidden_states"][0]
    g = out["hidden_states"][0].cpu().numpy()
    _check_fixture(FULL, g, meta, hs, norms)
    enc = expert._encoder_for(torch.device("cuda", torch.cuda.current_device()))
    assert enc.status() == 0
    assert np.array_equal(_forward(enc, wavs)[0].cpu().numpy(), g)


@pytest.mark.parametrize("name, hub, kwds", [("byol_a/byol_a_tiny_overlap", "byol_a_512", dict(window_secs=1.0, stride_secs=0.5))])
def test_hub_keywords_reach_the_segments(name, hub, kwds, golden_loader, tmp_path):
    """window_secs / stride_secs through a hub name (the tiny weights under the 512 name are refused by feature_d: the check works;
    the expert built directly takes them)"""
    torch = _torch()
    from s3prl_amd.upstream.byol_a.expert import UpstreamExpert

    meta, cfg, weights, wavs, hs, norms = golden_loader(name)
    with pytest.raises(ValueError, match="feature_d 512 was asked for, but fc.0.weight has 64 rows"):
        UpstreamExpert({k: torch.from_numpy(v) for k, v in weights.items()}, None, 512, **kwds)
    expert = UpstreamExpert({k: torch.from_numpy(v) for k, v in weights.items()}, None, 64, **kwds)
    assert expert.get_downsample_rates() == 8000
    g = expert([torch.from_numpy(w).cuda() for w in wavs])["hidden_states"][0].cpu().numpy()
    _check_fixture(name, g, meta, hs, norms)


@pytest.mark.parametrize("name", ["byol_a/byol_a_tiny_pad", "byol_a/byol_a_tiny_win025"])
def test_a_segments_row_depends_on_the_segment_only(name, golden_loader):
    """an utterance forwarded alone gives the rows of its own segments bit for bit (the rows behind them depend on the batch's
    longest utterance only through their number); a permuted batch gives permuted rows"""
    meta, cfg, weights, wavs, _, _ = golden_loader(name)
    enc = _encoder(cfg, weights)
    try:
        full = _forward(enc, wavs)[0].cpu().numpy()
        for b, w in enumerate(wavs):
            alone = _forward(enc, [w])[0].cpu().numpy()
            own = meta["frames"][b]
            assert alone.shape[1] == own and np.array_equal(alone[0], full[b, :own]), (name, b)
            padded = _forward(enc, [w], n_max=max(meta["lengths"]))[0].cpu().numpy()
            assert np.array_equal(padded[0], full[b]), (name, b)
        perm = [2, 0, 1]
        permuted = _forward(enc, [wavs[i] for i in perm])[0].cpu().numpy()
        for j, i in enumerate(perm):
            assert np.array_equal(permuted[j], full[i]), (name, j, i)
        assert enc.status() == 0
    finally:
        enc.close()


def test_one_handle_at_many_lengths_equals_fresh_handles(golden_loader):
    from s3prl_amd.synth import synth_wavs

    _, cfg, weights, _, _, _ = golden_loader("byol_a/byol_a_tiny_pad")
    batches = [synth_wavs(lens, 40 + i) for i, lens in enumerate([[16000], [50000, 7], [1, 16001, 33000], [20000, 20000]])]
    batches.append(batches[0])  # the first batch again behind longer and wider ones
    enc = _encoder(cfg, weights)
    try:
        reused = [_forward(enc, b)[0].cpu().numpy() for b in batches]
        assert enc.status() == 0
    finally:
        enc.close()
    for b, want in zip(batches, reused):
        fresh = _encoder(cfg, weights)
        try:
            assert np.array_equal(_forward(fresh, b)[0].cpu().numpy(), want)
        finally:
            fresh.close()
    assert np.array_equal(reused[0], reused[-1])


def test_the_two_front_end_forms_and_tile_widths_in_the_forward(golden_loader):
    """the GEMM-form front end within FP32_TOL of the fixture; the 128-wide n-tile bit for bit"""
    from s3prl_amd import _lib

    name = "byol_a/byol_a_tiny_pad"
    meta, cfg, weights, wavs, hs, norms = golden_loader(name)
    enc = _encoder(cfg, weights)
    try:
        base = _forward(enc, wavs)[0].cpu().numpy()
        _lib.check(_lib.load().s3enc_set_handle_tuning(enc._h, b"conv2d_n64", 0), "s3enc_set_handle_tuning")
        assert np.array_equal(_forward(enc, wavs)[0].cpu().numpy(), base)
        _lib.check(_lib.load().s3enc_set_handle_tuning(enc._h, b"melspec_fft", 0), "s3enc_set_handle_tuning")
        _check_fixture(name + " (gemm form)", _forward(enc, wavs)[0].cpu().numpy(), meta, hs, norms)
    finally:
        enc.close()


def test_against_float64_per_row(golden_loader):
    """the restatement in float64 on fresh waveforms (not the fixtures'): every (utterance, segment) row to FP32_TOL"""
    from s3prl_amd.synth import synth_wavs

    _, cfg, weights, _, _, _ = golden_loader("byol_a/byol_a_tiny_overlap")
    wavs = synth_wavs([20001, 8000, 31999], 77)
    enc = _encoder(cfg, weights)
    try:
        g = _forward(enc, wavs)[0].cpu().numpy()
    finally:
        enc.close()
    want = R.forward(cfg, weights, wavs)["state"]
    assert g.shape == want.shape and max(_row_errs(g, want)) < FP32_TOL


def test_refusals_by_name(golden_loader):
    from s3prl_amd.config import byol_a_config
    from s3prl_amd.synth import synth_weights

    _, cfg, weights, _, _, _ = golden_loader("byol_a/byol_a_tiny_eq")
    for dtype in ("bf16", "fp16", "fp32x3", "fp16x2"):
        with pytest.raises(ValueError, match=f"BYOL-A is built for compute dtype fp32 only; {dtype} is not built"):
            _encoder(cfg, weights, dtype=dtype)
    with pytest.raises(ValueError, match="cannot be reflect-padded"):
        byol_a_config(feature_d=64, window_secs=0.03)
    with pytest.raises(ValueError, match="fewer than 8 frames"):
        byol_a_config(feature_d=64, window_secs=0.06)
    # stride > window: an utterance that ends between two segments makes the reference's zero padding negative (it raises)
    gap = _encoder(byol_a_config(feature_d=64, window_secs=0.25, stride_secs=0.5), weights)
    try:
        from s3prl_amd import _lib as L_

        assert _forward(gap, [np.zeros(12000, np.float32)]).shape[2] == 2  # 8000 + 4000: reaches exactly
        with pytest.raises(L_.S3EncError, match="utterance 1 has 12001 samples, more than the 12000 the 2 segments of this batch reach"):
            _forward(gap, [np.zeros(9000, np.float32), np.zeros(12001, np.float32)])
    finally:
        gap.close()
    # the C ABI repeats both: a configuration whose Python check is bypassed
    from s3prl_amd import _lib

    for secs, msg in ((0.03, "cannot be reflect-padded"), (0.06, "fewer than 8 frames")):
        bad = byol_a_config(feature_d=64)
        bad.conv_layers = [(64, int(secs * 16000), 16000)]
        bad.ba_window_secs = secs
        bad.validate = lambda: None
        with pytest.raises(_lib.S3EncError, match=msg):
            _encoder(bad, weights)
