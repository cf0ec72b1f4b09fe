"""BYOL-A without a GPU: the float64 restatement tests/byol_a_ref.py against every fixture the reference produced (that pins the
yardstick of the GPU tests), the hub names and signatures, the checkpoint reader, the configuration round trip and the segment
arithmetic against the reference's own expressions."""

import inspect
import json
import os

import numpy as np
import pytest

import byol_a_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FP32_TOL = 1e-4
FIXTURES = ["byol_a_tiny_eq", "byol_a_tiny_pad", "byol_a_tiny_overlap", "byol_a_tiny_win025", "byol_a_2048_pseudo"]


def _rel(a, b):
    return float(np.linalg.norm(np.asarray(a, np.float64) - np.asarray(b, np.float64)) / np.linalg.norm(np.asarray(b, np.float64)))


# ---- the yardstick ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FIXTURES)
def test_the_float64_restatement_reproduces_the_fixture(name, golden_loader):
    meta, cfg, weights, wavs, hs, _ = golden_loader("byol_a/" + name)
    assert cfg.family == "byol_a" and cfg.conv_layers[0][1:] == (meta["window"], meta["stride"])
    out = R.forward(cfg, weights, wavs)
    h = hs[0]
    assert out["state"].shape == h.shape == tuple(meta["shape"]) and len(out["starts"]) == meta["segments"]
    rows = [_rel(out["state"][b, s], h[b, s]) for b in range(h.shape[0]) for s in range(h.shape[1])]
    assert _rel(out["state"], h) < FP32_TOL and max(rows) < FP32_TOL, (name, max(rows))
    assert [cfg.num_frames(n) for n in meta["lengths"]] == meta["frames"]
    for b, own in enumerate(meta["frames"]):  # rows past an utterance's own segments are the network's response, not zeros
        for s in range(own, meta["segments"]):
            assert np.abs(h[b, s]).max() > 0


def test_the_fixture_set_covers_what_it_should(golden_loader):
    metas = {n: golden_loader("byol_a/" + n)[0] for n in FIXTURES}
    pad = metas["byol_a_tiny_pad"]
    w, s = pad["window"], pad["stride"]
    assert any(n < w for n in pad["lengths"]) and any(n % s == 0 for n in pad["lengths"]) and any(n % s == 1 for n in pad["lengths"])
    assert metas["byol_a_tiny_overlap"]["stride"] < metas["byol_a_tiny_overlap"]["window"]
    assert (metas["byol_a_tiny_win025"]["window"], metas["byol_a_tiny_win025"]["stride"]) == (4000, 1600)
    assert metas["byol_a_2048_pseudo"]["shape"][2] == 2048 and 2 <= len(metas["byol_a_2048_pseudo"]["lengths"]) <= 3
    assert all("no torchaudio run" in m["reference"] for m in metas.values())


def test_the_mel_bank_is_sparse_and_matches_the_c_side_description():
    fb = R.mel_bank()
    assert fb.shape == (513, 64) and (np.count_nonzero(fb, axis=1) <= 2).all() and (fb >= 0).all() and fb.max() <= 1.0
    assert not fb[0].any() and not fb[-1].any()  # 0 Hz and 8000 Hz lie outside [60, 7800]


# ---- hub names --------------------------------------------------------------------------------------------------------------------
def test_hub_names_have_the_reference_signatures():
    import s3prl_amd.hub as amd
    from s3prl_amd.upstream.byol_a.expert import UpstreamExpert

    ref = json.load(open(os.path.join(ROOT, "tests", "golden", "byol_a", "reference_hub_byol_a.json")))
    everything = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_hub.json")))["options"]
    checked = []
    for name, params in ref["hubconfs"]["byol_a"]:
        assert name in everything and name in amd.options() and name in amd.options(only_registered_ckpt=True), name
        ours = inspect.signature(getattr(amd, name))
        assert [list(p) for p in params] == [[k, v.kind.name, repr(v.default)] for k, v in ours.parameters.items()], name
        checked.append(name)
    assert sorted(checked) == ["byol_a_1024", "byol_a_2048", "byol_a_512"]
    ours = inspect.signature(UpstreamExpert.__init__).parameters
    theirs = {p[0]: p for p in ref["expert_init"]}
    assert list(ours)[:6] == [p[0] for p in ref["expert_init"]] == ["self", "ckpt", "model_config", "feature_d", "window_secs", "stride_secs"]
    for k in ("window_secs", "stride_secs"):
        assert repr(ours[k].default) == theirs[k][2] == "1.0"


def test_hub_name_is_served_from_the_cache_directory(tmp_path):
    import torch

    import s3prl_amd.hub as amd
    from s3prl_amd import download
    from s3prl_amd.synth import named_config, synth_weights

    url = "https://github.com/nttcslab/byol-a/raw/master/pretrained_weights/AudioNTT2020-BYOLA-64x96d512.pth"
    cfg = named_config("byol_a_512")
    weights = synth_weights(cfg, 3)
    old = download.get_dir()
    download.set_dir(tmp_path)
    try:
        path = download.cache_path(url)
        assert path.name.split(".", 1)[1] == "AudioNTT2020-BYOLA-64x96d512.pth"
        torch.save({k: torch.from_numpy(v) for k, v in weights.items()}, str(path))
        expert = amd.byol_a_512()
        assert expert.cfg == cfg and expert.get_downsample_rates("hidden_states") == 16000 and expert.output_dim == 512
        assert expert.num_layers == 1 and expert.hidden_sizes == [512]
        assert set(expert._weights) == set(weights) and all(np.array_equal(expert._weights[k], weights[k]) for k in weights)
        half = amd.byol_a_512(window_secs=1.0, stride_secs=0.5)
        assert half.get_downsample_rates() == 8000
        assert half.cfg.conv_layers == [(512, 16000, 8000)]
        with pytest.raises(RuntimeError, match="inference-only"):
            expert([torch.zeros(16000, requires_grad=True)])
        if not torch.cuda.is_available():
            with pytest.raises(RuntimeError, match="no CPU fallback"):
                expert([torch.zeros(16000)])
        with pytest.raises(ValueError, match="feature_d 1024 was asked for, but fc.0.weight has 512 rows"):
            torch.save({k: torch.from_numpy(v) for k, v in weights.items()},
                       str(download.cache_path(url.replace("d512", "d1024"))))
            amd.byol_a_1024()
    finally:
        download.set_dir(old)


# ---- the checkpoint reader ----------------------------------------------------------------------------------------------------------
def test_checkpoint_reader_prefixes_and_refusals(tmp_path):
    import torch

    from s3prl_amd.ckpt import byol_a_state_dict, load_byol_a_checkpoint, load_checkpoint, save_checkpoint
    from s3prl_amd.synth import named_config, synth_weights

    cfg = named_config("tiny_byol_a")
    weights = synth_weights(cfg, 11)
    assert set(weights) == {f"features.{k}.{leaf}" for k in (0, 4, 8) for leaf in ("weight", "bias")} | \
        {f"features.{k}.{leaf}" for k in (1, 5, 9) for leaf in ("weight", "bias", "running_mean", "running_var")} | \
        {"fc.0.weight", "fc.0.bias", "fc.3.weight", "fc.3.bias"}
    assert all(weights[f"features.{k}.running_var"].min() >= 0.5 for k in (1, 5, 9))
    plain = {k: torch.from_numpy(v) for k, v in weights.items()}
    plain["features.1.num_batches_tracked"] = torch.tensor(100)
    prefixed = {"state_dict": {"learner.online_encoder.net." + k: v for k, v in plain.items()}}
    prefixed["state_dict"]["learner.target_encoder_ema"] = torch.zeros(3)  # no fc. / features. component: dropped
    for form in (plain, prefixed, {"state_dict": plain}):
        got_cfg, got = load_byol_a_checkpoint(form, feature_d=64)
        assert got_cfg == cfg and set(got) == set(weights) and all(np.array_equal(got[k], weights[k]) for k in weights)
    # the reference's rule, key by key (byol_a.py:66-74)
    assert set(byol_a_state_dict({"a.fc.0.weight": 1, "features.0.bias": 2, "x.features.4.weight": 3, "proj.weight": 4})) == \
        {"fc.0.weight", "features.0.bias", "features.4.weight"}
    with pytest.raises(ValueError, match="feature_d 2048 was asked for, but fc.0.weight has 64 rows"):
        load_byol_a_checkpoint(plain, feature_d=2048)
    missing = dict(plain)
    del missing["features.5.running_var"]
    with pytest.raises(ValueError, match="missing parameter features.5.running_var"):
        load_byol_a_checkpoint(missing)
    bad = dict(plain)
    bad["fc.3.weight"] = torch.zeros(64, 32)
    with pytest.raises(ValueError, match="fc.3.weight has shape"):
        load_byol_a_checkpoint(bad)
    # a file, through the family dispatcher
    path = str(tmp_path / "byol_a.pth")
    save_checkpoint(path, cfg, weights)
    got_cfg, got = load_checkpoint(path, "byol_a")
    assert got_cfg == cfg and all(np.array_equal(got[k], weights[k]) for k in weights)
    got_cfg, _ = load_byol_a_checkpoint(path, window_secs=0.25, stride_secs=0.1)
    assert got_cfg == named_config("tiny_byol_a_win025")


# ---- configuration ------------------------------------------------------------------------------------------------------------------
def test_config_round_trip_and_refusals():
    from s3prl_amd import _lib
    from s3prl_amd.config import EncoderConfig, byol_a_config
    from s3prl_amd.synth import named_config

    cfg = named_config("byol_a_2048")
    assert cfg.conv_layers == [(2048, 16000, 16000)] and cfg.encoder_layers == 0 and cfg.num_hidden_states == 1
    assert cfg.downsample_rate == 16000 and named_config("tiny_byol_a_overlap").downsample_rate == 8000
    again = EncoderConfig(**cfg.__dict__)
    again.validate()
    assert again == cfg
    c = _lib.make_byol_a_config(named_config("tiny_byol_a_win025"))
    assert (c.feature_d, c.window, c.stride) == (64, 4000, 1600)
    assert abs(c.norm_mean + 5.4919195) < 1e-6 and abs(c.norm_std - 5.0389895) < 1e-6 and abs(c.bn_eps - 1e-5) < 1e-12
    assert _lib.FAMILY["byol_a"] == 12
    # the C block as the header lays it out
    header = open(os.path.join(ROOT, "include", "s3enc.h")).read()
    block = header[header.index("typedef struct s3enc_byol_a_config {"):header.index("} s3enc_byol_a_config;")]
    fields = [ln.split(";")[0].split()[-1] for ln in block.splitlines()[1:] if ";" in ln]
    assert fields == [f[0] for f in _lib.S3ByolAConfig._fields_]
    assert "S3ENC_BYOL_A = 12" in header
    with pytest.raises(ValueError, match="cannot be reflect-padded"):
        byol_a_config(64, window_secs=0.032)       # 512 samples
    with pytest.raises(ValueError, match="fewer than 8 frames"):
        byol_a_config(64, window_secs=0.069)       # 1104 samples
    byol_a_config(64, window_secs=0.07)            # 1120 samples: 8 frames
    with pytest.raises(ValueError, match="multiple of 4"):
        byol_a_config(66)
    with pytest.raises(ValueError, match="stride must be at least one sample"):
        byol_a_config(64, stride_secs=0.0)
    with pytest.raises(_lib.S3EncError, match="needs a byol_a configuration"):
        _lib.make_byol_a_config(named_config("tiny_vggish"))


# ---- the segment arithmetic ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("window_secs, stride_secs", [(1.0, 1.0), (1.0, 0.5), (0.25, 0.1), (0.95, 0.3)])
def test_segment_arithmetic_is_the_references(window_secs, stride_secs):
    """S, the starts and the padded length for lengths around every multiple of the stride, against expert.py:83-86,119 as
    written there"""
    from s3prl_amd.config import byol_a_config

    cfg = byol_a_config(64, window_secs=window_secs, stride_secs=stride_secs)
    _, window, stride = cfg.conv_layers[0]
    assert (window, stride) == (int(window_secs * 16000), int(stride_secs * 16000))
    for k in range(0, 5):
        for delta in (-1, 0, 1, 2):
            n = k * stride + delta
            if n < 1:
                continue
            start_points = list(range(0, n, int(stride_secs * 16000)))
            padded_max_wav_len = start_points[-1] + int(window_secs * 16000)
            max_h_len = len(range(0, n, int(stride_secs * 16000)))
            assert cfg.num_frames(n) == len(start_points) == max_h_len, n
            assert cfg.valid_frames(n, n + 3 * stride) == len(start_points)
            starts, padded = R.segment_plan([n, 1], window, stride)
            assert starts == start_points and padded == padded_max_wav_len
    assert cfg.num_frames(0) == 0
