"""BYOL-S without a GPU: the float64 restatement tests/byol_s_ref.py against every fixture the reference produced (that pins the
yardstick of the GPU tests), the window geometry against frame_audio's own loop, the statistics with their division by the number of
windows, the refusals message by message at config.py and at s3enc_create_byol_s, the block's layout against the header, the hub
names and signatures, the checkpoint reader, and the refusal to shard the family."""

import ctypes as C
import inspect
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import byol_s_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FP32_TOL = 1e-4
FIXTURES = ["byol_s_tiny_eq", "byol_s_tiny_pad", "byol_s_tiny_win025", "byol_s_tiny_hop02", "byol_s_tiny_default",
            "byol_s_resnetish34_pseudo", "byol_s_default_pseudo"]


def _rel(a, b):
    return float(np.linalg.norm(np.asarray(a, np.float64) - np.asarray(b, np.float64)) / np.linalg.norm(np.asarray(b, np.float64)))


# ---- the yardstick ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FIXTURES)
def test_the_float64_restatement_reproduces_the_fixture(name, golden_loader):
    meta, cfg, weights, wavs, hs, _ = golden_loader("byol_s/" + name)
    assert cfg.family == "byol_s" and cfg.conv_layers[0] == (2048, meta["window"], meta["step"])
    out = R.forward(cfg, weights, wavs)
    h = hs[0]
    assert out["state"].shape == h.shape == tuple(meta["shape"]) and len(out["starts"]) == meta["windows"]
    rows = [_rel(out["state"][b, s], h[b, s]) for b in range(h.shape[0]) for s in range(h.shape[1])]
    bound = 0.25 * meta["bound"]  # the restatement stands a quarter of the GPU's bound from the reference
    assert meta["bound"] >= FP32_TOL and _rel(out["state"], h) <= bound and max(rows) <= bound, (name, max(rows))
    assert meta["bound"] == FP32_TOL or meta["bound"] == 4.0 * meta["reference_fp32_vs_float64"]
    # the two statistics, pinned from the reference's own run: both are divided by the number of windows
    N = meta["N"]
    assert N == h.shape[0] * h.shape[1]
    lm = out["logmel"].reshape(N, -1)
    assert abs(out["stats"][0] - meta["stats"][0]) <= 1e-5 * abs(meta["stats"][0])
    assert abs(out["stats"][1] - meta["stats"][1]) <= 1e-5 * abs(meta["stats"][1])
    assert abs(lm.mean() / N - meta["stats"][0]) <= 1e-5 * abs(meta["stats"][0])
    assert abs(lm.std(ddof=1) / N - meta["stats"][1]) <= 1e-5 * abs(meta["stats"][1])
    assert [cfg.num_frames(n) for n in meta["lengths"]] == meta["frames"]
    for b, own in enumerate(meta["frames"]):  # rows past an utterance's own windows are the network's response, not zeros
        for s in range(own, meta["windows"]):
            assert np.abs(h[b, s]).max() > 0


def test_the_fixture_set_covers_what_it_should(golden_loader):
    metas = {n: golden_loader("byol_s/" + n)[0] for n in FIXTURES}
    assert len(set(metas["byol_s_tiny_eq"]["lengths"])) == 1 and len(metas["byol_s_tiny_eq"]["lengths"]) == 2
    pad = metas["byol_s_tiny_pad"]
    s = pad["step"]
    assert any(n < s for n in pad["lengths"]) and any(n % s == 0 for n in pad["lengths"]) and any(n % s == 1 and n > s for n in pad["lengths"])
    assert (metas["byol_s_tiny_win025"]["window"], metas["byol_s_tiny_win025"]["step"]) == (4000, 1600)
    assert metas["byol_s_tiny_hop02"]["step"] == 3200
    for full in ("byol_s_resnetish34_pseudo", "byol_s_default_pseudo"):
        assert metas[full]["shape"] == [3, 4, 2048] and (metas[full]["window"], metas[full]["step"]) == (16000, 800)
    assert all("no torchaudio run" in m["reference"] for m in metas.values())
    assert golden_loader("byol_s/byol_s_resnetish34_pseudo")[1].bs_blocks == (3, 4, 6, 3)


# ---- the window geometry ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("window_secs, hop_secs", [(1, 0.05), (0.25, 0.1), (0.5, 0.2), (0.95, 0.033)])
def test_window_geometry_is_frame_audios(window_secs, hop_secs):
    """S and the starts for lengths around every multiple of the step, against utils.py:72-96 as written there"""
    from s3prl_amd.config import byol_s_config

    cfg = byol_s_config("resnetish", (1, 1, 1, 1), window_secs=window_secs, hop_secs=hop_secs)
    _, window, step = cfg.conv_layers[0]
    frame_duration, hop_size = window_secs * 1000, hop_secs * 1000  # expert.py:22-23
    frame_size = int((frame_duration / 1000) * 16000)  # serab.py:151-153, utils.py:72
    frame_step = int(hop_size / 1000.0 * 16000)  # utils.py:79
    assert (window, step) == (frame_size, frame_step) and cfg.downsample_rate == int(hop_size / 1000 * 16000)
    for k in range(0, 5):
        for delta in (-1, 0, 1, 2):
            n = k * step + delta
            if n < 1:
                continue
            num_padded_samples = n + frame_size // 2 + (frame_size - frame_size // 2)
            starts, frame_number, frame_start = [], 0, 0
            while True:
                starts.append(frame_start)
                frame_number += 1
                frame_start = int(round(frame_number * frame_step))
                if not frame_start + frame_size <= num_padded_samples:
                    break
            assert cfg.num_frames(n) == len(starts) == n // step + 1, n
            assert R.window_plan(n, window, step) == starts == [i * step for i in range(len(starts))]
            assert cfg.valid_frames(n, n + 3 * step) == len(starts) and cfg.valid_frames(n + 3 * step, n) == len(starts)
    frames = R.frame([np.arange(1, 6, dtype=np.float64)], window, step)
    assert frames.shape == (1, 5 // step + 1, window) and np.array_equal(frames[0, 0, window // 2:window // 2 + 5], np.arange(1, 6))
    assert not frames[0, 0, :window // 2].any()


def test_the_statistics_divide_by_the_number_of_windows():
    rng = np.random.default_rng(5)
    lm = rng.standard_normal((7, 11, 64)) * 3.0 - 4.0
    mean, std = R.batch_stats(lm)
    assert abs(mean - lm.mean() / 7) < 1e-15 and abs(std - lm.std(ddof=1) / 7) < 1e-15
    import torch

    t = torch.from_numpy(lm.astype(np.float32))
    m, s = t.mean(), t.std()  # utils.py:43-48
    m /= len(t)
    s /= len(t)
    assert abs(m.item() - mean) < 1e-6 and abs(s.item() - std) < 1e-6


# ---- hub names --------------------------------------------------------------------------------------------------------------------
def test_hub_names_have_the_reference_signatures():
    import s3prl_amd.hub as amd
    from s3prl_amd.upstream.byol_s.expert import UpstreamExpert

    ref = json.load(open(os.path.join(ROOT, "tests", "golden", "byol_s", "reference_hub_byol_s.json")))
    checked = []
    for name, params in ref["hubconfs"]["byol_s"]:
        if name == "byol_s_cvt":  # the CvT network is not built: the name is not registered
            assert name not in amd.options() and not hasattr(amd, name)
            continue
        assert name in amd.options() and name in amd.options(only_registered_ckpt=True), name
        ours = inspect.signature(getattr(amd, name))
        assert [list(p) for p in params] == [[k, v.kind.name, repr(v.default)] for k, v in ours.parameters.items()], name
        checked.append(name)
    assert sorted(checked) == ["byol_s_default", "byol_s_resnetish34"]
    ours = inspect.signature(UpstreamExpert.__init__).parameters
    assert [[k, v.kind.name, repr(v.default)] for k, v in list(ours.items())[:6]] == [list(p) for p in ref["expert_init"]]


def test_hub_names_are_served_from_the_cache_directory(tmp_path):
    import torch

    import s3prl_amd.hub as amd
    from s3prl_amd import download
    from s3prl_amd.synth import named_config, synth_weights

    base = "https://github.com/GasserElbanna/serab-byols/raw/main/checkpoints/"
    files = {"byol_s_default": "default2048_BYOLAs64x96-2105311814-e100-bs256-lr0003-rs42.pth",
             "byol_s_resnetish34": "resnetish34_BYOLAs64x96-2105271915-e100-bs256-lr0003-rs42.pth"}
    old = download.get_dir()
    download.set_dir(tmp_path)
    try:
        for name, fname in files.items():
            cfg = named_config(name)
            weights = synth_weights(cfg, 3)
            path = download.cache_path(base + fname)
            assert path.name.split(".", 1)[1] == fname
            sd = {k: torch.from_numpy(v) for k, v in weights.items()}
            sd[("features.1" if name == "byol_s_default" else "bn1") + ".num_batches_tracked"] = torch.tensor(100)
            torch.save(sd, str(path))
            expert = getattr(amd, name)()
            assert expert.cfg == cfg and expert.get_downsample_rates("hidden_states") == 800 and expert.output_dim == 2048
            assert expert.num_layers == 1 and expert.hidden_sizes == [2048]
            assert set(expert._weights) == set(weights) and all(np.array_equal(expert._weights[k], weights[k]) for k in weights)
            other = getattr(amd, name)(window_secs=0.5, hop_secs=0.2)
            assert other.get_downsample_rates() == 3200 and other.cfg.conv_layers == [(2048, 8000, 3200)]
            with pytest.raises(RuntimeError, match="inference-only"):
                expert([torch.zeros(16000, requires_grad=True)])
            if not torch.cuda.is_available():
                with pytest.raises(RuntimeError, match="no CPU fallback"):
                    expert([torch.zeros(16000)])
    finally:
        download.set_dir(old)


# ---- the checkpoint reader ----------------------------------------------------------------------------------------------------------
def test_checkpoint_reader_round_trip_and_refusals(tmp_path):
    import torch

    from s3prl_amd.ckpt import load_byol_s_checkpoint, load_checkpoint, save_checkpoint
    from s3prl_amd.synth import named_config, synth_weights

    cfg = named_config("tiny_byol_s_resnetish10")
    weights = synth_weights(cfg, 11)
    bns = ["bn1"] + [f"layer{L}.0.{b}" for L in (1, 2, 3, 4) for b in ("bn1", "bn2")] + [f"layer{L}.0.downsample.1" for L in (2, 3, 4)]
    convs = ["conv1"] + [f"layer{L}.0.{c}" for L in (1, 2, 3, 4) for c in ("conv1", "conv2")] + [f"layer{L}.0.downsample.0" for L in (2, 3, 4)]
    assert set(weights) == {f"{b}.{leaf}" for b in bns for leaf in ("weight", "bias", "running_mean", "running_var")} | \
        {f"{c}.weight" for c in convs}
    assert weights["conv1.weight"].shape == (64, 1, 7, 7) and weights["layer3.0.downsample.0.weight"].shape == (256, 128, 1, 1)
    assert all(weights[f"{b}.running_var"].min() >= 0.5 for b in bns)
    assert all(np.array_equal(synth_weights(cfg, 11)[k], weights[k]) for k in weights)  # seeded
    plain = {k: torch.from_numpy(v) for k, v in weights.items()}
    plain["bn1.num_batches_tracked"] = torch.tensor(100)
    for model_name in (None, "resnetish10"):
        got_cfg, got = load_byol_s_checkpoint(plain, model_name=model_name)
        assert got_cfg == cfg and set(got) == set(weights) and all(np.array_equal(got[k], weights[k]) for k in weights)
    with pytest.raises(ValueError, match=r"resnetish34 has \(3, 4, 6, 3\) blocks, but the checkpoint's layers hold \(1, 1, 1, 1\)"):
        load_byol_s_checkpoint(plain, model_name="resnetish34")
    for name in ("cvt", "clstm"):
        with pytest.raises(ValueError, match=f"byol_s network {name} is not built"):
            load_byol_s_checkpoint(plain, model_name=name)
    missing = dict(plain)
    del missing["layer2.0.downsample.1.running_var"]
    with pytest.raises(ValueError, match="missing parameter layer2.0.downsample.1.running_var"):
        load_byol_s_checkpoint(missing)
    bad = dict(plain)
    bad["layer4.0.conv2.weight"] = torch.zeros(512, 256, 3, 3)
    with pytest.raises(ValueError, match="layer4.0.conv2.weight has shape"):
        load_byol_s_checkpoint(bad)
    bottleneck = dict(plain)
    bottleneck["layer1.0.conv3.weight"] = torch.zeros(256, 64, 1, 1)
    with pytest.raises(ValueError, match="Bottleneck blocks .resnetish50. are not built"):
        load_byol_s_checkpoint(bottleneck)
    # a file, through the family dispatcher; and the default network's names
    path = str(tmp_path / "byol_s.pth")
    save_checkpoint(path, cfg, weights)
    got_cfg, got = load_checkpoint(path, "byol_s")
    assert got_cfg == cfg and all(np.array_equal(got[k], weights[k]) for k in weights)
    got_cfg, _ = load_byol_s_checkpoint(path, window_secs=0.25, hop_secs=0.1)
    assert got_cfg == named_config("tiny_byol_s_resnetish10_win025")
    dcfg = named_config("tiny_byol_s_default")
    dw = synth_weights(dcfg, 12)
    assert set(dw) == {f"features.{k}.{leaf}" for k in (0, 4, 8) for leaf in ("weight", "bias")} | \
        {f"features.{k}.{leaf}" for k in (1, 5, 9) for leaf in ("weight", "bias", "running_mean", "running_var")} | \
        {"fc.0.weight", "fc.0.bias", "fc.3.weight", "fc.3.bias"} and dw["fc.3.weight"].shape == (2048, 2048)
    got_cfg, got = load_byol_s_checkpoint({k: torch.from_numpy(v) for k, v in dw.items()}, "default", window_secs=0.25, hop_secs=0.1)
    assert got_cfg == dcfg and all(np.array_equal(got[k], dw[k]) for k in dw)


# ---- configuration ------------------------------------------------------------------------------------------------------------------
def test_config_round_trip_block_layout_and_refusals(tmp_path):
    from s3prl_amd import _lib
    from s3prl_amd.config import EncoderConfig, byol_s_config
    from s3prl_amd.synth import named_config

    cfg = named_config("byol_s_resnetish34")
    assert cfg.conv_layers == [(2048, 16000, 800)] and cfg.encoder_layers == 0 and cfg.num_hidden_states == 1
    assert cfg.downsample_rate == 800 and cfg.num_frames(160000) == 201 and named_config("byol_s_default").bs_network == "default"
    again = EncoderConfig(**cfg.__dict__)
    again.validate()
    assert again == cfg
    c = _lib.make_byol_s_config(named_config("tiny_byol_s_resnetish10_win025"))
    assert (c.network, list(c.blocks), c.bottleneck, c.window, c.step) == (1, [1, 1, 1, 1], 0, 4000, 1600) and abs(c.bn_eps - 1e-5) < 1e-12
    assert _lib.make_byol_s_config(named_config("byol_s_default")).network == 0
    assert _lib.FAMILY["byol_s"] == 14 and _lib.load().s3enc_version() == 8
    header = open(os.path.join(ROOT, "include", "s3enc.h")).read()
    assert "S3ENC_BYOL_S = 14" in header and "#define S3ENC_VERSION 8" in header
    # the C block as the header lays it out: field names, and every offset and the size from the compiler
    block = header[header.index("typedef struct s3enc_byol_s_config {"):header.index("} s3enc_byol_s_config;")]
    fields = [ln.split(";")[0].split()[-1].split("[")[0] for ln in block.splitlines()[1:] if ";" in ln]
    assert fields == [f[0] for f in _lib.S3ByolSConfig._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "s3enc.h"\nint main(void) {\n'
                   + "".join(f'    printf("%zu\\n", offsetof(s3enc_byol_s_config, {f}));\n' for f in fields)
                   + '    printf("%zu\\n", sizeof(s3enc_byol_s_config));\n    return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [getattr(_lib.S3ByolSConfig, f).offset for f in fields] + [C.sizeof(_lib.S3ByolSConfig)]
    # refused by name at config.py
    for network in ("cvt", "clstm"):
        with pytest.raises(ValueError, match=f"byol_s network {network} is not built"):
            byol_s_config(network)
    with pytest.raises(ValueError, match="unknown byol_s network 'sst'"):
        byol_s_config("sst")
    with pytest.raises(ValueError, match="cannot be reflect-padded"):
        byol_s_config("resnetish", window_secs=0.032)      # 512 samples
    byol_s_config("resnetish", window_secs=0.0325)         # 520 samples: the ResNet takes any window the reflection allows
    with pytest.raises(ValueError, match="too short for the default network: fewer than 8 frames"):
        byol_s_config("default", window_secs=0.069)        # 1104 samples
    byol_s_config("default", window_secs=0.07)             # 1120 samples: 8 frames
    with pytest.raises(ValueError, match="step must be at least one sample"):
        byol_s_config("default", hop_secs=0.0)
    with pytest.raises(ValueError, match="Bottleneck blocks .resnetish50. are not built"):
        byol_s_config("resnetish", block="bottleneck")
    with pytest.raises(ValueError, match="four layers of 1..64 BasicBlocks"):
        byol_s_config("resnetish", blocks=(3, 4, 0, 3))
    with pytest.raises(_lib.S3EncError, match="needs a byol_s configuration"):
        _lib.make_byol_s_config(named_config("tiny_byol_a"))
    from s3prl_amd.encoder import HipEncoder

    for dtype in ("bf16", "fp16", "fp32x3", "fp16x2"):
        with pytest.raises(ValueError, match=f"BYOL-S is built for compute dtype fp32 only; {dtype} is not built"):
            HipEncoder(cfg, {}, dtype=dtype)


def _create(block_edit=None, cfg_edit=None, entry="s3enc_create_byol_s"):
    """s3enc_create_byol_s on a valid tiny configuration with one field changed, no tensors: (return code, message); a configuration
    refusal comes before the device lookup"""
    from s3prl_amd import _lib
    from s3prl_amd.synth import named_config

    lib = _lib.load()
    cfg = named_config("tiny_byol_s_resnetish10")
    ccfg = _lib.make_config(cfg, "fp32")
    blk = _lib.make_byol_s_config(cfg)
    if block_edit:
        block_edit(blk)
    if cfg_edit:
        cfg_edit(ccfg)
    tensors = (_lib.S3Tensor * 1)()
    h = C.c_void_p(0xDEAD)
    rc = getattr(lib, entry)(C.byref(ccfg), C.byref(blk), tensors, 0, 0, C.byref(h))
    return rc, h.value, lib.s3enc_last_error().decode()


@pytest.mark.parametrize("edit, message", [
    (lambda b: setattr(b, "network", 2), "config: byol_s network cvt is not built (default and resnetish are)"),
    (lambda b: setattr(b, "network", 3), "config: byol_s network clstm is not built (default and resnetish are)"),
    (lambda b: setattr(b, "network", 4), "config: unknown byol_s network"),
    (lambda b: setattr(b, "bottleneck", 1), "config: byol_s Bottleneck blocks (resnetish50) are not built: BasicBlock layers only"),
    (lambda b: b.blocks.__setitem__(2, 0), "config: byol_s layer3 needs 1..64 BasicBlocks (got 0)"),
    (lambda b: setattr(b, "window", 512), "config: byol_s window of 512 samples is too short: a window of at most 512 samples cannot be "
                                          "reflect-padded by 512 (n_fft / 2)"),
    (lambda b: (setattr(b, "network", 0), setattr(b, "window", 1119)),
     "config: byol_s window of 1119 samples is too short for the default network: fewer than 8 frames (1120 samples), nothing survives "
     "three 2 x 2 pools"),
    (lambda b: setattr(b, "step", 0), "config: byol_s step must be at least one sample"),
    (lambda b: setattr(b, "bn_eps", 0.0), "config: byol_s bn_eps must be positive"),
    (lambda b: setattr(b, "window", 8000), "config: byol_s carries its window geometry as n_conv = 1, conv_kernel[0] / conv_stride[0] = "
                                           "window / step in samples"),
])
def test_create_refusals_message_by_message(edit, message):
    rc, handle, msg = _create(block_edit=edit)
    assert rc != 0 and handle is None and msg == message


def test_create_refuses_the_other_dtypes_and_the_other_entries():
    for dt, name in ((1, "bf16"), (2, "fp16"), (3, "fp32x3"), (4, "fp16x2")):
        rc, handle, msg = _create(cfg_edit=lambda c, dt=dt: setattr(c, "compute_dtype", dt))
        assert rc != 0 and handle is None
        assert msg == ("config: BYOL-S (FFT log-mel windows + whole-batch statistics + a ResNet of 3 x 3 convolutions) is built for compute "
                       f"dtype fp32 only; {name} is not built")
    rc, handle, msg = _create(cfg_edit=lambda c: setattr(c, "family", 12))
    assert rc != 0 and handle is None and msg == "s3enc_create_byol_s: the byol_s block belongs to family S3ENC_BYOL_S only"
    from s3prl_amd import _lib

    lib = _lib.load()
    ccfg = _lib.S3Config()
    ccfg.family = 14
    h = C.c_void_p(0xDEAD)
    assert lib.s3enc_create(C.byref(ccfg), (_lib.S3Tensor * 1)(), 0, 0, C.byref(h)) != 0 and h.value is None
    assert lib.s3enc_last_error().decode() == "s3enc_create: the BYOL-S family needs its window / network block: use s3enc_create_byol_s"
    assert lib.s3enc_create_byol_s(C.byref(ccfg), None, (_lib.S3Tensor * 1)(), 0, 0, C.byref(h)) != 0
    assert lib.s3enc_last_error().decode() == "s3enc_create_byol_s: null argument"


# ---- sharding -----------------------------------------------------------------------------------------------------------------------
def test_the_family_is_not_sharded():
    from s3prl_amd.parallel import DataParallelUpstream, featurized_data_parallel
    from s3prl_amd.synth import named_config, synth_weights
    from s3prl_amd.upstream.byol_s.expert import UpstreamExpert

    cfg = named_config("tiny_byol_s_resnetish10")
    expert = UpstreamExpert.from_weights(cfg, synth_weights(cfg, 1))
    with pytest.raises(ValueError, match="byol_s cannot be sharded over ranks: its log-mel statistics belong to the whole batch"):
        DataParallelUpstream(expert)
    with pytest.raises(ValueError, match="byol_s cannot be sharded over ranks"):
        featurized_data_parallel(expert, [1.0], [])
