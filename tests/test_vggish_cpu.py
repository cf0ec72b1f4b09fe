"""VGGish without a GPU: the float64 restatement (tests/vggish_ref.py) against every reference-generated fixture, the frame
arithmetic, the configuration and the checkpoint reader, the C configuration block against the header, the hub name and its cache
files, and the refusals of the library as error codes with a message."""

import ctypes as C
import inspect
import json
import os
import re

import numpy as np
import pytest

import vggish_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FP32_TOL = 1e-4
HALF_BAND = 0.02
RAW = ["vggish/vggish_raw_pad"]
QUANT = ["vggish/" + n for n in ["vggish_pad", "vggish_one", "vggish_10s", "vggish_eq"]]


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def _live(a, counts):
    return np.concatenate([a[b, :n] for b, n in enumerate(counts)])


@pytest.fixture(scope="module")
def w64(golden_loader):
    """the fixtures' full-size weights in float64, converted once per weight seed"""
    cache = {}

    def get(name):
        from s3prl_amd.synth import named_config, synth_weights

        meta, _, weights, _, _, _ = golden_loader(name)
        if meta["weight_seed"] not in cache:
            cache.clear()
            if "pca_means" not in weights:  # the raw form's weights are the quantised form's without the post-processor
                weights = synth_weights(named_config("vggish"), meta["weight_seed"])
            cache[meta["weight_seed"]] = {k: v.astype(np.float64) for k, v in weights.items()}
        return cache[meta["weight_seed"]]

    return get


# ---- the restatement against the reference -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", RAW)
def test_float64_restatement_matches_the_reference_raw(name, golden_loader, w64):
    meta, cfg, weights, wavs, hs, norms = golden_loader(name)
    assert not cfg.vg_postprocess and meta["n_states"] == 1 and not any(k.startswith("pca_") for k in weights)
    out = R.forward(cfg, w64(name), wavs)
    assert out["counts"] == meta["frames"] == [cfg.num_frames(n) for n in meta["lengths"]]
    assert list(out["state"].shape) == meta["shape"] == [len(wavs), max(meta["frames"]), 128]
    errs = [_rel(out["state"], hs[0])] + [_rel(out["state"][b, :n], hs[0][b, :n]) for b, n in enumerate(meta["frames"])]
    assert max(errs) < FP32_TOL, errs
    assert abs(np.linalg.norm(out["state"]) - norms[0]) / norms[0] < FP32_TOL
    for b, n in enumerate(meta["frames"]):
        assert not hs[0][b, n:].any() and not out["state"][b, n:].any()  # pad_sequence: exact zeros


@pytest.mark.parametrize("name", QUANT)
def test_float64_restatement_matches_the_reference_quantised(name, golden_loader, w64):
    """the reference's fp32 values q against the restatement's float64 pre-rounding values: |q - pre64| <= 0.5 + HALF_BAND on every
    live element, equal after rounding on at least 95 % (generator rule (d)); the stored raw embeddings to FP32_TOL"""
    meta, cfg, weights, wavs, hs, _ = golden_loader(name)
    assert cfg.vg_postprocess and meta["n_states"] == 1
    out = R.forward(cfg, w64(name), wavs)
    counts = meta["frames"]
    assert out["counts"] == counts and list(hs[0].shape) == meta["shape"]
    q, pre = _live(hs[0], counts).astype(np.float64), _live(out["pre"], counts)
    assert np.array_equal(q, np.rint(q)) and q.min() >= 0 and q.max() <= 255
    assert np.abs(q - pre).max() <= 0.5 + HALF_BAND
    assert (q == _live(out["state"], counts)).mean() >= 0.95
    z = np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"))
    assert _rel(out["emb"], z["emb"]) < FP32_TOL
    for b, n in enumerate(counts):
        assert not hs[0][b, n:].any()  # exact zeros also in the quantised form ...
    assert (q == 0).mean() < 0.1      # ... where a live row is rarely 0
    assert meta["near_half"] <= 0.05 and meta["at_ends"] <= 0.10 and 0.2 <= meta["zeros"] <= 0.7
    assert meta["ref_fp32_err"] <= 0.25 * FP32_TOL and meta["fp32_proxy_err"] <= 0.25 * FP32_TOL


def test_fixture_table(golden_loader):
    want = {"vggish_pad": ([48123, 15600, 40000], [3, 1, 2], True), "vggish_raw_pad": ([48123, 15600, 40000], [3, 1, 2], False),
            "vggish_eq": ([31000, 31000], [2, 2], True), "vggish_one": ([15600], [1], True), "vggish_10s": ([160000, 100000], [10, 6], True)}
    for name, (lengths, counts, post) in want.items():
        path = os.path.join(ROOT, "tests", "golden", "vggish", name + ".npz")
        assert os.path.getsize(path) < 256 * 1024
        meta = golden_loader("vggish/" + name)[0]
        assert (meta["lengths"], meta["frames"], meta["postprocess"]) == (lengths, counts, post), name
    eq = golden_loader("vggish/vggish_eq")[0]
    assert (eq["dc"], eq["scale"]) == (0.1, 0.5)


def test_tiny_fp32_variant_stays_near_float64():
    from s3prl_amd.synth import named_config, synth_wavs, synth_weights

    for name in ("tiny_vggish", "tiny_vggish_odd"):
        cfg = named_config(name)
        weights = synth_weights(cfg, 3)
        wavs = synth_wavs([cfg.vg_min_samples * 3 + 100, cfg.vg_min_samples], 4)
        a, b = R.forward(cfg, weights, wavs), R.forward(cfg, weights, wavs, np.float32)
        assert a["counts"] == b["counts"] == [3, 1]
        assert _rel(b["emb"], a["emb"]) < 0.25 * FP32_TOL
        assert np.abs(b["pre"] - a["pre"]).max() < HALF_BAND


def test_conv_and_pool_restatement_match_torch_in_float64():
    import torch

    rng = np.random.default_rng(0)
    x, w, b = rng.standard_normal((2, 6, 4, 5)), rng.standard_normal((7, 5, 3, 3)), rng.standard_normal(7)
    want = torch.nn.functional.conv2d(torch.from_numpy(x).permute(0, 3, 1, 2), torch.from_numpy(w), torch.from_numpy(b), padding=1)
    assert np.abs(R.conv3x3(x, w, b) - want.permute(0, 2, 3, 1).numpy()).max() < 1e-12
    pooled = torch.nn.functional.max_pool2d(want, 2, 2).permute(0, 2, 3, 1).numpy()
    assert np.array_equal(R.maxpool2(want.permute(0, 2, 3, 1).numpy()), pooled)


# ---- arithmetic, configuration, checkpoints --------------------------------------------------------------------------------------
@pytest.mark.parametrize("n, E", [(399, 0), (400, 0), (15599, 0), (15600, 1), (30959, 1), (30960, 2), (160000, 10), (100000, 6)])
def test_frame_arithmetic(n, E):
    from s3prl_amd.synth import named_config

    cfg = named_config("vggish")
    assert cfg.num_frames(n) == E == R.num_examples(cfg, n) == cfg.num_output_frames(n)
    assert cfg.valid_frames(n, max(n, 48123)) == E
    assert cfg.vg_min_samples == 15600 and cfg.downsample_rate == 16000 and cfg.num_hidden_states == 1


def test_named_configs_and_shapes():
    from s3prl_amd.config import vggish_config
    from s3prl_amd.synth import named_config, param_shapes

    cfg = named_config("vggish")
    assert cfg.vg_layers == [(64, True), (128, True), (256, False), (256, True), (512, False), (512, True)]
    assert [cfg.vg_seq_index(i) for i in range(6)] == [0, 3, 6, 8, 11, 13]
    s = param_shapes(cfg)
    assert s["features.0.weight"] == (64, 1, 3, 3) and s["features.13.weight"] == (512, 512, 3, 3)
    assert s["embeddings.0.weight"] == (4096, 12288) and s["embeddings.4.weight"] == (128, 4096)
    assert s["pca_eigen_vectors"] == (128, 128) and s["pca_means"] == (128,)
    assert sum(int(np.prod(v)) for v in s.values()) == 72141184 + 128 * 128 + 128
    assert "pca_means" not in param_shapes(named_config("vggish_raw"))
    tiny, odd = named_config("tiny_vggish"), named_config("tiny_vggish_odd")
    assert (tiny.vg_example_frames, tiny.vg_num_mel_bins, tiny.vg_fc, tiny.vg_min_samples) == (16, 16, (128, 128, 32), 2800)
    assert param_shapes(tiny)["embeddings.0.weight"] == (128, 64)
    assert odd.vg_layers == [(16, True), (48, True), (48, True)] and param_shapes(odd)["embeddings.0.weight"] == (128, 3 * 1 * 48)
    assert vggish_config(layers=[(64, True), (128, True), (256, False), (256, True), (512, False), (512, True)]) == cfg


REFUSALS = [
    (dict(layers=[24, "M"], example_frames=16, num_mel_bins=16), "multiple of 16"),
    (dict(layers=[16, "M", 16, "M"], example_frames=18, num_mel_bins=16), "example_frames 18 is not divisible by 2\\^pools = 4"),
    (dict(layers=[16, "M", 16, "M"], example_frames=16, num_mel_bins=10), "num_mel_bins 10 is not divisible by 2\\^pools = 4"),
    (dict(example_hop=48), "example_hop 48 is not built"),
    (dict(window=402), "multiple of 4 samples"),
    (dict(shift=162), "multiple of 4 samples"),
    (dict(fc=(4096, 4095, 128)), "multiples of 4"),
    (dict(layers=["M", 16]), "must follow a conv layer"),
    (dict(layers=[16] * 9), "1..8 conv layers"),
    (dict(mel_max_hz=9000.0), "mel edges"),
]


@pytest.mark.parametrize("kw, match", REFUSALS)
def test_config_refusals(kw, match):
    from s3prl_amd.config import vggish_config

    with pytest.raises(ValueError, match=match):
        vggish_config(**kw)


def test_checkpoint_round_trip_and_reader(tmp_path):
    """save_checkpoint -> the dict file -> load_checkpoint: a tiny shape (through this package's `config` entry), a dict in
    memory with the reference's tensor names, pca_means as (D,) or (D, 1), and the refusals by name"""
    import torch

    from s3prl_amd.ckpt import load_checkpoint, load_vggish_checkpoint, save_checkpoint
    from s3prl_amd.synth import named_config, synth_weights

    for name in ("tiny_vggish", "tiny_vggish_odd"):
        cfg = named_config(name)
        weights = synth_weights(cfg, 5)
        path = str(tmp_path / f"{name}.pt")
        save_checkpoint(path, cfg, weights)
        state = torch.load(path, map_location="cpu", weights_only=False)
        assert set(state) == {"vggish", "pca", "config"} and set(state["pca"]) == {"pca_eigen_vectors", "pca_means"}
        assert not any(k.startswith("pca_") for k in state["vggish"])
        back_cfg, back = load_checkpoint(path, "vggish")
        assert back_cfg == cfg and set(back) == set(weights) and all(np.array_equal(back[k], weights[k]) for k in weights)
        raw_cfg, raw = load_vggish_checkpoint(path, postprocess=False)
        assert raw_cfg == named_config(name + "_raw") and "pca_means" not in raw
        state["pca"]["pca_means"] = state["pca"]["pca_means"].reshape(-1, 1).numpy()  # the released file: numpy, a column
        cfg2, w2 = load_vggish_checkpoint(state)
        assert cfg2 == cfg and w2["pca_means"].shape == (32,) and np.array_equal(w2["pca_means"], weights["pca_means"])
        bad = dict(state, pca=dict(state["pca"], pca_means=np.zeros((2, 16), np.float32)))
        with pytest.raises(ValueError, match="pca_means has shape"):
            load_vggish_checkpoint(bad)
        with pytest.raises(ValueError, match="needs the key 'pca'"):
            load_vggish_checkpoint({"vggish": state["vggish"], "config": state["config"]})
        with pytest.raises(ValueError, match="'vggish' is missing"):
            load_vggish_checkpoint({"pca": state["pca"]})
        sd = dict(state["vggish"])
        del sd["embeddings.2.bias"]
        with pytest.raises(ValueError, match="missing parameter embeddings.2.bias"):
            load_vggish_checkpoint(dict(state, vggish=sd))


# ---- the C block and the library's refusals ------------------------------------------------------------------------------------
def test_vggish_block_follows_the_header(tmp_path):
    import subprocess

    from s3prl_amd import _lib

    header = open(os.path.join(ROOT, "include", "s3enc.h")).read()
    body = header[header.index("typedef struct s3enc_vggish_config {"):header.index("} s3enc_vggish_config;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = re.findall(r"(?:int32_t|float)\s+([a-z0-9_]+)(?:\[[^\]]*\])?;", body)
    assert names == [n for n, _ in _lib.S3VggishConfig._fields_] and names[0] == "num_mel_bins" and names[-1] == "quant_max"
    assert _lib.FAMILY["vggish"] == 11 and "S3ENC_VGGISH = 11" in header and "#define S3ENC_VERSION 8" in header
    for sym in ("s3enc_create_vggish", "s3enc_op_conv2d3x3"):
        assert re.search(r"\bint " + sym + r"\(", header), sym
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "s3enc.h"\n'
                   'int main(void){printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(s3enc_vggish_config), offsetof(s3enc_vggish_config, channels), '
                   'offsetof(s3enc_vggish_config, pool_after), offsetof(s3enc_vggish_config, fc), offsetof(s3enc_vggish_config, quant_max), '
                   'sizeof(s3enc_npc_config));return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    W = _lib.S3VggishConfig
    assert got == [C.sizeof(W), W.channels.offset, W.pool_after.offset, W.fc.offset, W.quant_max.offset, C.sizeof(_lib.S3NpcConfig)]


def _create_error(ccfg, vg):
    from s3prl_amd import _lib

    lib = _lib.load()
    h = C.c_void_p()
    tensors = (_lib.S3Tensor * 1)()
    assert lib.s3enc_create_vggish(C.byref(ccfg), C.byref(vg) if vg is not None else None, tensors, 0, 0, C.byref(h)) != 0
    assert not h.value
    return lib.s3enc_last_error().decode()


def _set(vg, field, value):
    if isinstance(field, tuple):
        getattr(vg, field[0])[field[1]] = value
    else:
        setattr(vg, field, value)


@pytest.mark.parametrize("field, value, match", [
    (("channels", 1), 24, "channels of layer 1 must be a multiple of 16"),
    ("example_frames", 20, "example_frames 20 is not divisible by 2^pools = 16"),
    ("num_mel_bins", 24, "num_mel_bins 24 is not divisible by 2^pools = 16"),
    ("example_hop", 8, "example_hop 8 is not built"),
    ("n_layers", 0, "n_layers must be 1..8"),
    ("n_layers", 9, "n_layers must be 1..8"),
    ("window", 402, "multiple of 4 samples"),
    ("shift", 80, "frame geometry"),
    ("n_fft", 1024, "n_fft must be the power of two"),
    (("fc", 1), 130, "Linear widths must be multiples of 4"),
    (("fc", 2), 64, "last Linear's width"),
    ("quant_max", -3.0, "quant_min < quant_max"),
    ("log_offset", 0.0, "log_offset must be positive"),
])
def test_the_library_refuses_by_name(field, value, match):
    """s3enc_create_vggish checks the configuration before it looks for a device: the refusals are the same without a GPU."""
    from s3prl_amd import _lib
    from s3prl_amd.synth import named_config

    cfg = named_config("tiny_vggish")
    ccfg, vg = _lib.make_config(cfg, "fp32"), _lib.make_vggish_config(cfg)
    assert ccfg.family == 11 and ccfg.n_conv == 1 and (ccfg.conv_kernel[0], ccfg.conv_stride[0]) == (400, 160)
    assert ccfg.encoder_layers == 0 and ccfg.embed_dim == ccfg.conv_dim == 32
    assert (vg.num_mel_bins, vg.window, vg.shift, vg.n_fft, vg.example_frames, vg.example_hop, vg.n_layers, list(vg.channels)[:6],
            list(vg.pool_after)[:6], list(vg.fc), vg.postprocess, vg.quant_min, vg.quant_max) == (
        16, 400, 160, 512, 16, 16, 6, [16, 32, 32, 32, 64, 64], [1, 1, 0, 1, 0, 1], [128, 128, 32], 1, -2.0, 2.0)
    assert abs(vg.mel_min_hz - 125.0) < 1e-6 and abs(vg.mel_max_hz - 7500.0) < 1e-3 and abs(vg.log_offset - 0.01) < 1e-8
    _set(vg, field, value)
    assert match in _create_error(ccfg, vg)


@pytest.mark.parametrize("dtype", ["bf16", "fp16", "fp16x2", "fp32x3"])
def test_non_fp32_modes_are_refused_with_the_mode_named(dtype):
    from s3prl_amd import _lib
    from s3prl_amd.encoder import HipEncoder
    from s3prl_amd.synth import named_config, synth_weights

    cfg = named_config("tiny_vggish")
    err = _create_error(_lib.make_config(cfg, dtype), _lib.make_vggish_config(cfg))
    assert "fp32 only" in err and dtype in err
    with pytest.raises(ValueError, match="fp32 only"):
        HipEncoder(cfg, synth_weights(cfg, 0), dtype=dtype)


def test_the_vggish_block_is_required_for_the_family_and_refused_elsewhere():
    from s3prl_amd import _lib
    from s3prl_amd.synth import named_config

    cfg = named_config("tiny_vggish")
    lib = _lib.load()
    h = C.c_void_p()
    tensors = (_lib.S3Tensor * 1)()
    ccfg = _lib.make_config(cfg, "fp32")
    assert lib.s3enc_create(C.byref(ccfg), tensors, 0, 0, C.byref(h)) != 0 and b"s3enc_create_vggish" in lib.s3enc_last_error()
    npc = _lib.make_npc_config(named_config("tiny_npc"))
    assert lib.s3enc_create_npc(C.byref(ccfg), C.byref(npc), tensors, 0, 0, C.byref(h)) != 0 and b"s3enc_create_vggish" in lib.s3enc_last_error()
    assert "null argument" in _create_error(ccfg, None)
    assert "S3ENC_VGGISH only" in _create_error(_lib.make_config(named_config("tiny_npc"), "fp32"), _lib.make_vggish_config(cfg))
    assert lib.s3enc_version() == 8  # every addition is a new symbol


def test_op_entry_validates_its_arguments():
    """s3enc_op_conv2d3x3 refuses bad arguments with a message before touching a device."""
    from s3prl_amd import _lib

    lib = _lib.load()
    one = C.c_void_p(256)

    def call(x=one, w=one, bias=one, B=2, H=4, W=4, Cc=16, N=64, act=1, pool=1, dst=one, dst_pad=1, ldo=64):
        rc = lib.s3enc_op_conv2d3x3(x, w, bias, B, H, W, Cc, N, act, pool, dst, dst_pad, ldo, None)
        return rc, lib.s3enc_last_error()

    for kw, msg in [(dict(x=None), b"null argument"), (dict(w=None), b"null argument"), (dict(dst=None), b"null argument"),
                    (dict(B=0), b"bad shape"), (dict(H=0), b"bad shape"), (dict(Cc=24), b"multiple of 16"), (dict(Cc=8), b"multiple of 16"),
                    (dict(N=66, ldo=68), b"Cout must be a multiple of 4"), (dict(H=5), b"even under pool"), (dict(W=6, H=3), b"even under pool"),
                    (dict(act=2), b"act must be"), (dict(pool=2), b"pool must be"), (dict(ldo=60), b"pixel pitch is smaller than Cout"),
                    (dict(ldo=66), b"multiples of 4"), (dict(dst_pad=-1), b"border width"), (dict(x=C.c_void_p(260)), b"16-byte aligned"),
                    (dict(dst=C.c_void_p(264)), b"16-byte aligned"), (dict(bias=C.c_void_p(260)), b"16-byte aligned"),
                    (dict(Cc=1, x=C.c_void_p(258)), b"4-byte aligned")]:
        rc, err = call(**kw)
        assert rc != 0 and msg in err, (kw, err)


# ---- the hub name ---------------------------------------------------------------------------------------------------------------
def test_hub_names_have_the_reference_signatures():
    import s3prl_amd.hub as amd
    from s3prl_amd.upstream.vggish.expert import UpstreamExpert

    ref = json.load(open(os.path.join(ROOT, "tests", "golden", "vggish", "reference_hub_vggish.json")))
    everything = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_hub.json")))["options"]
    assert ref["downsample_rate"] == 16000
    checked = []
    for name, params in ref["hubconfs"]["vggish"]:
        assert name in everything and name in amd.options(), name
        ours = inspect.signature(getattr(amd, name))
        assert [list(p) for p in params] == [[k, v.kind.name, repr(v.default)] for k, v in ours.parameters.items()], name
        checked.append(name)
    assert checked == ["vggish"] and "vggish" in amd.options(only_registered_ckpt=True)
    # the constructor contract: ckpt, then the model's pretrained / postprocess / progress with the reference's defaults
    ours = inspect.signature(UpstreamExpert.__init__).parameters
    assert [p[0] for p in ref["expert_init"][:2]] == ["self", "ckpt"] and list(ours)[:2] == ["self", "ckpt"]
    for k, _, default in ref["model_init"]:
        if k in ("pretrained", "postprocess", "progress"):
            assert repr(ours[k].default) == default, k


def test_hub_vggish_is_served_from_the_cache_directory(tmp_path):
    """the two URLs resolve to the reference's cache file names; two synthetic files there (the released layout: the PCA
    parameters as numpy arrays, the means as (128,)) make hub.vggish() without touching a network"""
    import torch

    import s3prl_amd.hub as amd
    from s3prl_amd import download
    from s3prl_amd.synth import named_config, synth_weights

    urls = ["https://github.com/harritaylor/torchvggish/releases/download/v0.1/vggish-10086976.pth",
            "https://github.com/harritaylor/torchvggish/releases/download/v0.1/vggish_pca_params-970ea276.pth"]
    cfg = named_config("vggish")
    weights = synth_weights(cfg, 7)
    old = download.get_dir()
    download.set_dir(tmp_path)
    try:
        paths = [download.cache_path(u) for u in urls]
        assert [p.name.split(".", 1)[1] for p in paths] == ["vggish-10086976.pth", "vggish_pca_params-970ea276.pth"]
        assert all(len(p.name.split(".", 1)[0]) == 64 for p in paths)
        torch.save({k: torch.from_numpy(v) for k, v in weights.items() if not k.startswith("pca_")}, str(paths[0]))
        torch.save({"pca_eigen_vectors": weights["pca_eigen_vectors"], "pca_means": weights["pca_means"]}, str(paths[1]))
        expert = amd.vggish()
        assert expert.cfg == cfg and expert.get_downsample_rates("hidden_states") == 16000
        assert expert.num_layers == 1 and expert.hidden_sizes == [128]
        assert set(expert._weights) == set(weights) and all(np.array_equal(expert._weights[k], weights[k]) for k in weights)
        raw = amd.vggish(postprocess=False)
        assert raw.cfg == named_config("vggish_raw") and "pca_means" not in raw._weights
        with pytest.raises(ValueError, match="pretrained=False"):
            amd.vggish(pretrained=False)
        wav = torch.zeros(16000, requires_grad=True)
        with pytest.raises(RuntimeError, match="inference-only"):
            expert([wav])
        if not torch.cuda.is_available():
            with pytest.raises(RuntimeError, match="no CPU fallback"):
                expert([torch.zeros(16000)])
    finally:
        download.set_dir(old)
