"""APC / VQ-APC without a GPU: the float64 restatement of tests/apc_ref.py against every reference-generated fixture and against
the pinned fbank oracle, the frame arithmetic, checkpoint reading, the refusals by name (Python and s3enc_create_apc), the
configuration block against the header, the op entries' argument checks and the hub names."""

import ctypes as C
import inspect
import json
import os
import re

import numpy as np
import pytest

from oracle import encoder_oracle as O
from oracle import fbank_oracle as FO

import apc_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NAMES = ["apc_tiny_pad", "apc_tiny_eq", "apc_tiny_nores", "apc_tiny_t1", "apc_tiny_l4", "vq_apc_tiny_pad", "apc_360hr_pseudo"]
FIXTURES = ["apc/" + n for n in NAMES]
REF_PIN = 1e-6  # the project's restatement bound: a float64 restatement against the reference's fp32 outputs


@pytest.fixture(scope="module")
def restated(golden_loader):
    """apc_ref's float64 forward of every fixture, computed once"""
    cache = {}

    def get(name):
        if name not in cache:
            meta, cfg, weights, wavs, hs, norms = golden_loader(name)
            feats, lens = R.features(cfg, wavs)
            # the generator fed the reference these features ROUNDED TO fp32
            cache[name] = (R.model(cfg, weights, feats.astype(np.float32), lens), lens)
        return cache[name]

    return get


@pytest.mark.parametrize("name", FIXTURES)
def test_float64_restatement_matches_the_reference(name, golden_loader, restated):
    meta, cfg, weights, wavs, hs, norms = golden_loader(name)
    out, lens = restated(name)
    assert len(hs) == cfg.num_hidden_states == 3 and meta["n_states"] == 3
    assert lens == meta["frames"] == [cfg.num_frames(n) for n in meta["lengths"]]
    ts, cs = meta["t_stride"], meta["c_stride"]
    assert meta["shape"] == [len(wavs), cfg.num_frames(max(meta["lengths"])), cfg.conv_dim]
    for l, h in enumerate(out["hidden_states"]):
        assert list(h.shape) == meta["shape"]
        assert O.rel_err(h[:, ::ts, ::cs], hs[l]) <= REF_PIN, (name, l)
        assert abs(np.linalg.norm(h) - norms[l]) / norms[l] <= REF_PIN
        for b, n in enumerate(lens):  # pad_packed_sequence: exactly zero behind every utterance's frames, on both sides
            assert not h[b, n:].any() and not hs[l][b, -(-n // ts):].any()
            assert O.rel_err(h[b, :n:ts, ::cs], hs[l][b, :-(-n // ts)]) <= REF_PIN, (name, l, b)
    assert len(meta["gate_std"]) == cfg.apc_layers and min(meta["gate_std"]) >= 1.0
    assert np.allclose(out["gate_std"], meta["gate_std"], rtol=1e-9)
    assert max(meta["ref_fp32_err"]) <= 8e-7 and max(meta["fp32_proxy_err"]) <= 0.25e-4


def test_fixture_table():
    """The fixtures the issue names: configurations, lengths, frames."""
    from conftest import golden_meta

    from s3prl_amd.synth import named_config

    want = {"apc_tiny_pad": ("tiny_apc", [4000, 2345, 3111], 23), "apc_tiny_eq": ("tiny_apc", [3200, 3200], 18),
            "apc_tiny_nores": ("tiny_apc_nores", [4000, 2345, 3111], 23), "apc_tiny_t1": ("tiny_apc_nocmvn", [400, 2000], 11),
            "apc_tiny_l4": ("tiny_apc_l4", [4000, 2345, 3111], 23), "vq_apc_tiny_pad": ("tiny_vq_apc", [4000, 2345, 3111], 23),
            "apc_360hr_pseudo": ("apc_360hr", [16000, 12345], 98)}
    assert sorted(want) == sorted(NAMES)
    for name, (cfg, lengths, T) in want.items():
        m = golden_meta("apc/" + name)
        assert (m["config"], m["lengths"], m["shape"][1]) == (cfg, lengths, T), name
        assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "apc", name + ".npz")) < 256 * 1024
    assert golden_meta("apc/apc_tiny_t1")["frames"] == [1, 11]  # one utterance of exactly one frame
    assert len(set(golden_meta("apc/apc_tiny_pad")["frames"])) == 3 and len(set(golden_meta("apc/apc_tiny_eq")["frames"])) == 1
    c = named_config("apc_360hr")
    assert (c.conv_dim, c.apc_layers, c.apc_residual, c.apc_feat_dim, c.apc_window, c.apc_cmvn) == (512, 3, True, 80, "hamming", True)
    assert not named_config("tiny_apc_nores").apc_residual and named_config("tiny_apc_l4").apc_layers == 4
    assert named_config("tiny_vq_apc").apc_vq is not None and named_config("tiny_vq_apc").conv_dim == 128
    assert named_config("tiny_apc").conv_dim == 64


# ---- the front end ---------------------------------------------------------------------------------------------------------
def test_hamming_window_is_numpys():
    for n in (400, 320, 16, 5):
        assert np.abs(R.hamming_window(n) - np.hamming(n)).max() <= 1e-15
    assert np.array_equal(R.window("povey", 400), FO.povey_window(400))


@pytest.mark.parametrize("n", [400, 2000, 3111])
def test_front_end_with_the_povey_window_is_the_pinned_oracle(n):
    """The restatement differs from oracle.fbank_oracle in the window only: with povey, no deltas and 80 bins it IS that oracle."""
    wav = np.random.default_rng(n).standard_normal(n)
    assert np.abs(R.kaldi_fbank(wav, window_type="povey") - FO.kaldi_fbank(wav)).max() <= 1e-12
    if n > 400:
        got = R.cmvn(R.kaldi_fbank(wav, window_type="povey"))
        assert np.abs(got - FO.extract(wav, order=0)).max() <= 1e-12
    ham = R.kaldi_fbank(wav)
    assert ham.shape == (FO.num_frames(n), 80) and np.abs(ham - FO.kaldi_fbank(wav)).max() > 1e-3  # the window matters


def test_front_end_known_answers():
    from s3prl_amd.synth import named_config

    cfg = named_config("tiny_apc")
    x, lens = R.features(cfg, [np.random.default_rng(1).standard_normal(n) for n in (4000, 2345)])
    assert x.shape == (2, 23, 80) and lens == [23, 13] and not x[1, 13:].any()
    for b, n in enumerate(lens):  # CMVN over time: zero mean, unit unbiased std per bin
        assert np.abs(x[b, :n].mean(0)).max() < 1e-12 and np.abs(x[b, :n].std(0, ddof=1) - 1).max() < 1e-9
    one = R.frontend(cfg, np.random.default_rng(2).standard_normal(400))
    assert one.shape == (1, 80) and np.isnan(one).all()  # one frame has no std: nan, like torch
    raw = R.frontend(named_config("tiny_apc_nocmvn"), np.random.default_rng(2).standard_normal(400))
    assert raw.shape == (1, 80) and np.isfinite(raw).all()


def test_packed_gru_matches_torch_in_float64():
    import torch
    from torch.nn.utils.rnn import pack_padded_sequence, pad_packed_sequence

    B, T, I, H = 3, 11, 20, 24
    lens = [11, 1, 6]
    torch.manual_seed(3)
    net = torch.nn.GRU(I, H, batch_first=True).double()
    with torch.no_grad():
        for p in net.parameters():
            p.mul_(6.0)
        x = torch.randn(B, T, I, dtype=torch.float64)
        packed = pack_padded_sequence(x, torch.LongTensor(lens), batch_first=True, enforce_sorted=False)
        want = pad_packed_sequence(net(packed)[0], batch_first=True, total_length=T)[0].numpy()
    g = lambda n: getattr(net, f"{n}_l0").detach().numpy()  # noqa: E731
    got, gates = R.gru_layer_packed(x.numpy(), lens, g("weight_ih"), g("weight_hh"), g("bias_ih"), g("bias_hh"))
    assert gates.std() > 1.0 and np.abs(got - want).max() <= 1e-12
    assert not got[1, 1:].any() and not got[2, 6:].any()


@pytest.mark.parametrize("n, T", [(160000, 998), (16000, 98), (4000, 23), (400, 1), (399, 0)])
def test_frame_arithmetic(n, T):
    from s3prl_amd.synth import named_config

    for name in ("tiny_apc", "tiny_apc_l4", "apc_360hr"):
        cfg = named_config(name)
        assert cfg.num_frames(n) == T == FO.num_frames(n) and cfg.num_output_frames(n) == T
        assert cfg.valid_frames(n, 160000) == T and cfg.downsample_rate == 160
        assert cfg.num_hidden_states == 3  # three hooks, also with four layers
    assert named_config("tiny_apc").valid_frames(2345, 4000) == 13


# ---- checkpoints -----------------------------------------------------------------------------------------------------------
def _config(audio=None, paras=None):
    a = dict(feat_type="fbank", feat_dim=80, frame_length=25, frame_shift=10, decode_wav=False, cmvn=True)
    a.update(audio or {})
    p = dict(hidden_size=64, num_layers=3, dropout=0.1, residual=True)
    p.update(paras or {})
    return {"data": {"audio": {k: v for k, v in a.items() if v is not None}}, "model": {"paras": p}}


def _save(tmp_path, config, weights_of="tiny_apc", drop=None, extra=None):
    import torch

    from s3prl_amd.synth import named_config, synth_weights

    sd = {k: torch.from_numpy(v) for k, v in synth_weights(named_config(weights_of), 3).items() if k != drop}
    sd.update(extra or {})
    path = str(tmp_path / "c.pt")
    torch.save({"config": config, "model": sd}, path)
    return path


def test_checkpoint_round_trip(tmp_path):
    import torch

    from s3prl_amd.ckpt import load_apc_checkpoint, load_checkpoint, save_checkpoint
    from s3prl_amd.config import config_from_apc
    from s3prl_amd.synth import named_config, synth_weights

    d = config_from_apc(_config(audio=dict(frame_length=None, frame_shift=None, cmvn=None, decode_wav=None)))  # kaldi's defaults
    assert (d.apc_frame_length, d.apc_frame_shift, d.apc_cmvn, d.conv_layers) == (25.0, 10.0, True, [(64, 400, 160)])
    over = config_from_apc(_config(audio=dict(frame_length=20, cmvn=False), paras=dict(hidden_size=128, num_layers=4, residual=False)))
    assert (over.conv_dim, over.apc_layers, over.apc_residual, over.apc_cmvn, over.conv_layers) == (128, 4, False, False, [(128, 320, 160)])
    for name in ("tiny_apc", "tiny_apc_nores", "tiny_apc_nocmvn", "tiny_apc_l4", "tiny_vq_apc", "apc_360hr"):
        cfg = named_config(name)
        weights = synth_weights(cfg, 5)
        assert len(weights) == 4 * cfg.apc_layers
        path = str(tmp_path / "c.pt")
        save_checkpoint(path, cfg, weights)
        state = torch.load(path, map_location="cpu", weights_only=False)
        assert set(state) == {"config", "model"} and set(state["config"]) == {"data", "model"}  # apc/expert.py:22-27
        # the tensors that feed only the discarded prediction are accepted and left in the file
        state["model"]["postnet.weight"] = torch.zeros(80, cfg.conv_dim)
        state["model"]["postnet.bias"] = torch.zeros(80)
        state["model"]["vq_layers.0.vq_logits.weight"] = torch.zeros(32, cfg.conv_dim)
        torch.save(state, path)
        cfg2, back = load_apc_checkpoint(path)
        assert cfg2 == cfg and load_checkpoint(path, "apc")[0] == cfg
        assert set(back) == set(weights) and all(np.array_equal(back[k], weights[k]) for k in weights)


@pytest.mark.parametrize("drop", ["rnn_layers.0.weight_ih_l0", "rnn_layers.1.weight_hh_l0", "rnn_layers.2.bias_ih_l0", "rnn_layers.2.bias_hh_l0"])
def test_a_missing_gru_tensor_raises(tmp_path, drop):
    from s3prl_amd.ckpt import load_apc_checkpoint

    with pytest.raises(ValueError, match=re.escape(drop)):
        load_apc_checkpoint(_save(tmp_path, _config(), drop=drop))


def test_missing_keys_are_named(tmp_path):
    import torch

    from s3prl_amd.ckpt import load_apc_checkpoint

    path = str(tmp_path / "c.pt")
    torch.save({"model": {}}, path)
    with pytest.raises(ValueError, match="config"):
        load_apc_checkpoint(path)
    torch.save({"config": _config()}, path)
    with pytest.raises(ValueError, match="model"):
        load_apc_checkpoint(path)
    with pytest.raises(ValueError, match="hidden_size"):
        load_apc_checkpoint(_save(tmp_path, {"data": {"audio": dict(feat_type="fbank", feat_dim=80)}, "model": {"paras": dict(num_layers=3, residual=True)}}))


REFUSALS = [
    (dict(paras=dict(num_layers=2)), "num_layers must be 3 or 4"),
    (dict(paras=dict(num_layers=1)), "num_layers must be 3 or 4"),
    (dict(paras=dict(num_layers=5)), "num_layers must be 3 or 4"),
    (dict(paras=dict(hidden_size=96)), "multiple of 64"),
    (dict(paras=dict(hidden_size=1024)), "at most 512"),
    (dict(audio=dict(feat_type="mfcc")), "feat_type='mfcc'"),
    (dict(audio=dict(num_ceps=13)), "['num_ceps']"),
    (dict(audio=dict(dither=1.0)), "['dither']"),
    (dict(audio=dict(window_type="hanning")), "['window_type']"),
    (dict(audio=dict(frame_length=25.1)), "multiple of 4 samples"),   # 401 samples
    (dict(audio=dict(frame_shift=10.125)), "multiple of 4 samples"),  # 162 samples
    (dict(audio=dict(feat_dim=82)), "feat_dim"),
]


@pytest.mark.parametrize("kw, match", REFUSALS)
def test_config_refusals(tmp_path, kw, match):
    from s3prl_amd.ckpt import load_apc_checkpoint
    from s3prl_amd.config import config_from_apc

    with pytest.raises(ValueError, match=re.escape(match)):
        config_from_apc(_config(**kw))
    with pytest.raises(ValueError, match=re.escape(match)):  # the checkpoint's own config decides
        load_apc_checkpoint(_save(tmp_path, _config(**kw)))


def _create_error(ccfg, apc):
    from s3prl_amd import _lib

    lib = _lib.load()
    h = C.c_void_p()
    tensors = (_lib.S3Tensor * 1)()
    assert lib.s3enc_create_apc(C.byref(ccfg), C.byref(apc) if apc is not None else None, tensors, 0, 0, C.byref(h)) != 0
    assert not h.value
    return lib.s3enc_last_error().decode()


@pytest.mark.parametrize("field, value, match", [
    ("num_layers", 2, "at least 3"),
    ("num_layers", 0, "at least 3"),
    ("num_layers", 5, "above 4"),
    ("window", 2, "window"),
    ("num_mel_bins", 82, "num_mel_bins"),
    ("frame_length_ms", 25.1, "multiple of 4 samples"),
    ("frame_shift_ms", 10.125, "multiple of 4 samples"),
    ("frame_shift_ms", 20.0, "frame geometry"),
])
def test_the_library_refuses_by_name(field, value, match):
    """s3enc_create_apc checks the configuration before it looks for a device: the refusals are the same without a GPU."""
    from s3prl_amd import _lib
    from s3prl_amd.synth import named_config

    cfg = named_config("tiny_apc")
    ccfg, apc = _lib.make_config(cfg, "fp32"), _lib.make_apc_config(cfg)
    assert ccfg.family == 7 and ccfg.n_conv == 1 and (ccfg.conv_kernel[0], ccfg.conv_stride[0]) == (400, 160) and ccfg.encoder_layers == 2
    assert (apc.num_mel_bins, apc.frame_length_ms, apc.frame_shift_ms, apc.window, apc.cmvn, apc.hidden, apc.num_layers,
            apc.residual) == (80, 25.0, 10.0, 1, 1, 64, 3, 1)
    setattr(apc, field, value)
    assert match in _create_error(ccfg, apc)


@pytest.mark.parametrize("width, match", [(96, "multiple of 64"), (576, "at most 512")])
def test_the_library_refuses_widths_the_recurrent_kernel_does_not_take(width, match):
    from s3prl_amd import _lib
    from s3prl_amd.synth import named_config

    cfg = named_config("tiny_apc")
    ccfg, apc = _lib.make_config(cfg, "fp32"), _lib.make_apc_config(cfg)
    ccfg.conv_dim = ccfg.embed_dim = apc.hidden = width
    assert match in _create_error(ccfg, apc)


@pytest.mark.parametrize("dtype", ["bf16", "fp16", "fp16x2", "fp32x3"])
def test_non_fp32_modes_are_refused_with_the_mode_named(dtype):
    from s3prl_amd import _lib
    from s3prl_amd.encoder import HipEncoder
    from s3prl_amd.synth import named_config, synth_weights

    cfg = named_config("tiny_apc")
    err = _create_error(_lib.make_config(cfg, dtype), _lib.make_apc_config(cfg))
    assert "fp32 only" in err and dtype in err
    with pytest.raises(ValueError, match="fp32 only"):
        HipEncoder(cfg, synth_weights(cfg, 0), dtype=dtype)


def test_the_apc_block_is_required_for_the_family_and_refused_elsewhere():
    from s3prl_amd import _lib
    from s3prl_amd.synth import named_config

    cfg = named_config("tiny_apc")
    lib = _lib.load()
    h = C.c_void_p()
    tensors = (_lib.S3Tensor * 1)()
    ccfg = _lib.make_config(cfg, "fp32")
    assert lib.s3enc_create(C.byref(ccfg), tensors, 0, 0, C.byref(h)) != 0 and b"s3enc_create_apc" in lib.s3enc_last_error()
    assert lib.s3enc_create_ex(C.byref(ccfg), None, tensors, 0, 0, C.byref(h)) != 0 and b"s3enc_create_apc" in lib.s3enc_last_error()
    cpc = _lib.make_cpc_config(named_config("tiny_cpc"))
    assert lib.s3enc_create_cpc(C.byref(ccfg), C.byref(cpc), tensors, 0, 0, C.byref(h)) != 0 and b"s3enc_create_apc" in lib.s3enc_last_error()
    assert "null argument" in _create_error(ccfg, None)
    assert "S3ENC_APC only" in _create_error(_lib.make_config(named_config("tiny_hubert"), "fp32"), _lib.make_apc_config(cfg))
    assert lib.s3enc_version() == 8  # every addition is a new symbol


def test_apc_block_follows_the_header(tmp_path):
    """s3enc_apc_config: field order against the header text, size and offsets against the header compiled as C; s3enc_config and
    s3enc_fbank_config stay what they were."""
    import subprocess

    from s3prl_amd import _lib

    header = open(os.path.join(ROOT, "include", "s3enc.h")).read()
    body = header[header.index("typedef struct s3enc_apc_config {"):header.index("} s3enc_apc_config;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = re.findall(r"(?:int32_t|float)\s+([a-z0-9_]+)(?:\[[^\]]*\])?;", body)
    assert names == [n for n, _ in _lib.S3ApcConfig._fields_] and names[0] == "num_mel_bins" and names[-1] == "residual"
    assert _lib.FAMILY["apc"] == 7 and "S3ENC_APC = 7" in header and "#define S3ENC_VERSION 8" in header
    assert [n for n, _ in _lib.S3Config._fields_][-1] == "dw_kernel"
    for sym in ("s3enc_create_apc", "s3enc_op_rnn_len", "s3enc_fbank_forward_ex"):
        assert re.search(r"\bint " + sym + r"\(", header), sym
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "s3enc.h"\n'
                   'int main(void){printf("%zu %zu %zu %zu %zu\\n", sizeof(s3enc_apc_config), offsetof(s3enc_apc_config, frame_shift_ms), '
                   'offsetof(s3enc_apc_config, window), offsetof(s3enc_apc_config, residual), sizeof(s3enc_fbank_config));return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    W = _lib.S3ApcConfig
    assert got == [C.sizeof(W), W.frame_shift_ms.offset, W.window.offset, W.residual.offset, C.sizeof(_lib.S3FbankConfig)]


def test_op_entries_validate_their_arguments():
    """s3enc_op_rnn_len and s3enc_fbank_forward_ex refuse bad arguments with a message before touching a device."""
    from s3prl_amd import _lib

    lib = _lib.load()
    one = C.c_void_p(256)
    lens = (C.c_int32 * 2)(3, 1)
    lp = C.cast(lens, C.c_void_p)
    call = lambda cell, b_hn, lp_, res, ld_res, B, T, H, ld_pre, out, ldo: lib.s3enc_op_rnn_len(  # noqa: E731
        cell, one, one, b_hn, lp_, res, ld_res, B, T, H, ld_pre, out, ldo, None)
    assert call(2, one, lp, None, 0, 2, 3, 64, 192, one, 64) != 0 and b"cell" in lib.s3enc_last_error()
    assert call(1, None, lp, None, 0, 2, 3, 64, 192, one, 64) != 0 and b"b_hn" in lib.s3enc_last_error()
    assert call(1, one, None, None, 0, 2, 3, 64, 192, one, 64) != 0 and b"null argument" in lib.s3enc_last_error()
    assert call(1, one, lp, None, 0, 2, 3, 96, 288, one, 96) != 0 and b"multiple of 64" in lib.s3enc_last_error()
    assert call(1, one, lp, None, 0, 2, 3, 576, 1728, one, 576) != 0 and b"at most 512" in lib.s3enc_last_error()
    assert call(1, one, lp, None, 0, 2, 3, 64, 191, one, 64) != 0 and b"ld_pre" in lib.s3enc_last_error()
    assert call(1, one, lp, one, 63, 2, 3, 64, 192, one, 64) != 0 and b"ld_res" in lib.s3enc_last_error()
    assert call(1, one, lp, None, 0, 2, 3, 64, 192, one, 66) != 0 and b"multiple of 4" in lib.s3enc_last_error()
    assert call(1, one, lp, None, 0, 2, 3, 64, 192, C.c_void_p(260), 64) != 0 and b"16-byte aligned" in lib.s3enc_last_error()
    assert call(1, one, lp, None, 0, 2, 2, 64, 192, one, 64) != 0 and b"1..T" in lib.s3enc_last_error()  # 3 > T
    lens[1] = 0
    assert call(1, one, lp, None, 0, 2, 3, 64, 192, one, 64) != 0 and b"1..T" in lib.s3enc_last_error()
    fc = _lib.S3FbankConfig()
    ln = (C.c_int64 * 1)(4000)
    assert lib.s3enc_fbank_forward_ex(C.byref(fc), 2, one, ln, 1, one, 23, 0, None) != 0 and b"window" in lib.s3enc_last_error()


def test_hub_names_have_the_reference_signatures():
    import s3prl_amd.hub as amd

    ref = json.load(open(os.path.join(ROOT, "tests", "golden", "apc", "reference_hub_apc.json")))
    everything = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_hub.json")))["options"]
    assert ref["downsample_rate"] == 160
    checked = []
    for fam in ("apc", "vq_apc"):
        for name, params in ref["hubconfs"][fam]:
            assert name in everything and name in amd.options(), name
            ours = inspect.signature(getattr(amd, name))
            assert [list(p) for p in params] == [[k, v.kind.name, repr(v.default)] for k, v in ours.parameters.items()], name
            checked.append(name)
    assert sorted(checked) == ["apc", "apc_360hr", "apc_960hr", "apc_local", "apc_url", "vq_apc", "vq_apc_360hr", "vq_apc_960hr",
                               "vq_apc_url"]
    reg = set(amd.options(only_registered_ckpt=True))
    assert {"apc", "apc_360hr", "apc_960hr", "vq_apc", "vq_apc_360hr", "vq_apc_960hr"} <= reg
    assert not {"apc_local", "apc_url", "vq_apc_url"} & reg
    assert amd.vq_apc_url is amd.apc_url


def test_expert_loads_a_checkpoint_and_reports_the_reference_geometry(tmp_path):
    """Without a GPU: construction, the stride, the state count and sizes; the forward itself needs the MI355X."""
    import torch

    import s3prl_amd.hub as amd
    from s3prl_amd.ckpt import save_checkpoint
    from s3prl_amd.synth import named_config, synth_weights
    from s3prl_amd.upstream.vq_apc.expert import UpstreamExpert as VqExpert

    for name in ("tiny_apc_l4", "tiny_vq_apc"):
        cfg = named_config(name)
        path = str(tmp_path / "c.pt")
        save_checkpoint(path, cfg, synth_weights(cfg, 0))
        expert = amd.apc_local(path) if name == "tiny_apc_l4" else VqExpert(path)
        assert expert.cfg == cfg and expert.get_downsample_rates("hidden_states") == 160
        assert expert.num_layers == 3 and expert.hidden_sizes == [cfg.conv_dim] * 3
        assert expert._states_info(3) == ("self.model.rnn_layers[1]", "self.model.rnn_layers[2]", "self.model")
        wav = torch.zeros(4000, requires_grad=True)
        with pytest.raises(RuntimeError, match="inference-only"):
            expert([wav])
        if not torch.cuda.is_available():
            with pytest.raises(RuntimeError, match="no CPU fallback"):
                expert([torch.zeros(4000)])
