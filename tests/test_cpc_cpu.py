"""modified CPC without a GPU: the float64 restatement of tests/cpc_ref.py against every reference-generated fixture, its LSTM and
GRU against torch's in float64, the frame arithmetic with the paddings, checkpoint reading (defaults, overrides, missing tensors),
the refusals by name (Python and s3enc_create_cpc), the configuration block against the header, and the hub names."""

import ctypes as C
import inspect
import json
import os
import re
import sys

import numpy as np
import pytest

from oracle import encoder_oracle as O

import cpc_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import ref_shim  # noqa: E402

NAMES = ["cpc_tiny_pad", "cpc_tiny_eq", "cpc_tiny_t1", "cpc_tiny_gru_pad", "cpc_tiny_lstm1_pad", "cpc_base_pseudo", "cpc_base_10s"]
FIXTURES = ["cpc/" + n for n in NAMES]
REF_PIN = 1e-6  # the pin of tests/test_wav2vec_cpu.py: a float64 restatement against the reference's fp32 outputs


@pytest.mark.parametrize("name", FIXTURES)
def test_float64_restatement_matches_the_reference(name, golden_loader):
    meta, cfg, weights, wavs, hs, norms = golden_loader(name)
    assert len(hs) == cfg.num_hidden_states == 2 and meta["n_states"] == 2
    out = R.forward(cfg, weights, wavs)
    ts, cs = meta["t_stride"], meta["c_stride"]
    assert meta["shape"] == [len(wavs), cfg.num_frames(max(meta["lengths"])), cfg.conv_dim]
    for l, h in enumerate(out["hidden_states"]):
        assert list(h.shape) == meta["shape"]
        assert O.rel_err(h[:, ::ts, ::cs], hs[l]) <= REF_PIN, (name, l)
        assert abs(np.linalg.norm(h) - norms[l]) / norms[l] <= REF_PIN
    # the gates leave their linear range in every recurrent layer (the generator's own condition, re-measured)
    assert len(meta["gate_std"]) == cfg.ar_layers and min(meta["gate_std"]) >= 1.0
    assert np.allclose(out["gate_std"], meta["gate_std"], rtol=1e-9)


def test_fixture_table():
    """The fixtures the issue names: configurations, lengths and strides."""
    from conftest import golden_meta

    want = {"cpc_tiny_pad": ("tiny_cpc", [4000, 2345, 3111], 25), "cpc_tiny_eq": ("tiny_cpc", [3200, 3200], 20),
            "cpc_tiny_t1": ("tiny_cpc", [159, 163], 1), "cpc_tiny_gru_pad": ("tiny_cpc_gru", [4000, 2345, 3111], 25),
            "cpc_tiny_lstm1_pad": ("tiny_cpc_lstm1", [4000, 2345, 3111], 25), "cpc_base_pseudo": ("cpc_base", [16000, 12345], 100),
            "cpc_base_10s": ("cpc_base", [160000], 1000)}
    for name, (cfg, lengths, T) in want.items():
        m = golden_meta("cpc/" + name)
        assert (m["config"], m["lengths"], m["shape"][1]) == (cfg, lengths, T), name
        assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "cpc", name + ".npz")) < 256 * 1024
    m = golden_meta("cpc/cpc_tiny_eq")
    assert (m["dc"], m["scale"]) == (0.1, 0.5)
    assert golden_meta("cpc/cpc_base_pseudo")["c_stride"] == 4
    m = golden_meta("cpc/cpc_base_10s")
    assert (m["t_stride"], m["c_stride"]) == (4, 8)


@pytest.mark.skipif(not os.path.isdir(ref_shim.REFERENCE), reason="runs where the reference tree is present")
@pytest.mark.parametrize("cell", ["LSTM", "GRU"])
@pytest.mark.parametrize("layers", [1, 3])
def test_restated_cells_match_torch_in_float64(cell, layers):
    import torch

    B, T, I, H = 3, 19, 24, 40
    torch.manual_seed(7)
    net = (torch.nn.LSTM if cell == "LSTM" else torch.nn.GRU)(I, H, num_layers=layers, batch_first=True).double()
    with torch.no_grad():
        for p in net.parameters():
            p.mul_(6.0)  # gates outside their linear range
        x = torch.randn(B, T, I, dtype=torch.float64)
        want = net(x)[0].numpy()
    h = x.numpy()
    for l in range(layers):
        g = lambda n: getattr(net, f"{n}_l{l}").detach().numpy()  # noqa: E731
        h, gates = R.rnn_layer(h, g("weight_ih"), g("weight_hh"), g("bias_ih"), g("bias_hh"), cell)
        assert gates.std() > 1.0
    assert np.abs(h - want).max() <= 1e-12


@pytest.mark.parametrize("n, T", [(160000, 1000), (16000, 100), (4000, 25), (159, 1), (158, 0)])
def test_frame_arithmetic(n, T):
    from s3prl_amd.synth import named_config

    for name in ("tiny_cpc", "tiny_cpc_gru", "cpc_base"):
        cfg = named_config(name)
        assert cfg.num_frames(n) == T and cfg.num_output_frames(n) == T
        assert cfg.valid_frames(n, 160000) == T and cfg.downsample_rate == 160
        assert cfg.num_hidden_states == 2


def test_conv_lengths_follow_the_paddings():
    from s3prl_amd.synth import named_config

    cfg = named_config("cpc_base")
    assert cfg.conv_pads == [3, 2, 1, 1, 1] and [(k, s) for _, k, s in cfg.conv_layers] == [(10, 5), (8, 4), (4, 2), (4, 2), (4, 2)]
    assert cfg.conv_lengths(160000) == [32000, 8000, 4000, 2000, 1000]
    assert cfg.conv_lengths(159) == [32, 8, 4, 2, 1] and cfg.conv_lengths(158)[-1] == 0
    assert cfg.valid_frames(2345, 4000) == 14 and cfg.valid_frames(100, 4000) == 0


def _save(tmp_path, config, weights_of="tiny_cpc", drop=None):
    import torch

    from s3prl_amd.synth import named_config, synth_weights

    cfg = named_config(weights_of)
    sd = {k: torch.from_numpy(v) for k, v in synth_weights(cfg, 3).items() if k != drop}
    path = str(tmp_path / "c.pt")
    torch.save({"config": config, "weights": sd}, path)
    return path


def test_checkpoint_defaults_and_overrides(tmp_path):
    import torch

    from s3prl_amd.ckpt import load_checkpoint, load_cpc_checkpoint, save_checkpoint
    from s3prl_amd.config import config_from_cpc
    from s3prl_amd.synth import named_config, synth_weights

    d = config_from_cpc({})  # cpc_default_config.py
    assert (d.conv_dim, d.ar_hidden, d.ar_mode, d.ar_layers, d.norm_mode) == (256, 256, "LSTM", 1, "layerNorm")
    over = config_from_cpc(dict(hiddenEncoder=128, hiddenGar=128, arMode="GRU", nLevelsGRU=3, nPredicts=12, dropout=False))
    assert (over.conv_dim, over.ar_hidden, over.ar_mode, over.ar_layers) == (128, 128, "GRU", 3)
    for name in ("tiny_cpc", "tiny_cpc_gru", "tiny_cpc_lstm1", "cpc_base"):
        cfg = named_config(name)
        weights = synth_weights(cfg, 5)
        path = str(tmp_path / "c.pt")
        save_checkpoint(path, cfg, weights)
        state = torch.load(path, map_location="cpu", weights_only=False)
        assert set(state) == {"config", "weights"}  # cpc/expert.py:30-36
        state["weights"]["gAR.baseNet.weight_ih_l9"] = torch.zeros(4)  # a tensor the forward never reads is dropped
        torch.save(state, path)
        cfg2, back = load_cpc_checkpoint(path)
        assert cfg2 == cfg and load_checkpoint(path, "cpc")[0] == cfg
        assert set(back) == set(weights) and all(np.array_equal(back[k], weights[k]) for k in weights)
    assert named_config("tiny_cpc").ar_layers == 2 and named_config("cpc_base").conv_dim == 256


@pytest.mark.parametrize("drop", ["gEncoder.conv3.bias", "gEncoder.batchNorm0.weight", "gAR.baseNet.weight_hh_l1", "gAR.baseNet.bias_ih_l0"])
def test_a_missing_tensor_raises(tmp_path, drop):
    from s3prl_amd.ckpt import load_cpc_checkpoint

    path = _save(tmp_path, dict(hiddenEncoder=64, hiddenGar=64, nLevelsGRU=2), drop=drop)
    with pytest.raises(ValueError, match=re.escape(drop)):
        load_cpc_checkpoint(path)


def test_missing_keys_are_named(tmp_path):
    import torch

    from s3prl_amd.ckpt import load_cpc_checkpoint

    path = str(tmp_path / "c.pt")
    torch.save({"weights": {}}, path)
    with pytest.raises(ValueError, match="config"):
        load_cpc_checkpoint(path)
    torch.save({"config": {}}, path)
    with pytest.raises(ValueError, match="weights"):
        load_cpc_checkpoint(path)


REFUSALS = [
    (dict(normMode="batchNorm"), "normMode='batchNorm'"),
    (dict(normMode="instanceNorm"), "normMode='instanceNorm'"),
    (dict(normMode="ID"), "normMode='ID'"),
    (dict(arMode="RNN"), "arMode='RNN'"),
    (dict(arMode="transformer"), "arMode='transformer'"),
    (dict(arMode="no_ar"), "arMode='no_ar'"),
    (dict(cpc_mode="reverse"), "cpc_mode='reverse'"),
    (dict(samplingType="sequential"), "samplingType='sequential'"),
    (dict(hiddenGar=128), "hiddenGar != hiddenEncoder"),
    (dict(hiddenEncoder=96, hiddenGar=96), "multiple of 64"),
    (dict(hiddenEncoder=1024, hiddenGar=1024), "at most 512"),
    (dict(nLevelsGRU=5), "nLevelsGRU"),
    (dict(encoder_type="mfcc"), "encoder_type='mfcc'"),
    (dict(encoder_type="lfb"), "encoder_type='lfb'"),
]


@pytest.mark.parametrize("kw, match", REFUSALS)
def test_config_refusals(tmp_path, kw, match):
    from s3prl_amd.ckpt import load_cpc_checkpoint
    from s3prl_amd.config import config_from_cpc

    with pytest.raises(ValueError, match=re.escape(match)):
        config_from_cpc(kw)
    with pytest.raises(ValueError, match=re.escape(match)):  # the checkpoint's own config decides
        load_cpc_checkpoint(_save(tmp_path, kw))


def _create_error(ccfg, cpc):
    from s3prl_amd import _lib

    lib = _lib.load()
    h = C.c_void_p()
    tensors = (_lib.S3Tensor * 1)()
    assert lib.s3enc_create_cpc(C.byref(ccfg), C.byref(cpc) if cpc is not None else None, tensors, 0, 0, C.byref(h)) != 0
    assert not h.value
    return lib.s3enc_last_error().decode()


@pytest.mark.parametrize("field, value, match", [
    ("norm_mode", 1, 'normMode="instanceNorm"'),
    ("norm_mode", 2, 'normMode="ID"'),
    ("norm_mode", 3, 'normMode="batchNorm"'),
    ("ar_mode", 2, 'arMode="RNN"'),
    ("ar_mode", 3, 'arMode="transformer"'),
    ("ar_mode", 4, 'arMode="no_ar"'),
    ("reverse", 1, 'cpc_mode="reverse"'),
    ("keep_hidden", 1, 'samplingType="sequential"'),
    ("ar_hidden", 128, "hiddenGar != hiddenEncoder"),
    ("ar_layers", 5, "nLevelsGRU"),
    ("ar_layers", 0, "nLevelsGRU"),
    ("conv_pad", 9, "padding"),
])
def test_the_library_refuses_by_name(field, value, match):
    """s3enc_create_cpc checks the configuration before it looks for a device: the refusals are the same without a GPU."""
    from s3prl_amd import _lib
    from s3prl_amd.synth import named_config

    cfg = named_config("tiny_cpc")
    ccfg, cpc = _lib.make_config(cfg, "fp32"), _lib.make_cpc_config(cfg)
    assert ccfg.family == 6 and ccfg.n_conv == 5 and list(cpc.conv_pad)[:5] == [3, 2, 1, 1, 1] and ccfg.encoder_layers == 1
    assert (cpc.norm_mode, cpc.ar_mode, cpc.ar_layers, cpc.ar_hidden, cpc.reverse, cpc.keep_hidden) == (0, 0, 2, 64, 0, 0)
    if field == "conv_pad":
        cpc.conv_pad[1] = value
    else:
        setattr(cpc, field, value)
    assert match in _create_error(ccfg, cpc)


@pytest.mark.parametrize("width, match", [(96, "multiple of 64"), (576, "at most 512")])
def test_the_library_refuses_widths_the_recurrent_kernel_does_not_take(width, match):
    from s3prl_amd import _lib
    from s3prl_amd.synth import named_config

    cfg = named_config("tiny_cpc")
    ccfg, cpc = _lib.make_config(cfg, "fp32"), _lib.make_cpc_config(cfg)
    ccfg.conv_dim = ccfg.embed_dim = cpc.ar_hidden = width
    assert match in _create_error(ccfg, cpc)


@pytest.mark.parametrize("dtype", ["bf16", "fp16", "fp16x2", "fp32x3"])
def test_non_fp32_modes_are_refused_with_the_mode_named(dtype):
    from s3prl_amd import _lib
    from s3prl_amd.synth import named_config

    cfg = named_config("tiny_cpc_gru")
    err = _create_error(_lib.make_config(cfg, dtype), _lib.make_cpc_config(cfg))
    assert "fp32 only" in err and dtype in err


def test_the_cpc_block_is_required_for_the_family_and_refused_elsewhere():
    from s3prl_amd import _lib
    from s3prl_amd.synth import named_config

    cfg = named_config("tiny_cpc")
    lib = _lib.load()
    h = C.c_void_p()
    tensors = (_lib.S3Tensor * 1)()
    ccfg = _lib.make_config(cfg, "fp32")
    assert lib.s3enc_create(C.byref(ccfg), tensors, 0, 0, C.byref(h)) != 0 and b"s3enc_create_cpc" in lib.s3enc_last_error()
    assert lib.s3enc_create_ex(C.byref(ccfg), None, tensors, 0, 0, C.byref(h)) != 0 and b"s3enc_create_cpc" in lib.s3enc_last_error()
    w2v = _lib.make_wav2vec_config(named_config("tiny_wav2vec"))
    assert lib.s3enc_create_ex(C.byref(ccfg), C.byref(w2v), tensors, 0, 0, C.byref(h)) != 0 and b"s3enc_create_cpc" in lib.s3enc_last_error()
    assert "null argument" in _create_error(ccfg, None)
    assert "S3ENC_CPC only" in _create_error(_lib.make_config(named_config("tiny_hubert"), "fp32"), _lib.make_cpc_config(cfg))


def test_cpc_block_follows_the_header(tmp_path):
    """s3enc_cpc_config: field order against the header text, size and offsets against the header compiled as C; s3enc_config
    stays what it was."""
    import subprocess

    from s3prl_amd import _lib

    header = open(os.path.join(ROOT, "include", "s3enc.h")).read()
    body = header[header.index("typedef struct s3enc_cpc_config {"):header.index("} s3enc_cpc_config;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = re.findall(r"(?:int32_t|float)\s+([a-z0-9_]+)(?:\[[^\]]*\])?;", body)
    assert names == [n for n, _ in _lib.S3CpcConfig._fields_] and names[0] == "conv_pad" and names[-1] == "keep_hidden"
    assert _lib.FAMILY["cpc"] == 6 and "S3ENC_CPC = 6" in header
    assert [n for n, _ in _lib.S3Config._fields_][-1] == "dw_kernel"
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "s3enc.h"\n'
                   'int main(void){printf("%zu %zu %zu %zu\\n", sizeof(s3enc_cpc_config), offsetof(s3enc_cpc_config, norm_mode), '
                   'offsetof(s3enc_cpc_config, ar_hidden), offsetof(s3enc_cpc_config, keep_hidden));return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    W = _lib.S3CpcConfig
    assert got == [C.sizeof(W), W.norm_mode.offset, W.ar_hidden.offset, W.keep_hidden.offset]


def test_op_entries_validate_their_arguments():
    """The two op entries refuse bad shapes with a message before touching a device."""
    from s3prl_amd import _lib

    lib = _lib.load()
    one = C.c_void_p(256)
    assert lib.s3enc_op_rnn(2, one, one, None, 1, 1, 64, 256, one, 64, None) != 0 and b"cell" in lib.s3enc_last_error()
    assert lib.s3enc_op_rnn(0, one, one, None, 1, 1, 96, 384, one, 96, None) != 0 and b"multiple of 64" in lib.s3enc_last_error()
    assert lib.s3enc_op_rnn(0, one, one, None, 1, 1, 576, 2304, one, 576, None) != 0 and b"at most 512" in lib.s3enc_last_error()
    assert lib.s3enc_op_rnn(1, one, one, None, 1, 1, 64, 192, one, 64, None) != 0 and b"b_hn" in lib.s3enc_last_error()
    assert lib.s3enc_op_rnn(0, one, one, one, 1, 1, 64, 256, one, 64, None) != 0 and b"b_hn" in lib.s3enc_last_error()
    assert lib.s3enc_op_rnn(0, one, one, None, 1, 1, 64, 255, one, 64, None) != 0 and b"ld_pre" in lib.s3enc_last_error()
    assert lib.s3enc_op_channelnorm_relu(one, None, None, 1, 1, 66, 0, one, None, None) != 0 and b"C % 4" in lib.s3enc_last_error()
    assert lib.s3enc_op_channelnorm_relu(one, None, None, 1, 1, 64, 1, None, one, None) != 0 and b"border rows" in lib.s3enc_last_error()
    assert lib.s3enc_op_channelnorm_relu(one, None, None, 1, 1, 64, 0, None, None, None) != 0


def test_hub_names_have_the_reference_signatures():
    import s3prl_amd.hub as amd

    ref = json.load(open(os.path.join(ROOT, "tests", "golden", "cpc", "reference_hub_cpc.json")))
    everything = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_hub.json")))["options"]
    assert ref["downsample_rate"] == 160
    checked = []
    for name, params in ref["hubconfs"]["cpc"]:
        assert name in everything and name in amd.options(), name
        ours = inspect.signature(getattr(amd, name))
        assert [list(p) for p in params] == [[k, v.kind.name, repr(v.default)] for k, v in ours.parameters.items()], name
        checked.append(name)
    assert sorted(checked) == ["cpc_local", "cpc_url", "modified_cpc"]
    reg = set(amd.options(only_registered_ckpt=True))
    assert "modified_cpc" in reg and "cpc_local" not in reg and "cpc_url" not in reg
    assert amd.modified_cpc.url.endswith("CPC_checkpoints/60k_epoch4-d0f474de.pt")


def test_expert_loads_a_checkpoint_and_reports_the_reference_geometry(tmp_path):
    """Without a GPU: construction, the stride, the state count and sizes; the forward itself needs the MI355X."""
    import torch

    import s3prl_amd.hub as amd
    from s3prl_amd.ckpt import save_checkpoint
    from s3prl_amd.synth import named_config, synth_weights

    cfg = named_config("tiny_cpc_gru")
    path = str(tmp_path / "c.pt")
    save_checkpoint(path, cfg, synth_weights(cfg, 0))
    expert = amd.cpc_local(path)
    assert expert.cfg == cfg and expert.get_downsample_rates("hidden_states") == 160
    assert expert.num_layers == 2 and expert.hidden_sizes == [64, 64]
    assert expert._states_info(2) == ("self.model.gEncoder", "self.model.gAR")
    wav = torch.zeros(4000, requires_grad=True)
    with pytest.raises(RuntimeError, match="inference-only"):
        expert([wav])
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            expert([torch.zeros(4000)])
    with pytest.raises(ValueError, match="fp32 only"):
        from s3prl_amd.encoder import HipEncoder

        HipEncoder(cfg, synth_weights(cfg, 0), dtype="bf16")
