"""DeCoAR / DeCoAR-layers without a GPU: the float64 restatement of tests/decoar_ref.py against every reference-generated fixture
and against torch's nn.LSTM on packed sequences, the frame arithmetic, checkpoint reading, the refusals by name (Python and
s3enc_create_decoar), the configuration block against the header and the hub names."""

import ctypes as C
import inspect
import json
import os
import re

import numpy as np
import pytest

from oracle import encoder_oracle as O
from oracle import fbank_oracle as FO

import decoar_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NAMES = ["decoar_tiny_pad", "decoar_tiny_eq", "decoar_tiny_t2", "decoar_tiny_l1", "decoar_layers_tiny_pad", "decoar_layers_tiny_h192"]
FIXTURES = ["decoar/" + n for n in NAMES]
REF_PIN = 1e-6  # the project's restatement bound: a float64 restatement against the reference's fp32 outputs


@pytest.mark.parametrize("name", FIXTURES)
def test_float64_restatement_matches_the_reference(name, golden_loader):
    meta, cfg, weights, wavs, hs, norms = golden_loader(name)
    feats, lens = R.features(cfg, wavs)
    out = R.model(cfg, weights, feats.astype(np.float32), lens)  # the generator fed the reference these features ROUNDED TO fp32
    NS = cfg.decoar_layers if cfg.decoar_per_layer else 1
    assert len(hs) == cfg.num_hidden_states == meta["n_states"] == NS
    assert lens == meta["frames"] == [cfg.num_frames(n) for n in meta["lengths"]]
    ts, cs = meta["t_stride"], meta["c_stride"]
    assert meta["shape"] == [len(wavs), cfg.num_frames(max(meta["lengths"])), 2 * cfg.decoar_hidden]
    for l, h in enumerate(out["hidden_states"]):
        assert list(h.shape) == meta["shape"]
        assert O.rel_err(h[:, ::ts, ::cs], hs[l]) <= REF_PIN, (name, l)
        assert abs(np.linalg.norm(h) - norms[l]) / norms[l] <= REF_PIN
        for b, n in enumerate(lens):  # pad_packed_sequence: exactly zero behind every utterance's frames, on both sides
            assert not h[b, n:].any() and not hs[l][b, -(-n // ts):].any()
            assert O.rel_err(h[b, :n:ts, ::cs], hs[l][b, :-(-n // ts)]) <= REF_PIN, (name, l, b)
    assert len(meta["gate_std"]) == 2 * cfg.decoar_layers and min(meta["gate_std"]) >= 1.0  # per layer and direction
    assert np.allclose(out["gate_std"], meta["gate_std"], rtol=1e-9)
    assert max(meta["ref_fp32_err"]) <= 8e-7 and max(meta["fp32_proxy_err"]) <= 0.25e-4


def test_fixture_table():
    """The fixtures: configurations, lengths, frames."""
    from conftest import golden_meta

    from s3prl_amd.synth import named_config

    want = {"decoar_tiny_pad": ("tiny_decoar", [4000, 2345, 3111], 23), "decoar_tiny_eq": ("tiny_decoar", [3200, 3200], 18),
            "decoar_tiny_t2": ("tiny_decoar", [560, 2000], 11), "decoar_tiny_l1": ("tiny_decoar_l1", [4000, 2345, 3111], 23),
            "decoar_layers_tiny_pad": ("tiny_decoar_layers", [4000, 2345, 3111], 23),
            "decoar_layers_tiny_h192": ("tiny_decoar_h192", [4000, 2345, 3111], 23)}
    assert sorted(want) == sorted(NAMES)
    for name, (cfg, lengths, T) in want.items():
        m = golden_meta("decoar/" + name)
        assert (m["config"], m["lengths"], m["shape"][1]) == (cfg, lengths, T), name
        assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "decoar", name + ".npz")) < 512 * 1024
    assert (golden_meta("decoar/decoar_tiny_pad")["n_states"], golden_meta("decoar/decoar_layers_tiny_pad")["n_states"]) == (1, 3)
    assert golden_meta("decoar/decoar_tiny_t2")["frames"] == [2, 11]  # the fewest frames the front end's std over time allows
    assert len(set(golden_meta("decoar/decoar_tiny_pad")["frames"])) == 3 and len(set(golden_meta("decoar/decoar_tiny_eq")["frames"])) == 1
    c = named_config("decoar")
    assert (c.decoar_hidden, c.decoar_layers, c.decoar_feat_dim, c.decoar_subsample, c.encoder_embed_dim, c.num_hidden_states) == \
           (1024, 4, 80, 1, 2048, 1)
    assert named_config("decoar_layers").num_hidden_states == 4 and named_config("tiny_decoar_h192").decoar_hidden == 192
    assert named_config("tiny_decoar_l1").decoar_layers == 1 and named_config("tiny_decoar_sub2").decoar_subsample == 2


# ---- the model ---------------------------------------------------------------------------------------------------------------
def test_stacks_match_torch_lstm_on_packed_sequences_in_float64():
    """decoar_ref's forward and backward stacks against nn.LSTM on pack_padded_sequence, the backward one between two flips of
    every utterance's own rows."""
    import torch
    from torch.nn.utils.rnn import pack_padded_sequence, pad_packed_sequence

    B, T, H, NL = 3, 11, 24, 2
    lens = [11, 1, 6]
    torch.manual_seed(3)
    nets = [torch.nn.LSTM(H, H, num_layers=NL, batch_first=True).double() for _ in range(2)]
    weights = {}
    with torch.no_grad():
        for stack, net in zip(R.STACKS, nets):
            for n, p in net.named_parameters():
                p.mul_(6.0)
                weights[f"{stack}.{n}"] = p.detach().numpy().copy()
        x = torch.randn(B, T, H, dtype=torch.float64)

        def run(net, inp):
            packed = pack_padded_sequence(inp, torch.LongTensor(lens), batch_first=True, enforce_sorted=False)
            return pad_packed_sequence(net(packed)[0], batch_first=True, total_length=T)[0]

        def flipped(t):
            t = t.clone()
            for b, n in enumerate(lens):
                t[b, :n] = t[b, :n].flip(dims=[0])
            return t

        want_f, want_b = run(nets[0], x).numpy(), flipped(run(nets[1], flipped(x))).numpy()
    for b, n in enumerate(lens):
        fwd, gates = R.lstm_stack(x[b, :n].numpy(), weights, R.STACKS[0], NL)
        bwd, _ = R.lstm_stack(R.flip(x[b, :n].numpy()), weights, R.STACKS[1], NL)
        assert gates[0].std() > 1.0
        assert np.abs(fwd[-1] - want_f[b, :n]).max() <= 1e-12 and np.abs(R.flip(bwd[-1]) - want_b[b, :n]).max() <= 1e-12
        assert not want_f[b, n:].any() and not want_b[b, n:].any()


def test_front_end_and_subsampling():
    from s3prl_amd.synth import named_config

    import apc_ref

    cfg, sub = named_config("tiny_decoar"), named_config("tiny_decoar_sub2")
    wavs = [np.random.default_rng(1).standard_normal(n) for n in (4000, 2345)]
    x, lens = R.features(cfg, wavs)
    assert x.shape == (2, 23, 80) and lens == [23, 13] and not x[1, 13:].any()
    for b, n in enumerate(lens):  # the hamming front end of APC with CMVN over time
        assert np.array_equal(x[b, :n], apc_ref.cmvn(apc_ref.kaldi_fbank(wavs[b])))
    x2, lens2 = R.features(sub, wavs)
    assert lens2 == [12, 7] and np.array_equal(x2[0], x[0, ::2]) and np.array_equal(x2[1, :7], x[1, :13:2])  # ceil(f / 2) frames


@pytest.mark.parametrize("n, f", [(160000, 998), (16000, 98), (8000, 48), (5555, 33), (560, 2), (400, 1), (399, 0)])
def test_frame_arithmetic(n, f):
    from s3prl_amd.synth import named_config

    for name in ("tiny_decoar", "tiny_decoar_layers", "decoar"):
        cfg = named_config(name)
        assert cfg.num_frames(n) == f == FO.num_frames(n) and cfg.num_output_frames(n) == f
        assert cfg.valid_frames(n, 160000) == f and cfg.downsample_rate == 160
    sub = named_config("tiny_decoar_sub2")
    assert sub.num_frames(n) == -(-f // 2) and sub.downsample_rate == 160  # what the reference's get_downsample_rates returns
    assert named_config("tiny_decoar").valid_frames(2345, 4000) == 13 and sub.valid_frames(5555, 8000) == 17


# ---- checkpoints -----------------------------------------------------------------------------------------------------------
def test_checkpoint_round_trip_and_both_experts_read_one_file(tmp_path):
    import torch

    import s3prl_amd.hub as amd
    from s3prl_amd.ckpt import load_checkpoint, load_decoar_checkpoint, save_checkpoint
    from s3prl_amd.synth import named_config, synth_weights

    for name in ("tiny_decoar", "tiny_decoar_l1", "tiny_decoar_h192"):
        cfg = named_config(name)
        weights = synth_weights(cfg, 5)
        assert len(weights) == 2 + 8 * cfg.decoar_layers
        assert {"post_extract_proj.weight", "post_extract_proj.bias", "forward_lstm.weight_ih_l0", "backward_lstm.bias_hh_l0"} <= set(weights)
        path = str(tmp_path / "c.pt")
        save_checkpoint(path, cfg, weights)
        state = torch.load(path, map_location="cpu", weights_only=False)
        assert set(state) == {"model"}  # decoar/expert.py:30
        cfg2, back = load_decoar_checkpoint(path)
        one = named_config(name) if not cfg.decoar_per_layer else None
        assert (cfg2.decoar_hidden, cfg2.decoar_layers, cfg2.decoar_feat_dim, cfg2.decoar_per_layer) == \
               (cfg.decoar_hidden, cfg.decoar_layers, 80, False)
        assert one is None or cfg2 == one
        assert load_checkpoint(path, "decoar")[0] == cfg2
        assert set(back) == set(weights) and all(np.array_equal(back[k], weights[k]) for k in weights)
        a, b = amd.decoar_local(path), amd.decoar_layers_local(ckpt=path)
        assert a.cfg == cfg2 and not a.cfg.decoar_per_layer and b.cfg.decoar_per_layer
        assert a.num_layers == 1 and b.num_layers == cfg.decoar_layers
        assert a.hidden_sizes == [2 * cfg.decoar_hidden] and b.hidden_sizes == [2 * cfg.decoar_hidden] * cfg.decoar_layers
        assert a.get_downsample_rates("hidden_states") == b.get_downsample_rates("hidden_states") == 160
        assert all(np.array_equal(a._weights[k], b._weights[k]) for k in weights)
        with pytest.raises(RuntimeError, match="inference-only"):
            a([torch.zeros(4000, requires_grad=True)])
        if not torch.cuda.is_available():
            with pytest.raises(RuntimeError, match="no CPU fallback"):
                b([torch.zeros(4000)])


@pytest.mark.parametrize("drop", ["post_extract_proj.weight", "post_extract_proj.bias", "forward_lstm.weight_ih_l0",
                                  "forward_lstm.weight_hh_l0", "backward_lstm.weight_hh_l1", "backward_lstm.bias_ih_l1",
                                  "forward_lstm.bias_hh_l1"])
def test_a_missing_tensor_raises(tmp_path, drop):
    import torch

    from s3prl_amd.ckpt import load_decoar_checkpoint
    from s3prl_amd.synth import named_config, synth_weights

    sd = {k: torch.from_numpy(v) for k, v in synth_weights(named_config("tiny_decoar"), 3).items() if k != drop}
    path = str(tmp_path / "c.pt")
    torch.save({"model": sd}, path)
    with pytest.raises(ValueError, match=re.escape(drop)):
        load_decoar_checkpoint(path)
    torch.save({"weights": sd}, path)
    with pytest.raises(ValueError, match="model"):
        load_decoar_checkpoint(path)


# ---- refusals on both sides of the ABI -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw, match", [
    (dict(num_layers=0), "num_layers must be 1..4"),
    (dict(num_layers=5), "num_layers must be 1..4"),
    (dict(hidden=96), "multiple of 64"),
    (dict(hidden=1088), "at most 1024"),
    (dict(subsample=3), "subsample must be 1 or 2"),
    (dict(feat_dim=82), "num_mel_bins"),
    (dict(frame_length=25.1), "multiple of 4 samples"),
    (dict(frame_shift=10.125), "multiple of 4 samples"),
])
def test_config_refusals(kw, match):
    from s3prl_amd.config import decoar_config

    with pytest.raises(ValueError, match=re.escape(match)):
        decoar_config(**{**dict(hidden=64, num_layers=2), **kw})


def _create_error(ccfg, dc):
    from s3prl_amd import _lib

    lib = _lib.load()
    h = C.c_void_p()
    tensors = (_lib.S3Tensor * 1)()
    assert lib.s3enc_create_decoar(C.byref(ccfg), C.byref(dc) if dc is not None else None, tensors, 0, 0, C.byref(h)) != 0
    assert not h.value
    return lib.s3enc_last_error().decode()


@pytest.mark.parametrize("field, value, match", [
    ("num_layers", 0, "num_layers must be 1..4"),
    ("num_layers", 5, "num_layers must be 1..4"),
    ("subsample", 0, "subsample must be 1 or 2"),
    ("subsample", 3, "subsample must be 1 or 2"),
    ("per_layer_states", 2, "per_layer_states"),
    ("per_layer_states", 1, "number of states - 1"),  # the two blocks disagree
    ("num_mel_bins", 82, "num_mel_bins"),
    ("frame_length_ms", 25.1, "multiple of 4 samples"),
    ("frame_shift_ms", 10.125, "multiple of 4 samples"),
    ("frame_shift_ms", 20.0, "frame geometry"),
])
def test_the_library_refuses_by_name(field, value, match):
    """s3enc_create_decoar checks the configuration before it looks for a device: the refusals are the same without a GPU."""
    from s3prl_amd import _lib
    from s3prl_amd.synth import named_config

    cfg = named_config("tiny_decoar")
    ccfg, dc = _lib.make_config(cfg, "fp32"), _lib.make_decoar_config(cfg)
    assert ccfg.family == 9 and ccfg.n_conv == 1 and (ccfg.conv_kernel[0], ccfg.conv_stride[0]) == (400, 160)
    assert (ccfg.conv_dim, ccfg.embed_dim, ccfg.encoder_layers) == (128, 128, 0)
    assert (dc.num_mel_bins, dc.hidden, dc.num_layers, dc.frame_length_ms, dc.frame_shift_ms, dc.subsample, dc.per_layer_states) == \
           (80, 64, 2, 25.0, 10.0, 1, 0)
    setattr(dc, field, value)
    assert match in _create_error(ccfg, dc)


@pytest.mark.parametrize("width, match", [(96, "multiple of 64"), (1088, "at most 1024")])
def test_the_library_refuses_widths_the_recurrent_kernel_does_not_take(width, match):
    from s3prl_amd import _lib
    from s3prl_amd.synth import named_config

    cfg = named_config("tiny_decoar")
    ccfg, dc = _lib.make_config(cfg, "fp32"), _lib.make_decoar_config(cfg)
    dc.hidden = width
    ccfg.conv_dim = ccfg.embed_dim = 2 * width
    assert match in _create_error(ccfg, dc)


@pytest.mark.parametrize("dtype", ["bf16", "fp16", "fp16x2", "fp32x3"])
def test_non_fp32_modes_are_refused_with_the_mode_named(dtype):
    from s3prl_amd import _lib
    from s3prl_amd.encoder import HipEncoder
    from s3prl_amd.synth import named_config, synth_weights

    cfg = named_config("tiny_decoar")
    err = _create_error(_lib.make_config(cfg, dtype), _lib.make_decoar_config(cfg))
    assert "fp32 only" in err and dtype in err
    with pytest.raises(ValueError, match="fp32 only"):
        HipEncoder(cfg, synth_weights(cfg, 0), dtype=dtype)


def test_the_decoar_block_is_required_for_the_family_and_refused_elsewhere():
    from s3prl_amd import _lib
    from s3prl_amd.synth import named_config

    cfg = named_config("tiny_decoar")
    lib = _lib.load()
    h = C.c_void_p()
    tensors = (_lib.S3Tensor * 1)()
    ccfg = _lib.make_config(cfg, "fp32")
    assert lib.s3enc_create(C.byref(ccfg), tensors, 0, 0, C.byref(h)) != 0 and b"s3enc_create_decoar" in lib.s3enc_last_error()
    assert lib.s3enc_create_ex(C.byref(ccfg), None, tensors, 0, 0, C.byref(h)) != 0 and b"s3enc_create_decoar" in lib.s3enc_last_error()
    apc = _lib.make_apc_config(named_config("tiny_apc"))
    assert lib.s3enc_create_apc(C.byref(ccfg), C.byref(apc), tensors, 0, 0, C.byref(h)) != 0 and b"s3enc_create_decoar" in lib.s3enc_last_error()
    mj = _lib.make_mockingjay_config(named_config("tiny_mockingjay"))
    assert lib.s3enc_create_mockingjay(C.byref(ccfg), C.byref(mj), tensors, 0, 0, C.byref(h)) != 0
    assert b"s3enc_create_decoar" in lib.s3enc_last_error()
    assert "null argument" in _create_error(ccfg, None)
    for other in ("tiny_hubert", "tiny_apc", "tiny_mockingjay"):
        assert "S3ENC_DECOAR only" in _create_error(_lib.make_config(named_config(other), "fp32"), _lib.make_decoar_config(cfg))
    assert lib.s3enc_version() == _lib.ABI_VERSION == 8  # every addition is a new symbol


def test_decoar_block_follows_the_header(tmp_path):
    """s3enc_decoar_config: field order against the header text, size and offsets against the header compiled as C; s3enc_config
    stays what it was."""
    import subprocess

    from s3prl_amd import _lib

    header = open(os.path.join(ROOT, "include", "s3enc.h")).read()
    body = header[header.index("typedef struct s3enc_decoar_config {"):header.index("} s3enc_decoar_config;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = re.findall(r"(?:int32_t|float)\s+([a-z0-9_]+)(?:\[[^\]]*\])?;", body)
    assert names == [n for n, _ in _lib.S3DecoarConfig._fields_] and names[0] == "num_mel_bins" and names[-1] == "per_layer_states"
    assert _lib.FAMILY["decoar"] == 9 and "S3ENC_DECOAR = 9" in header and "#define S3ENC_VERSION 8" in header
    assert [n for n, _ in _lib.S3Config._fields_][-1] == "dw_kernel"
    for sym in ("s3enc_create_decoar", "s3enc_op_lstm_bidir", "s3enc_pack_lstm_bidir_whh"):
        assert re.search(r"\bint " + sym + r"\(", header), sym
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "s3enc.h"\n'
                   'int main(void){printf("%zu %zu %zu %zu\\n", sizeof(s3enc_decoar_config), offsetof(s3enc_decoar_config, frame_length_ms), '
                   'offsetof(s3enc_decoar_config, subsample), offsetof(s3enc_decoar_config, per_layer_states));return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    W = _lib.S3DecoarConfig
    assert got == [C.sizeof(W), W.frame_length_ms.offset, W.subsample.offset, W.per_layer_states.offset]


def test_hub_names_have_the_reference_signatures():
    import s3prl_amd.hub as amd

    ref = json.load(open(os.path.join(ROOT, "tests", "golden", "decoar", "reference_hub_decoar.json")))
    everything = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_hub.json")))["options"]
    assert ref["downsample_rate"] == 160
    checked = []
    for fam in ("decoar", "decoar_layers"):
        for name, params in ref["hubconfs"][fam]:
            assert name in everything and name in amd.options(), name
            ours = inspect.signature(getattr(amd, name))
            assert [list(p) for p in params] == [[k, v.kind.name, repr(v.default)] for k, v in ours.parameters.items()], name
            checked.append(name)
    assert sorted(checked) == ["decoar", "decoar_custom", "decoar_layers", "decoar_layers_custom", "decoar_layers_local",
                               "decoar_layers_url", "decoar_local", "decoar_url"]
    reg = set(amd.options(only_registered_ckpt=True))
    assert {"decoar", "decoar_layers"} <= reg and not {"decoar_local", "decoar_url", "decoar_custom", "decoar_layers_custom"} & reg
