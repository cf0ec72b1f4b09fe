"""wav2vec / vq-wav2vec without a GPU: the float64 restatement of tests/wav2vec_ref.py against every reference-generated fixture
(states, codewords, code ids), checkpoint round trips of the converted and the fairseq layout, the refusals by name (Python
and s3enc_create), the hub names and signatures, and the frame arithmetic."""

import ctypes as C
import inspect
import json
import os
import re

import numpy as np
import pytest

from oracle import encoder_oracle as O

import wav2vec_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["wav2vec_tiny_pad", "wav2vec_tiny_eq", "wav2vec_tiny_t1", "wav2vec_tiny_zeropad_noaffine", "vq_gumbel_tiny_pad",
         "vq_kmeans_tiny_pad", "wav2vec_large_pseudo"]
FIXTURES = ["wav2vec/" + n for n in NAMES]
REF_PIN = 1e-6  # the pin of tests/conformer_ref.py: a float64 restatement against the reference's fp32 outputs


def _raw(name):
    return np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"))


@pytest.mark.parametrize("name", FIXTURES)
def test_float64_restatement_matches_the_reference(name, golden_loader):
    meta, cfg, weights, wavs, hs, norms = golden_loader(name)
    assert len(hs) == cfg.num_hidden_states == len(cfg.agg_layers) + 1
    out = R.forward(cfg, weights, wavs)
    ts, cs = meta["t_stride"], meta["c_stride"]
    for l, h in enumerate(out["hidden_states"]):
        assert list(h.shape) == meta["shape"]
        assert O.rel_err(h[:, ::ts, ::cs], hs[l]) <= REF_PIN, (name, l)
        assert abs(np.linalg.norm(h) - norms[l]) / norms[l] <= REF_PIN
    z = _raw(name)
    if cfg.vq_type != "none":
        assert meta["margin"] >= 1e-4 and out["margin"] >= 0.5e-4  # no decision of the fixture is a near-tie
        assert z["codeids"].dtype == np.int64 and np.array_equal(out["codeids"], z["codeids"])  # every frame, every group
        assert O.rel_err(out["codewords"][:, ::ts, ::cs], z["codewords"]) <= REF_PIN
    else:
        assert "codeids" not in z.files and out["codeids"] is None


@pytest.mark.parametrize("cfg_name", ["tiny_wav2vec", "tiny_wav2vec_zeropad_noaffine", "tiny_vq_wav2vec_gumbel", "tiny_vq_wav2vec_kmeans"])
@pytest.mark.parametrize("layout", ["converted", "fairseq", "fairseq_args"])
def test_checkpoint_round_trip(tmp_path, cfg_name, layout):
    import argparse

    import torch

    from s3prl_amd.ckpt import load_checkpoint, save_checkpoint
    from s3prl_amd.synth import named_config, synth_weights

    cfg = named_config(cfg_name)
    weights = synth_weights(cfg, 5)
    path = str(tmp_path / "c.pt")
    save_checkpoint(path, cfg, weights)
    state = torch.load(path, map_location="cpu", weights_only=False)
    assert set(state) == {"task_cfg", "model_cfg", "model_weight"}  # wav2vec/convert.py:13-17
    # tensors the inference path never reads are accepted and dropped
    state["model_weight"]["wav2vec_predictions.project_to_steps.weight"] = torch.zeros(4, 4, 1, 12)
    state["model_weight"]["project_features.conv_layers.0.1.weight"] = torch.zeros(4, 4, 2)
    if layout == "fairseq":
        state = {"cfg": {"task": state["task_cfg"], "model": state["model_cfg"]}, "model": state["model_weight"]}
    elif layout == "fairseq_args":
        state = {"args": argparse.Namespace(**state["model_cfg"]), "model": state["model_weight"]}
    torch.save(state, path)
    cfg2, back = load_checkpoint(path, "wav2vec")
    assert cfg2 == cfg
    assert set(back) == set(weights) and all(np.array_equal(back[k], weights[k]) for k in weights)


def test_missing_keys_and_tensors_are_named(tmp_path):
    import torch

    from s3prl_amd.ckpt import load_checkpoint, save_checkpoint
    from s3prl_amd.synth import named_config, synth_weights

    cfg = named_config("tiny_vq_wav2vec_kmeans")
    path = str(tmp_path / "c.pt")
    save_checkpoint(path, cfg, synth_weights(cfg, 0))
    state = torch.load(path, map_location="cpu", weights_only=False)
    del state["model_weight"]["vector_quantizer.embedding"]
    torch.save(state, path)
    with pytest.raises(ValueError, match="vector_quantizer.embedding"):
        load_checkpoint(path, "wav2vec")
    torch.save({"model_cfg": {}, "model_weight": {}}, path)
    with pytest.raises(ValueError, match="task_cfg"):
        load_checkpoint(path, "wav2vec")


def test_reference_defaults_are_the_released_large_shape():
    from s3prl_amd.config import config_from_wav2vec
    from s3prl_amd.synth import named_config

    cfg = config_from_wav2vec({})  # Wav2VecConfig's defaults carry one more 1x1 extractor layer than the released model
    assert len(cfg.conv_layers) == 8 and [k for _, k, _ in cfg.agg_layers] == list(range(2, 14))
    assert cfg.skip_connections_agg and cfg.log_compression and cfg.residual_scale == 0.5 and cfg.vq_type == "none"
    large = named_config("wav2vec_large")
    assert [(k, s) for _, k, s in large.conv_layers] == [(10, 5), (8, 4), (4, 2), (4, 2), (4, 2), (1, 1), (1, 1)]
    assert large.conv_lengths(160000) == [31999, 7998, 3998, 1998, 998, 998, 998] and large.num_hidden_states == 13

    class Choice:
        name = "kmeans"

    assert config_from_wav2vec(dict(vq_type=Choice(), vq_vars=16)).vq_type == "kmeans"


@pytest.mark.parametrize("n, T", [(160000, 998), (465, 1), (4000, 23), (464, 0)])
def test_frame_arithmetic(n, T):
    from s3prl_amd.synth import named_config

    for name in ("tiny_wav2vec", "wav2vec_large"):
        cfg = named_config(name)
        assert cfg.num_frames(n) == T and cfg.num_output_frames(n) == T
        assert cfg.valid_frames(n, 160000) == T and cfg.downsample_rate == 160


def _w2v(**kw):
    d = dict(conv_feature_layers="[(64, 10, 5), (64, 8, 4)]", conv_aggregator_layers="[(64, 2, 1), (64, 3, 1)]")
    d.update(kw)
    return d


@pytest.mark.parametrize("kw, match", [
    (dict(aggregator="gru"), "aggregator='gru'"),
    (dict(activation="gelu"), "activation='gelu'"),
    (dict(skip_connections_feat=True), "skip_connections_feat"),
    (dict(conv_aggregator_layers="[(64, 2, 1), (128, 3, 1)]"), "unequal widths"),
    (dict(conv_feature_layers="[(32, 10, 5), (64, 8, 4)]"), "unequal widths"),
    (dict(conv_aggregator_layers="[(64, 2, 1), (64, 3, 2)]"), "strides other than 1"),
    (dict(vq_type="gumbel", vq_dim=32), "vq_dim"),
    (dict(vq_type="lloyd"), "vq_type"),
])
def test_config_refusals(kw, match):
    from s3prl_amd.config import config_from_wav2vec

    with pytest.raises(ValueError, match=re.escape(match)):
        config_from_wav2vec(_w2v(**kw))


def _create_error(ccfg, w2v):
    from s3prl_amd import _lib

    lib = _lib.load()
    h = C.c_void_p()
    tensors = (_lib.S3Tensor * 1)()
    assert lib.s3enc_create_ex(C.byref(ccfg), C.byref(w2v) if w2v is not None else None, tensors, 0, 0, C.byref(h)) != 0
    return lib.s3enc_last_error().decode()


@pytest.mark.parametrize("field, value, match", [
    ("w2v_aggregator", 1, 'aggregator="gru"'),
    ("w2v_activation", 1, "activation"),
    ("w2v_skip_feat", 1, "skip_connections_feat"),
    ("agg_dim", 128, "unequal widths"),
    ("agg_stride", 2, "strides other than 1"),
    ("vq_type", 3, "vq_type"),
])
def test_the_library_refuses_by_name(field, value, match):
    """s3enc_create_ex checks the configuration before it looks for a device: the refusals are the same without a GPU."""
    from s3prl_amd import _lib
    from s3prl_amd.synth import named_config

    cfg = named_config("tiny_wav2vec")
    ccfg, w2v = _lib.make_config(cfg, "fp32"), _lib.make_wav2vec_config(cfg)
    assert ccfg.family == 5 and w2v.n_agg == 4 and list(w2v.agg_kernel)[:4] == [2, 3, 4, 5] and ccfg.encoder_layers == 4
    if field in ("agg_dim", "agg_stride"):
        getattr(w2v, field)[1] = value
    else:
        setattr(w2v, field, value)
    assert match in _create_error(ccfg, w2v)


def test_the_wav2vec_block_is_required_for_the_family_and_refused_elsewhere():
    from s3prl_amd import _lib
    from s3prl_amd.synth import named_config

    cfg = named_config("tiny_wav2vec")
    assert "s3enc_create_ex" in _create_error(_lib.make_config(cfg, "fp32"), None)
    lib = _lib.load()
    h = C.c_void_p()
    tensors = (_lib.S3Tensor * 1)()
    ccfg = _lib.make_config(cfg, "fp32")
    assert lib.s3enc_create(C.byref(ccfg), tensors, 0, 0, C.byref(h)) != 0 and b"s3enc_create_ex" in lib.s3enc_last_error()
    assert "S3ENC_WAV2VEC only" in _create_error(_lib.make_config(named_config("tiny_hubert"), "fp32"), _lib.make_wav2vec_config(cfg))


@pytest.mark.parametrize("dtype", ["bf16", "fp16", "fp16x2", "fp32x3"])
def test_non_fp32_modes_are_refused_with_the_mode_named(dtype):
    from s3prl_amd import _lib
    from s3prl_amd.synth import named_config

    cfg = named_config("tiny_vq_wav2vec_gumbel")
    err = _create_error(_lib.make_config(cfg, dtype), _lib.make_wav2vec_config(cfg))
    assert "fp32 only" in err and dtype in err


def test_wav2vec_block_follows_the_header(tmp_path):
    """s3enc_wav2vec_config: field order against the header text, size and offsets against the header compiled as C; s3enc_config
    and the ABI version stay what they were."""
    import subprocess

    from s3prl_amd import _lib

    header = open(os.path.join(ROOT, "include", "s3enc.h")).read()
    body = header[header.index("typedef struct s3enc_wav2vec_config {"):header.index("} s3enc_wav2vec_config;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = re.findall(r"(?:int32_t|float)\s+([a-z0-9_]+)(?:\[[^\]]*\])?;", body)
    assert names == [n for n, _ in _lib.S3Wav2vecConfig._fields_] and names[0] == "n_agg" and names[-1] == "combine_groups"
    assert _lib.FAMILY["wav2vec"] == 5 and "S3ENC_WAV2VEC = 5" in header
    assert [n for n, _ in _lib.S3Config._fields_][-1] == "dw_kernel" and _lib.ABI_VERSION == 8
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "s3enc.h"\n'
                   'int main(void){printf("%zu %zu %zu %zu\\n", sizeof(s3enc_wav2vec_config), offsetof(s3enc_wav2vec_config, agg_stride), '
                   'offsetof(s3enc_wav2vec_config, residual_scale), offsetof(s3enc_wav2vec_config, combine_groups));return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    W = _lib.S3Wav2vecConfig
    assert got == [C.sizeof(W), W.agg_stride.offset, W.residual_scale.offset, W.combine_groups.offset]


def test_hub_names_have_the_reference_signatures():
    import s3prl_amd.hub as amd

    ref = json.load(open(os.path.join(ROOT, "tests", "golden", "wav2vec", "reference_hub_wav2vec.json")))
    everything = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_hub.json")))["options"]
    checked = []
    for family, entries in ref["hubconfs"].items():
        for name, params in entries:
            if family == "vq_wav2vec" and name.startswith("wav2vec2_"):
                continue  # the reference's vq_wav2vec/hubconf.py misnames its local / url aliases: wav2vec 2.0 owns those names
            assert name in everything and name in amd.options(), name
            ours = inspect.signature(getattr(amd, name))
            assert [list(p) for p in params] == [[k, v.kind.name, repr(v.default)] for k, v in ours.parameters.items()], name
            checked.append(name)
    assert sorted(checked) == sorted(["wav2vec", "wav2vec_custom", "wav2vec_local", "wav2vec_url", "wav2vec_large", "vq_wav2vec",
                                      "vq_wav2vec_custom", "vq_wav2vec_gumbel", "vq_wav2vec_kmeans"])
    assert not hasattr(amd, "vq_wav2vec_kmeans_roberta")
    reg = set(amd.options(only_registered_ckpt=True))
    assert {"wav2vec", "wav2vec_large", "vq_wav2vec", "vq_wav2vec_gumbel", "vq_wav2vec_kmeans"} <= reg
    assert amd.wav2vec_large.url.endswith("converted_ckpts/resolve/main/wav2vec_large.pt")
    assert amd.vq_wav2vec_kmeans.legacy_url.endswith("fairseq/wav2vec/vq-wav2vec_kmeans.pt")


def test_expert_loads_a_checkpoint_and_reports_the_reference_geometry(tmp_path):
    """Without a GPU: construction, the stride, the state count and sizes; the forward itself needs the MI355X."""
    import torch

    import s3prl_amd.hub as amd
    from s3prl_amd.ckpt import save_checkpoint
    from s3prl_amd.synth import named_config, synth_weights

    cfg = named_config("tiny_vq_wav2vec_gumbel")
    path = str(tmp_path / "c.pt")
    save_checkpoint(path, cfg, synth_weights(cfg, 0))
    expert = amd.vq_wav2vec_custom(ckpt=path)
    assert expert.get_downsample_rates("hidden_states") == 160
    assert expert.num_layers == 5 and expert.hidden_sizes == [64] * 5
    assert expert._states_info(5) == ("self.model.feature_extractor", "self.model.feature_aggregator.conv_layers[1]",
                                      "self.model.feature_aggregator.conv_layers[2]",
                                      "self.model.feature_aggregator.conv_layers[3]", "self.model.feature_aggregator")
    wav = torch.zeros(4000, requires_grad=True)
    with pytest.raises(RuntimeError, match="inference-only"):
        expert([wav])
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            expert([torch.zeros(4000)])
