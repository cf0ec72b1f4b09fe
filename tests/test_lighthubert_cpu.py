"""LightHuBERT without a GPU: the float64 restatement (tests/lighthubert_ref.py) against the fixtures the reference's own expert
produced (tests/golden/lighthubert/, tools/make_lighthubert_goldens.py), the checkpoint reader's cut of the supernet against the
restatement's, the state list's padded rows, the hub names and signatures, and every refusal by name."""

import ctypes as C
import dataclasses
import inspect
import json
import os

import numpy as np
import pytest

import lighthubert_ref as R
from conftest import GOLDEN_DIR
from oracle import encoder_oracle as O

FIXTURES = ("base_ragged", "base_equal", "base_two_tiles", "small_ragged", "small_one_frame", "stage1", "base_pl")
LH_DIR = os.path.join(GOLDEN_DIR, "lighthubert")
RESTATEMENT_TOL = 1e-5  # tests/test_conformer_cpu.py's band for a float64 restatement against the reference's fp32 run, all rows


@pytest.fixture(scope="module")
def restated(golden_loader):
    cache = {}

    def get(name):
        if name not in cache:
            meta, cfg, weights, wavs, hs, norms = golden_loader(f"lighthubert/{name}")
            cache[name] = R.forward(cfg, weights, wavs)
        return cache[name]

    return get


@pytest.mark.parametrize("name", FIXTURES)
def test_restatement_matches_the_reference_fixture_on_all_rows(name, golden_loader, restated):
    meta, cfg, weights, wavs, hs, norms = golden_loader(f"lighthubert/{name}")
    ref = restated(name)
    ts, cs = meta["t_stride"], meta["c_stride"]
    assert len(ref) == len(hs) == 13 == cfg.num_hidden_states and list(ref[0].shape) == meta["shape"]
    errs = [O.rel_err(ref[l][:, ::ts, ::cs], hs[l]) for l in range(13)]
    nerr = [abs(np.linalg.norm(ref[l]) - norms[l]) / norms[l] for l in range(13)]
    print(f"LIGHTHUBERT restatement {name}: max rel-err {max(errs):.2e}, max norm err {max(nerr):.2e}")
    assert max(errs) < RESTATEMENT_TOL and max(nerr) < RESTATEMENT_TOL, (errs, nerr)


@pytest.mark.parametrize("name", FIXTURES)
def test_state_0_pad_rows_are_zero_and_the_layer_states_are_not(name, golden_loader, restated):
    meta, cfg, weights, wavs, hs, norms = golden_loader(f"lighthubert/{name}")
    valid = R.valid_frames(cfg, meta["lengths"])
    assert valid == meta["valid"]
    ref, ts = restated(name), meta["t_stride"]
    for b, v in enumerate(valid):
        first = -(-v // ts)  # first stored frame at or behind the valid count
        assert not ref[0][b, v:].any() and not hs[0][b, first:].any(), "state 0: padded frames exactly zero"
        assert ref[0][b, :v].all(axis=1).any()
        if v < ref[0].shape[1]:
            for l in range(1, 13):
                assert np.abs(ref[l][b, v:]).min(axis=1).max() > 0 and np.linalg.norm(hs[l][b, first:]) > 0, f"state {l}: pad rows are the reference's values"
    if name != "base_equal":
        assert min(valid) < ref[0].shape[1]


@pytest.mark.parametrize("config", ("lighthubert_base", "lighthubert_small", "lighthubert_stage1", "small_groupnorm_bias"))
def test_the_reader_cuts_the_supernet_as_the_restatement_does(config, tmp_path):
    """Bit for bit, through a written checkpoint; and only the subnet is returned."""
    from s3prl_amd.ckpt import load_checkpoint, save_checkpoint
    from s3prl_amd.config import config_from_lighthubert
    from s3prl_amd.synth import named_config, synth_weights

    if config == "small_groupnorm_bias":  # what a checkpoint's own config may ask of the extractor
        cfg = config_from_lighthubert(dict(_name="hubert_pruner", pruner_supernet="lighthubert_small.yaml", extractor_mode="default", conv_bias=True))
    else:
        cfg = named_config(config)
    sd = synth_weights(cfg, 11)
    g = sd["encoder.pos_conv.0.weight_g"]
    assert g.shape == (1, 1, 128) and g.std() > 0.05, "weight_g is not constant, so the order of fold and cut matters"
    path = str(tmp_path / "lh.pt")
    save_checkpoint(path, cfg, sd)
    cfg2, got = load_checkpoint(path, "lighthubert")
    assert cfg2.to_dict() == cfg.to_dict()
    want = R.subnet_weights(cfg, sd)
    assert set(got) == set(want) and "mask_emb" not in got and not any(k.startswith("layer_pred_heads") for k in got)
    for k in want:
        assert got[k].dtype == np.float32 and np.array_equal(got[k], want[k].astype(np.float32)), k
    E = cfg.encoder_embed_dim
    assert got["encoder.pos_conv.0.weight"].shape == (E, E // 16, 128) and got["encoder.layers.3.fc1.weight"].shape == (4 * E, E)
    if E < 768:  # fc1 keeps the leading rows of each 768-row block, not the leading 4 E rows
        assert np.array_equal(got["encoder.layers.3.fc1.weight"][E], sd["encoder.layers.3.fc1.weight"][768, :E])
        wrong = R.subnet_weights(cfg, sd, fold_before_slice=False)["encoder.pos_conv.0.weight"]
        rel = np.linalg.norm(wrong - want["encoder.pos_conv.0.weight"]) / np.linalg.norm(want["encoder.pos_conv.0.weight"])
        assert rel > 0.05 and not np.array_equal(wrong.astype(np.float32), got["encoder.pos_conv.0.weight"]), rel


def test_the_subnet_is_resolved_as_the_expert_does():
    from s3prl_amd.config import config_from_lighthubert

    base = dict(_name="hubert_pruner", pruner_supernet="config/lighthubert_base.yaml")
    for model_cfg, (E, H, F) in ((base, (640, 10, 2560)), (dict(base, pruner_supernet="LightHuBERT_Small.YAML"), (384, 6, 1536)),
                                 (dict(_name="student_hubert"), (768, 12, 3072)),
                                 (dict(_name="student_hubert", supernet_type="small"), (512, 8, 2048))):
        cfg = config_from_lighthubert(model_cfg)
        assert (cfg.encoder_embed_dim, cfg.encoder_attention_heads, cfg.encoder_ffn_embed_dim, cfg.encoder_layers) == (E, H, F, 12)
        assert cfg.normalize and cfg.extractor_mode == "layer_norm" and not cfg.conv_bias and cfg.num_hidden_states == 13
        assert cfg.downsample_rate == 320
    with pytest.raises(ValueError, match="'hubert_pruner' or 'student_hubert'"):
        config_from_lighthubert(dict(_name="hubert"))


def test_hub_names_and_signatures_equal_the_reference(tmp_path):
    import s3prl_amd.hub as amd

    with open(os.path.join(LH_DIR, "reference_hub_lighthubert.json")) as f:
        ref = json.load(f)
    entries = ref["hubconfs"]["lighthubert"]
    assert sorted(n for n, _ in entries) == ["lighthubert", "lighthubert_base", "lighthubert_local", "lighthubert_small",
                                             "lighthubert_stage1", "lighthubert_url"]
    for name, params in entries:
        ours = inspect.signature(getattr(amd, name))
        assert [list(p) for p in params] == [[k, v.kind.name, repr(v.default)] for k, v in ours.parameters.items()], (name, str(ours))
        assert name in amd.options()
    reg = set(amd.options(only_registered_ckpt=True))
    for name, url in ref["urls"].items():
        assert getattr(amd, name).url == url and name in reg
    assert "lighthubert" in reg and "lighthubert_local" not in reg
    with pytest.raises(AssertionError):
        amd.lighthubert_local(str(tmp_path / "absent.pt"))


def _create_message(cfg, dtype="fp32"):
    """s3enc_create on a configuration with no tensors: the refusal of the configuration itself comes first (no GPU is touched)."""
    from s3prl_amd import _lib

    lib = _lib.load()
    ccfg = _lib.make_config(cfg, "fp32")
    ccfg.compute_dtype = _lib.DTYPES[dtype]
    h = C.c_void_p()
    tensors = (_lib.S3Tensor * 1)()
    rc = lib.s3enc_create(C.byref(ccfg), tensors, 0, 0, C.byref(h))
    return rc, lib.s3enc_last_error().decode()


@pytest.mark.parametrize("dtype", ("bf16", "fp16", "fp32x3", "fp16x2"))
def test_every_operand_mode_but_fp32_is_refused_by_name(dtype):
    from s3prl_amd import _lib
    from s3prl_amd.synth import named_config

    for name in ("lighthubert_base", "lighthubert_stage1"):
        cfg = named_config(name)
        with pytest.raises(_lib.S3EncError, match=f"LightHuBERT is built for compute dtype fp32 only; {dtype} is not built"):
            _lib.make_config(cfg, dtype)
        rc, msg = _create_message(cfg, dtype)
        assert rc != 0 and "fp32 only" in msg and dtype in msg, msg
    # the group widths themselves, whatever the family: a HuBERT configuration at 640 / 16 and 384 / 16
    for D in (640, 384):
        cfg = dataclasses.replace(named_config("hubert_base"), encoder_embed_dim=D, encoder_attention_heads=D // 64)
        cfg.validate()
        with pytest.raises(_lib.S3EncError, match=f"group width {D // 16} is built for compute dtype fp32 only; {dtype} is not built"):
            _lib.make_config(cfg, dtype)
        rc, msg = _create_message(cfg, dtype)
        assert rc != 0 and f"the positional conv at group width {D // 16} is built for compute dtype fp32 only; {dtype} is not built" in msg, msg


def test_the_other_refusals_are_raised_by_name():
    from s3prl_amd import _lib
    from s3prl_amd.config import check_lighthubert_subnet, config_from_lighthubert, lighthubert_subnet
    from s3prl_amd.synth import named_config

    base = dict(_name="hubert_pruner", pruner_supernet="lighthubert_base.yaml")
    with pytest.raises(ValueError, match="layer_norm_first=True is not built"):
        config_from_lighthubert(dict(base, layer_norm_first=True))
    with pytest.raises(ValueError, match="pos_conv_depth > 1 is not built"):
        config_from_lighthubert(dict(base, pos_conv_depth=5))
    # the library repeats both
    cfg = named_config("lighthubert_base")
    for field, value, want in (("layer_norm_first", 1, "LightHuBERT with layer_norm_first is not built"),
                               ("pos_conv_depth", 5, "LightHuBERT with pos_conv_depth > 1 is not built")):
        lib = _lib.load()
        ccfg = _lib.make_config(cfg, "fp32")
        setattr(ccfg, field, value)
        h = C.c_void_p()
        assert lib.s3enc_create(C.byref(ccfg), (_lib.S3Tensor * 1)(), 0, 0, C.byref(h)) != 0
        assert want in lib.s3enc_last_error().decode(), lib.s3enc_last_error()
    # subnets: non-uniform per-layer widths, atten_dim != embed_dim, fewer layers, a sliding window
    good = lighthubert_subnet("hubert_pruner", "base")
    check_lighthubert_subnet(good)
    for key, value in (("atten_dim", [640] * 11 + [512]), ("ffn_embed", [2560] * 11 + [2240]), ("heads_num", [10] * 11 + [8])):
        with pytest.raises(ValueError, match=f"non-uniform {key} is not built"):
            config_from_lighthubert(base, dict(good, **{key: value}))
    with pytest.raises(ValueError, match="atten_dim != embed_dim is not built"):
        config_from_lighthubert(base, dict(good, atten_dim=[512] * 12, heads_num=[8] * 12))
    with pytest.raises(ValueError, match="11 layers is not built"):
        config_from_lighthubert(base, dict(good, layer_num=11))
    with pytest.raises(ValueError, match="sliding-window attention"):
        config_from_lighthubert(base, dict(good, slide_wsz=["global"] * 11 + [32]))
    # feature_selection: the reference's expert has no such argument and one list
    from s3prl_amd.upstream.lighthubert.expert import UpstreamExpert

    with pytest.raises(ValueError, match="feature_selection='fairseq_layers' is not defined for LightHuBERT"):
        UpstreamExpert("unused.pt", feature_selection="fairseq_layers")
    header = open(os.path.join(os.path.dirname(GOLDEN_DIR), "..", "include", "s3enc.h")).read()
    assert "S3ENC_LIGHTHUBERT = 15" in header and "#define S3ENC_VERSION 8" in header


def test_fixture_sizes_are_under_the_limit():
    files = sorted(os.listdir(LH_DIR))
    assert [f for f in files if f.endswith(".npz")] == sorted(f"{n}.npz" for n in FIXTURES) and "reference_hub_lighthubert.json" in files
    for f in files:
        assert os.path.getsize(os.path.join(LH_DIR, f)) < 256 * 1024, f
