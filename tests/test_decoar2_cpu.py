"""DeCoAR 2.0 without a GPU: the float64 restatement (tests/decoar2_ref.py) against the fixtures the reference's own expert produced
(tests/golden/decoar2/, tests/golden/make_golden_decoar2.py) on all stored rows, padded ones included; the checkpoint reader (the
reference's file layout, extra tensors ignored, a missing one named); the configuration rules and every refusal with its message; the
hub names, signatures and cache path; the frame rules."""

import ctypes as C
import dataclasses
import inspect
import json
import os

import numpy as np
import pytest

import decoar2_ref as R
from conftest import GOLDEN_DIR
from oracle import encoder_oracle as O

FIXTURES = ("tiny_ragged_odd", "tiny_ragged_even", "tiny_equal", "tiny_t1", "tiny_two_tiles", "tiny_d192", "pseudo")
D2_DIR = os.path.join(GOLDEN_DIR, "decoar2")
# tests/test_lighthubert_cpu.py's and tests/test_conformer_cpu.py's band for a float64 restatement against the reference's fp32 run, all
# rows.  The one state it does not fit is named below: a CMVN over TWO frames divides by a standard deviation that fp32 log-mels of
# magnitude 10 give to 1e-6 relative, and every row of that utterance carries it (the generator's fp32 proxy bound, a quarter of the GPU
# tests' FP32_TOL, is what the fixture was admitted under and what holds there)
RESTATEMENT_TOL = 1e-5
TWO_FRAME_TOL = 0.25 * 1e-4


@pytest.fixture(scope="module")
def restated(golden_loader):
    cache = {}

    def get(name):
        if name not in cache:
            meta, cfg, weights, wavs, hs, norms = golden_loader(f"decoar2/{name}")
            cache[name] = R.forward(cfg, weights, wavs)
        return cache[name]

    return get


@pytest.mark.parametrize("name", FIXTURES)
def test_restatement_matches_the_reference_fixture_on_all_rows(name, golden_loader, restated):
    meta, cfg, weights, wavs, hs, norms = golden_loader(f"decoar2/{name}")
    ref = restated(name)
    ts, cs = meta["t_stride"], meta["c_stride"]
    NS = cfg.encoder_layers + 1
    assert len(ref) == len(hs) == NS == cfg.num_hidden_states == meta["n_states"] and list(ref[0].shape) == meta["shape"]
    assert meta["valid"] == [R.num_frames(n) for n in meta["lengths"]] == [cfg.num_frames(n) for n in meta["lengths"]]
    assert meta["fbank_frames"] == [R.fbank_frames(n) for n in meta["lengths"]] and max(meta["ref_fp32_err"]) <= 8e-7
    tol = TWO_FRAME_TOL if min(meta["fbank_frames"]) == 2 else RESTATEMENT_TOL
    errs = [O.rel_err(ref[l][:, ::ts, ::cs], hs[l]) for l in range(NS)]
    nerr = [abs(np.linalg.norm(ref[l]) - norms[l]) / norms[l] for l in range(NS)]
    print(f"DECOAR2 restatement {name}: max rel-err {max(errs):.2e}, max norm err {max(nerr):.2e} (< {tol:.1e})")
    assert max(errs) < tol and max(nerr) < tol, (errs, nerr)


@pytest.mark.parametrize("name", FIXTURES)
def test_padded_rows_are_the_references_values(name, golden_loader, restated):
    """HuBERT's rule: post_extract_proj's rows at and after T_b are zeroed, the positional conv, the LayerNorm and the layers then
    write values there, and the states carry them — in state 0 as in the later ones."""
    meta, cfg, weights, wavs, hs, norms = golden_loader(f"decoar2/{name}")
    ref, ts, cs = restated(name), meta["t_stride"], meta["c_stride"]
    tol = TWO_FRAME_TOL if min(meta["fbank_frames"]) == 2 else RESTATEMENT_TOL
    seen = 0
    for b, v in enumerate(meta["valid"]):
        first = -(-v // ts)  # first stored frame at or behind the valid count
        if first >= hs[0].shape[1]:
            continue
        for l in range(len(hs)):
            want = hs[l][b, first:]
            assert np.linalg.norm(want) > 0, f"state {l}: padded rows are not zeros"
            assert O.rel_err(ref[l][b, ::ts, ::cs][first:], want) < tol, (name, l, b)
            seen += 1
    assert (seen > 0) == (len(set(meta["valid"])) > 1), "every ragged fixture stores padded rows"


def test_fixture_sizes_are_under_the_limit():
    files = sorted(os.listdir(D2_DIR))
    assert [f for f in files if f.endswith(".npz")] == sorted(f"{n}.npz" for n in FIXTURES) and "reference_hub_decoar2.json" in files
    for f in files:
        assert os.path.getsize(os.path.join(D2_DIR, f)) < 256 * 1024, f


@pytest.mark.parametrize("n, F", [(399, 0), (400, 1), (559, 1), (560, 2), (719, 2), (720, 3)])
def test_frame_rules(n, F):
    from s3prl_amd.synth import named_config

    cfg = named_config("decoar2")
    T = -(-F // 2)
    assert R.fbank_frames(n) == F == cfg.conv_lengths(n)[-1] and R.num_frames(n) == T == cfg.num_frames(n) == cfg.num_output_frames(n)
    assert cfg.valid_frames(n, 4000) == T and cfg.valid_frames(4000, 4000) == cfg.num_frames(4000) == 12
    assert cfg.downsample_rate == 320 and cfg.num_hidden_states == 13
    if F:
        assert R.frontend(np.random.default_rng(n).standard_normal(n)).shape == (T, 80)


def test_named_configs_and_synthetic_weights():
    from s3prl_amd import _lib
    from s3prl_amd.config import FAMILIES
    from s3prl_amd.synth import named_config, param_shapes, synth_weights

    assert "decoar2" in FAMILIES and _lib.FAMILY["decoar2"] == 16
    cfg = named_config("decoar2")
    assert (cfg.encoder_embed_dim, cfg.encoder_ffn_embed_dim, cfg.encoder_layers, cfg.encoder_attention_heads, cfg.conv_pos,
            cfg.conv_pos_groups, cfg.conv_layers, cfg.layer_norm_first) == (768, 3072, 12, 12, 128, 16, [(80, 400, 160)], False)
    tiny = named_config("tiny_decoar2")
    assert tiny.encoder_embed_dim == 128 and tiny.encoder_attention_heads == 2 and tiny.num_hidden_states == 3
    for c in (cfg, tiny):
        shapes = param_shapes(c)
        assert shapes["post_extract_proj.weight"] == (c.encoder_embed_dim, 80) and "layer_norm.weight" not in shapes
        assert not any(k.startswith("feature_extractor.") for k in shapes)
        for profile in ("synthetic", "pretrained_like"):
            w = synth_weights(c, 3, profile)
            assert set(w) == set(shapes) and all(w[k].shape == shapes[k] and w[k].dtype == np.float32 for k in shapes)
    ccfg = _lib.make_config(cfg, "fp32")
    assert (ccfg.family, ccfg.n_conv, ccfg.conv_dim, ccfg.conv_kernel[0], ccfg.conv_stride[0]) == (16, 1, 80, 400, 160)
    for dtype in ("fp32x3", "fp16x2", "fp16", "bf16"):  # every operand mode is served (profiles/decoar2_fp32.md)
        assert _lib.make_config(cfg, dtype).compute_dtype == _lib.DTYPES[dtype]


def test_the_reader_takes_the_widths_from_the_tensors(tmp_path):
    """The reference's file layout ``{"model": state_dict}``; tensors of the pre-training model the encoder does not own are ignored;
    a missing tensor it does own is an error by name."""
    import torch

    from s3prl_amd.ckpt import load_checkpoint, save_checkpoint
    from s3prl_amd.synth import named_config, synth_weights

    for name in ("tiny_decoar2", "tiny_decoar2_d192", "decoar2"):
        cfg = named_config(name)
        sd = synth_weights(cfg, 5)
        path = str(tmp_path / f"{name}.pt")
        extra = dict(sd, mask_emb=np.zeros(cfg.encoder_embed_dim, np.float32), **{"final_proj.weight": np.zeros((4, 4), np.float32)})
        save_checkpoint(path, cfg, extra)
        state = torch.load(path, map_location="cpu", weights_only=False)
        assert list(state) == ["model"] and set(state["model"]) == set(extra)
        assert tuple(state["model"]["encoder.pos_conv.0.weight_g"].shape) == (1, 1, cfg.conv_pos)
        cfg2, got = load_checkpoint(path, "decoar2")
        assert cfg2.to_dict() == cfg.to_dict() and cfg2.encoder_attention_heads == cfg.encoder_embed_dim // 64
        assert set(got) == set(sd) and all(np.array_equal(got[k], sd[k]) for k in sd)
    cfg = named_config("tiny_decoar2")
    sd = synth_weights(cfg, 5)
    for missing in ("encoder.layers.1.fc2.bias", "encoder.layer_norm.weight", "post_extract_proj.weight", "encoder.pos_conv.0.weight_v",
                    "encoder.pos_conv.0.weight_g"):
        path = str(tmp_path / "missing.pt")
        save_checkpoint(path, cfg, {k: v for k, v in sd.items() if k != missing})
        with pytest.raises(ValueError, match=f"missing parameter {missing.replace('.', '[.]')}"):
            load_checkpoint(path, "decoar2")
    torch.save({"weights": {}}, str(tmp_path / "bad.pt"))
    with pytest.raises(ValueError, match="required key: model is missing"):
        load_checkpoint(str(tmp_path / "bad.pt"), "decoar2")


def test_config_rules_and_refusals():
    from s3prl_amd.config import config_from_decoar2, decoar2_config
    from s3prl_amd.synth import named_config, param_shapes

    cfg = named_config("decoar2")
    shapes = {k: np.zeros(v, np.float32) for k, v in param_shapes(named_config("tiny_decoar2_d192")).items()}
    got = config_from_decoar2(shapes)
    assert (got.encoder_embed_dim, got.encoder_attention_heads, got.encoder_ffn_embed_dim, got.encoder_layers, got.conv_pos,
            got.conv_pos_groups) == (192, 3, 384, 2, 16, 4)
    with pytest.raises(ValueError, match="embed_dim must be a multiple of 64"):
        decoar2_config(embed_dim=160)
    with pytest.raises(ValueError, match="group width[)] must be 32, 48 or 64 [(]fp32: also 24 or 40[)], got 128 / 8"):
        decoar2_config(embed_dim=128, ffn_dim=256, layers=2, conv_pos_groups=8)
    with pytest.raises(ValueError, match="post_extract_proj reads 40 features"):
        config_from_decoar2(dict(shapes, **{"post_extract_proj.weight": np.zeros((192, 40), np.float32)}))
    for field, value, what in (("layer_norm_first", True, "decoar2 with layer_norm_first=True is not built"),
                               ("pos_conv_depth", 5, "decoar2 with pos_conv_depth > 1 is not built"),
                               ("layer_type", "conformer", "decoar2: only layer_type='transformer' exists in the reference"),
                               ("relative_position_embedding", True, "decoar2 takes none of the WavLM / DistilHuBERT options"),
                               ("pred_heads", 2, "decoar2 takes none of the WavLM / DistilHuBERT options"),
                               ("feature_layer_norm", False, "decoar2 takes none of the WavLM / DistilHuBERT options"),
                               ("normalize", True, "decoar2 has no conv extractor and no waveform normalisation"),
                               ("conv_layers", [(80, 400, 320)], "decoar2: conv_layers carries the front end's constants"),
                               ("encoder_attention_heads", 6, "embed_dim must be a multiple of 64 and heads embed_dim / 64")):
        with pytest.raises(ValueError, match=what):
            dataclasses.replace(cfg, **{field: value}).validate()


def _create_message(mutate):
    """s3enc_create on a configuration with no tensors: the refusal of the configuration itself comes first (no GPU is touched)."""
    from s3prl_amd import _lib
    from s3prl_amd.synth import named_config

    lib = _lib.load()
    ccfg = _lib.make_config(named_config("decoar2"), "fp32")
    mutate(ccfg)
    h = C.c_void_p(0xDEAD)
    rc = lib.s3enc_create(C.byref(ccfg), (_lib.S3Tensor * 1)(), 0, 0, C.byref(h))
    return rc, h.value, lib.s3enc_last_error().decode()


def test_the_library_repeats_the_refusals_by_name():
    def setter(field, value):
        return lambda c: setattr(c, field, value)

    def stride(c):
        c.conv_stride[0] = 320

    for mutate, what in ((setter("layer_norm_first", 1), "config: DeCoAR 2.0 with layer_norm_first is not built"),
                         (setter("pos_conv_depth", 5), "config: DeCoAR 2.0 with pos_conv_depth > 1 is not built"),
                         (setter("layer_type", 1), "config: DeCoAR 2.0 takes none of the Conformer / WavLM / DistilHuBERT options"),
                         (setter("rel_pos", 1), "config: DeCoAR 2.0 takes none of the Conformer / WavLM / DistilHuBERT options"),
                         (setter("pred_heads", 2), "config: pred_heads is a DistilHuBERT feature"),  # (the engine's own rule comes first)
                         (setter("no_feature_layer_norm", 1), "config: DeCoAR 2.0 takes none of the Conformer / WavLM / DistilHuBERT options"),
                         (setter("normalize", 1), "config: DeCoAR 2.0 has no conv extractor and no waveform normalisation"),
                         (setter("conv_dim", 40), "config: DeCoAR 2.0 carries its front end as n_conv = 1"),
                         (stride, "config: DeCoAR 2.0 carries its front end as n_conv = 1"),
                         (setter("heads", 10), "config: head_dim must be 64"),
                         (setter("conv_pos_groups", 8), "config: embed_dim/conv_pos_groups must be 32, 48 or 64 (fp32: also 24 or 40)"),
                         (setter("family", 17), "config: unknown family")):
        rc, handle, msg = _create_message(mutate)
        assert rc != 0 and handle is None and msg.startswith(what), msg
    # a whole configuration gets as far as the first tensor
    rc, handle, msg = _create_message(lambda c: None)
    assert rc != 0 and handle is None and "missing tensor" in msg or "no HIP device" in msg, msg
    header = open(os.path.join(os.path.dirname(GOLDEN_DIR), "..", "include", "s3enc.h")).read()
    assert "S3ENC_DECOAR2 = 16" in header and "#define S3ENC_VERSION 8" in header and "s3enc_op_fbank_batch" in header


def test_expert_surface_refusals():
    from s3prl_amd.upstream.decoar2.expert import UpstreamExpert

    with pytest.raises(ValueError, match="feature_selection='fairseq_layers' is not defined for DeCoAR 2.0"):
        UpstreamExpert("unused.pt", feature_selection="fairseq_layers")
    e = UpstreamExpert.__new__(UpstreamExpert)  # the layerdrop surface needs no checkpoint
    assert UpstreamExpert.layer_drop.fget(e) == 0.0
    UpstreamExpert.set_layer_drop(e, None)
    UpstreamExpert.set_layer_drop(e, 0.0)
    with pytest.raises(ValueError, match="layerdrop is a training-time option"):
        UpstreamExpert.set_layer_drop(e, 0.05)
    with pytest.raises(ValueError, match="layerdrop can only be float or None"):
        UpstreamExpert.set_layer_drop(e, 1)
    assert UpstreamExpert.get_downsample_rates(e, "hidden_states") == 320


def test_hub_names_signatures_and_cache_path(tmp_path, monkeypatch):
    import s3prl_amd.hub as amd
    from s3prl_amd import download

    with open(os.path.join(D2_DIR, "reference_hub_decoar2.json")) as f:
        ref = json.load(f)
    entries = ref["hubconfs"]["decoar2"]
    assert sorted(n for n, _ in entries) == ["decoar2", "decoar2_custom", "decoar2_local", "decoar2_url"] and ref["downsample_rate"] == 320
    for name, params in entries:
        ours = inspect.signature(getattr(amd, name))
        assert [list(p) for p in params] == [[k, v.kind.name, repr(v.default)] for k, v in ours.parameters.items()], (name, str(ours))
        assert name in amd.options()
    assert set(amd.options(only_registered_ckpt=True)) & {n for n, _ in entries} == {"decoar2"}
    with open(os.path.join(GOLDEN_DIR, "reference_hub.json")) as f:
        listed = json.load(f)
    assert {n for n, _ in entries} <= _names(listed), "the reference's hub lists the four names"
    with pytest.raises(AssertionError):
        amd.decoar2_local(str(tmp_path / "absent.pt"))
    # the released URL resolves to the reference's cache file: <dir>/<sha256(url)>.<basename>; a file placed there is what decoar2() reads
    from s3prl_amd.upstream.decoar2 import hubconf

    assert hubconf._RELEASED == ref["urls"]["decoar2"]
    def no_fetch(url, dst):
        raise AssertionError(f"a fetch of {url} was attempted")

    monkeypatch.setattr(download, "_fetch", no_fetch)
    old = download.get_dir()
    try:
        download.set_dir(tmp_path)
        path = download.cache_path(hubconf._RELEASED)
        assert path.parent == tmp_path and path.name.endswith(".checkpoint_decoar2.pt") and len(path.name.split(".")[0]) == 64
        path.write_bytes(b"not a checkpoint")
        assert download.urls_to_filepaths(hubconf._RELEASED) == str(path.resolve())
        with pytest.raises(Exception) as err:  # found in the cache, read by torch.load: nothing is fetched
            amd.decoar2()
        assert "cannot fetch" not in str(err.value)
    finally:
        download.set_dir(old)


def _names(listed):
    """every string of the hub record, whatever its nesting"""
    out = set()

    def walk(x):
        if isinstance(x, str):
            out.add(x)
        elif isinstance(x, dict):
            for k, v in x.items():
                out.add(k)
                walk(v)
        elif isinstance(x, (list, tuple)):
            for v in x:
                walk(v)

    walk(listed)
    return out
