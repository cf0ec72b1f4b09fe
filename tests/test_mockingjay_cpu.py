"""Mockingjay / TERA / AudioALBERT without a GPU: the float64 restatement of tests/mockingjay_ref.py against every
reference-generated fixture, its STFT against torch.stft in float64 (reflect edges, a short utterance inside a longer batch), the
mel filter bank against its closed form, the batch-dependent frame-count rule, chunk sizes against torch.chunk, configuration
parsing, checkpoint key mapping, the refusals by name (Python and s3enc_create_mockingjay), the configuration block against the
header, the op entries' argument checks and the hub names."""

import ctypes as C
import inspect
import json
import math
import os
import re

import numpy as np
import pytest

from oracle import encoder_oracle as O

import mockingjay_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NAMES = ["tiny_pad", "tiny_eq", "tiny_chunk", "tiny_chunk3", "tiny_eps", "tiny_albert", "tiny_kaldi", "tera_base_pseudo"]
FIXTURES = ["mockingjay/" + n for n in NAMES]
REF_PIN = 1e-6  # the project's restatement bound: a float64 restatement against the reference's fp32 outputs


def _live(h, counts, ts=1):
    return np.concatenate([np.asarray(h[b, :-(-n // ts)], np.float64).reshape(-1) for b, n in enumerate(counts)])


@pytest.fixture(scope="module")
def restated(golden_loader):
    cache = {}

    def get(name):
        if name not in cache:
            meta, cfg, weights, wavs, hs, norms = golden_loader(name)
            feats, counts = R.features(cfg, wavs)
            # the generator fed the reference these features ROUNDED TO fp32
            cache[name] = (R.model(cfg, weights, feats.astype(np.float32), counts), counts)
        return cache[name]

    return get


@pytest.mark.parametrize("name", FIXTURES)
def test_float64_restatement_matches_the_reference(name, golden_loader, restated):
    meta, cfg, weights, wavs, hs, norms = golden_loader(name)
    out, counts = restated(name)
    n_max = max(meta["lengths"])
    assert len(hs) == cfg.num_hidden_states == cfg.encoder_layers + 1 == meta["n_states"]
    assert counts == meta["frames"] == [cfg.valid_frames(n, n_max) for n in meta["lengths"]]
    assert meta["chunks"] == R.chunk_sizes(cfg.num_frames(n_max), cfg.mj_sequence_length)
    assert meta["shape"] == [len(wavs), cfg.num_frames(n_max), cfg.encoder_embed_dim]
    ts, cs = meta["t_stride"], meta["c_stride"]
    for l, h in enumerate(out["hidden_states"]):
        assert list(h.shape) == meta["shape"]
        for b, n in enumerate(counts):  # live rows only: padding rows are outside the contract
            assert O.rel_err(h[b, :n:ts, ::cs], hs[l][b, :-(-n // ts)]) <= REF_PIN, (name, l, b)
        assert abs(np.linalg.norm(_live(h, counts)) - norms[l]) / norms[l] <= REF_PIN
    assert meta["score_std"][0] >= 0.5
    assert max(meta["ref_fp32_err"]) <= 2e-6 and max(meta["fp32_proxy_err"]) <= 0.25e-4


def test_the_fixtures_cover_what_they_are_named_for(golden_loader):
    get = lambda n: golden_loader("mockingjay/" + n)  # noqa: E731
    meta, cfg = get("tiny_chunk")[:2]
    assert cfg.mj_sequence_length == 16 and meta["chunks"] == [13, 13] and min(meta["frames"]) < 13  # one ends inside chunk 0
    meta, cfg = get("tiny_chunk3")[:2]
    assert cfg.mj_sequence_length == 3 and meta["chunks"] == [3, 3, 3, 1]
    assert get("tiny_eps")[1].mj_layer_norm_eps == 1e-2 and get("tiny_pad")[1].mj_layer_norm_eps == 1e-12
    meta, cfg = get("tiny_albert")[:2]
    assert cfg.mj_share_layer and cfg.encoder_layers == 3 and meta["n_states"] == 4
    assert get("tiny_kaldi")[1].mj_frontend == "kaldi" and get("tiny_kaldi")[1].mj_delta_order == 2 and get("tiny_kaldi")[1].mj_cmvn
    meta, cfg = get("tera_base_pseudo")[:2]
    assert (cfg.encoder_embed_dim, cfg.encoder_layers, meta["lengths"]) == (768, 3, [16000, 12345])
    assert get("tiny_pad")[0]["lengths"] == [4000, 2345, 3111] and get("tiny_pad")[1].mj_input_dim == 16


def test_a_baked_in_eps_would_show_on_the_eps_fixture(golden_loader):
    """tiny_eps runs layer_norm_eps = 1e-2: the restatement evaluated with 1e-5 instead misses the fixture by far more than any
    tolerance of the suite (so a kernel with 1e-5 baked in cannot pass it)."""
    import dataclasses

    meta, cfg, weights, wavs, hs, norms = golden_loader("mockingjay/tiny_eps")
    feats, counts = R.features(cfg, wavs)
    wrong = R.model(dataclasses.replace(cfg, mj_layer_norm_eps=1e-5), weights, feats.astype(np.float32), counts)["hidden_states"]
    for l in range(len(hs)):
        assert O.rel_err(_live(wrong[l], counts), _live(hs[l], counts)) > 1e-3


# ---- front end ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lengths", [[4000, 3900], [201], [320, 250], [8000, 16000], [4000, 2345, 3111]])
def test_stft_matches_torch_stft_in_float64(lengths):
    """reflect edges; a shorter utterance's tail frames see the batch's zeros; one ending within 200 samples of max_len a mixture"""
    import torch

    rng = np.random.default_rng(sum(lengths))
    batch = np.zeros((len(lengths), max(lengths)))
    for b, n in enumerate(lengths):
        batch[b, :n] = rng.standard_normal(n)
    got = R.stft_power(batch)
    ref = torch.stft(torch.from_numpy(batch), n_fft=400, hop_length=160, win_length=400, window=torch.hann_window(400, dtype=torch.float64),
                     center=True, pad_mode="reflect", normalized=False, onesided=True, return_complex=True)
    ref = (ref.abs() ** 2).transpose(1, 2).numpy()
    assert got.shape == ref.shape == (len(lengths), 1 + max(lengths) // 160, 201)
    assert np.abs(got - ref).max() <= 1e-12 * ref.max()
    assert np.array_equal(R.hann_periodic(), torch.hann_window(400, dtype=torch.float64).numpy()) or \
        np.abs(R.hann_periodic() - torch.hann_window(400, dtype=torch.float64).numpy()).max() < 1e-15


def test_stft_refuses_what_torch_refuses():
    with pytest.raises(ValueError):
        R.stft_power(np.zeros((1, 200)))
    assert R.stft_power(np.ones((1, 201))).shape == (1, 2, 201)


@pytest.mark.parametrize("n_mels", [16, 40, 80])
def test_mel_filter_bank_closed_form(n_mels):
    """HTK triangles, f_min 0, f_max 8000, no norm: corners equally spaced in mel, each filter piecewise linear in Hz with peak 1 at
    its centre, zero outside its corners; written out per element here, independently of the vectorised form."""
    fb = R.mel_banks(n_mels)
    assert fb.shape == (201, n_mels) and fb.min() >= 0.0 and fb.max() <= 1.0
    mel = lambda f: 2595.0 * math.log10(1.0 + f / 700.0)  # noqa: E731
    inv = lambda m: 700.0 * (10.0 ** (m / 2595.0) - 1.0)  # noqa: E731
    pts = [inv(mel(8000.0) * i / (n_mels + 1)) for i in range(n_mels + 2)]
    assert abs(pts[0]) < 1e-9 and abs(pts[-1] - 8000.0) < 1e-6
    for k in range(0, 201, 7):
        f = 40.0 * k
        for m in range(n_mels):
            lo, ce, hi = pts[m], pts[m + 1], pts[m + 2]
            want = 0.0 if f <= lo or f >= hi else ((f - lo) / (ce - lo) if f <= ce else (hi - f) / (hi - ce))
            assert abs(fb[k, m] - want) < 1e-12, (k, m)
    assert not fb[0].any() and fb[200].max() < 1e-12  # DC and Nyquist sit on the outer corners (the last one up to rounding)


def test_frame_count_rule_is_batch_dependent():
    from s3prl_amd.synth import named_config

    cfg = named_config("tera_base")
    assert R.frame_counts([8000, 16000]) == [50, 101] and R.frame_counts([8000]) == [51]
    assert cfg.valid_frames(8000, 16000) == 50 and cfg.valid_frames(8000, 8000) == 51 and cfg.num_frames(8000) == 51
    assert cfg.num_frames(200) == 0 and cfg.num_frames(201) == 2 and cfg.num_frames(240000) == 1501
    import dataclasses

    assert dataclasses.replace(cfg, mj_cmvn=False).valid_frames(8000, 16000) == 101  # no zero rows without CMVN
    kal = named_config("mockingjay_base")
    assert kal.num_frames(16000) == 98 and kal.valid_frames(8000, 16000) == 48 and kal.num_frames(399) == 0


def test_logmel_rows_behind_the_count_are_zero_and_the_scale_is_removed():
    from s3prl_amd.synth import synth_wavs

    wavs = synth_wavs([8000, 16000], 5)
    feats, counts = R.logmel(wavs, 16)
    assert counts == [50, 101] and not feats[0, 50:].any() and feats[0, 49].any()
    again, _ = R.logmel([w.astype(np.float64) * 30.0 for w in wavs], 16)  # (in float64: an fp32 product would round the samples)
    assert np.abs(again - feats).max() < 1e-8  # the decibel normalisation removes an input scale
    raw, cnt = R.logmel(wavs, 16, cmvn=False)
    assert cnt == [101, 101] and raw[0, 60:].max() < -20.0  # log(1e-10) = -23.03: the batch's zeros


@pytest.mark.parametrize("T, seq", [(1501, 1500), (26, 16), (10, 3), (9, 2), (7, 2), (5, 3), (100, 0), (16, 16), (17, 16), (1001, 500)])
def test_chunk_sizes_follow_torch_chunk(T, seq):
    import torch

    x = torch.zeros(1, T, 1)
    want = [T] if seq == 0 or T <= seq else [int(c.shape[1]) for c in torch.chunk(x, math.ceil(T / seq), dim=1)]
    assert R.chunk_sizes(T, seq) == want and sum(want) == T
    if (T, seq) == (1501, 1500):
        assert want == [751, 750]
    if (T, seq) == (10, 3):
        assert want == [3, 3, 3, 1]


def test_position_table_is_the_reference_formula():
    tab = R.position_table(5, 8)
    assert tab.dtype == np.float32 and tab.shape == (5, 8)
    for t in range(5):
        for j in range(8):
            a = t / (10000.0 ** (2 * (j // 2) / 8))
            assert tab[t, j] == np.float32(math.sin(a) if j % 2 == 0 else math.cos(a))


# ---- configuration ----------------------------------------------------------------------------------------------------------------
def _upstream_config(**over):
    from s3prl_amd.ckpt import mockingjay_upstream_config
    from s3prl_amd.synth import named_config

    config = mockingjay_upstream_config(named_config(over.pop("base", "tera_base")))
    for key, value in over.items():
        block, field = key.split("__")
        config[block][field] = value
    return config


def test_config_parsing_of_the_released_shapes():
    from s3prl_amd.config import config_from_mockingjay
    from s3prl_amd.synth import named_config

    for name in ("tera_base", "mockingjay_base", "mockingjay_large", "audio_albert_base", "tiny_mockingjay_kaldi", "tiny_mockingjay_eps"):
        cfg = named_config(name)
        assert config_from_mockingjay(_upstream_config(base=name)) == cfg, name
    tera, large, albert, base = (named_config(n) for n in ("tera_base", "mockingjay_large", "audio_albert_base", "mockingjay_base"))
    assert (tera.encoder_embed_dim, tera.encoder_layers, tera.encoder_attention_heads, tera.encoder_ffn_embed_dim) == (768, 3, 12, 3072)
    assert tera.mj_sequence_length == 1500 and tera.mj_input_dim == 80 and tera.mj_frontend == "mel" and tera.mj_layer_norm_eps == 1e-12
    assert large.encoder_layers == 12 and large.mj_sequence_length == 500 and large.num_hidden_states == 13
    assert albert.mj_share_layer and not tera.mj_share_layer
    assert base.mj_frontend == "kaldi" and base.mj_input_dim == 240 and base.conv_layers == [(768, 400, 160)]
    assert tera.conv_layers == [(768, 0, 160)] and tera.downsample_rate == 160


@pytest.mark.parametrize("over, exc, match", [
    (dict(audio__input=dict(feat_type="linear", log=True, delta=0, cmvn=True)), NotImplementedError, "feat_type"),
    (dict(audio__input=dict(feat_type="mfcc", log=True, delta=0, cmvn=True)), NotImplementedError, "feat_type"),
    (dict(audio__input=dict(feat_type="mel", log=True, delta=1, cmvn=True)), NotImplementedError, "delta"),
    (dict(audio__input=dict(feat_type="mel", log=False, delta=0, cmvn=True)), NotImplementedError, "log"),
    (dict(audio__win_ms=20), NotImplementedError, "win_ms"),
    (dict(transformer__pre_layer_norm=True), ValueError, "pre_layer_norm"),
    (dict(transformer__hidden_act="relu"), ValueError, "hidden_act"),
    (dict(transformer__num_attention_heads=8), ValueError, "must be 64"),
    (dict(audio__n_mels=42), ValueError, "multiple of 4"),
])
def test_config_refusals_by_name(over, exc, match):
    from s3prl_amd.config import config_from_mockingjay

    with pytest.raises(exc, match=match):
        config_from_mockingjay(_upstream_config(**over))


def test_a_config_without_an_audio_block_is_refused():
    from s3prl_amd.config import config_from_mockingjay

    config = _upstream_config()
    del config["audio"]
    with pytest.raises(ValueError, match="audio"):
        config_from_mockingjay(config)
    assert config_from_mockingjay(_upstream_config(audio__input=dict(feat_type="mel", log=True, delta=0, cmvn=False))).mj_cmvn is False


# ---- checkpoints --------------------------------------------------------------------------------------------------------------------
def test_checkpoint_key_mapping(tmp_path):
    """{"Transformer", "Upstream_Config"} and the legacy {"Transformer", "Config"} with gamma / beta LayerNorm names; SpecHead is
    ignored; a missing tensor is named."""
    import torch

    from s3prl_amd.ckpt import load_checkpoint, mockingjay_upstream_config, save_checkpoint
    from s3prl_amd.synth import named_config, param_shapes, synth_weights

    cfg = named_config("tiny_mockingjay_albert")
    weights = synth_weights(cfg, 3)
    assert set(weights) == set(param_shapes(cfg)) and all(k.startswith(("input_representations.", "encoder.layer.0.")) for k in weights)
    path = str(tmp_path / "new.ckpt")
    save_checkpoint(path, cfg, weights)
    got_cfg, got = load_checkpoint(path, "mockingjay")
    assert got_cfg == cfg and set(got) == set(weights) and all(np.array_equal(got[k], weights[k]) for k in weights)
    # legacy: 'Config' holds the upstream config, LayerNorm parameters are called gamma / beta, the pre-training head rides along
    legacy = {}
    for k, v in weights.items():
        k = k.replace("LayerNorm.weight", "LayerNorm.gamma").replace("LayerNorm.bias", "LayerNorm.beta")
        legacy[k] = torch.from_numpy(v)
    assert any(k.endswith("gamma") for k in legacy) and any(k.endswith("beta") for k in legacy)
    old = str(tmp_path / "old.ckpt")
    torch.save({"Transformer": legacy, "SpecHead": {"dense.weight": torch.zeros(2, 2)}, "Config": mockingjay_upstream_config(cfg)}, old)
    got_cfg, got = load_checkpoint(old, "mockingjay")
    assert got_cfg == cfg and set(got) == set(weights) and all(np.array_equal(got[k], weights[k]) for k in weights)
    # no audio block: refused, as the reference's expert refuses it
    config = mockingjay_upstream_config(cfg)
    del config["audio"]
    torch.save({"Transformer": legacy, "Upstream_Config": config, "Config": {}}, old)
    with pytest.raises(ValueError, match="audio"):
        load_checkpoint(old, "mockingjay")
    del legacy["encoder.layer.0.output.dense.bias"]
    torch.save({"Transformer": legacy, "Upstream_Config": mockingjay_upstream_config(cfg), "Config": {}}, old)
    with pytest.raises(Exception, match="encoder.layer.0.output.dense.bias"):
        load_checkpoint(old, "mockingjay")
    torch.save({"Upstream_Config": mockingjay_upstream_config(cfg)}, old)
    with pytest.raises(ValueError, match="Transformer"):
        load_checkpoint(old, "mockingjay")


# ---- the library's own refusals ---------------------------------------------------------------------------------------------------
def _create_error(ccfg, mj):
    from s3prl_amd import _lib

    lib = _lib.load()
    h = C.c_void_p()
    tensors = (_lib.S3Tensor * 1)()
    assert lib.s3enc_create_mockingjay(C.byref(ccfg), C.byref(mj) if mj is not None else None, tensors, 0, 0, C.byref(h)) != 0
    assert not h.value
    return lib.s3enc_last_error().decode()


@pytest.mark.parametrize("field, value, match", [
    ("pre_layer_norm", 1, "pre_layer_norm"),
    ("hidden_act", 1, "hidden_act"),
    ("input_dim", 18, "multiple of 4"),
    ("sequence_length", -1, "sequence_length"),
    ("frontend", 2, "frontend"),
    ("n_mels", 20, "n_mels"),
    ("layer_norm_eps", -1.0, "layer_norm_eps"),
])
def test_the_library_refuses_by_name(field, value, match):
    from s3prl_amd import _lib
    from s3prl_amd.synth import named_config

    cfg = named_config("tiny_mockingjay")
    ccfg, mj = _lib.make_config(cfg, "fp32"), _lib.make_mockingjay_config(cfg)
    assert ccfg.family == 8 and ccfg.n_conv == 1 and (ccfg.conv_kernel[0], ccfg.conv_stride[0]) == (0, 160) and ccfg.encoder_layers == 2
    assert (mj.input_dim, mj.share_layer, mj.sequence_length, mj.frontend, mj.n_mels, mj.cmvn) == (16, 0, 0, 1, 16, 1)
    assert abs(mj.layer_norm_eps - 1e-12) < 1e-18 and mj.target_level == -25.0
    setattr(mj, field, value)
    assert match in _create_error(ccfg, mj)


def test_the_library_refuses_a_head_width_other_than_64():
    from s3prl_amd import _lib
    from s3prl_amd.synth import named_config

    cfg = named_config("tiny_mockingjay")
    ccfg, mj = _lib.make_config(cfg, "fp32"), _lib.make_mockingjay_config(cfg)
    ccfg.heads = 4
    assert "must be 64" in _create_error(ccfg, mj)


@pytest.mark.parametrize("dtype", ["bf16", "fp16", "fp16x2", "fp32x3"])
def test_non_fp32_modes_are_refused_with_the_mode_named(dtype):
    from s3prl_amd import _lib
    from s3prl_amd.encoder import HipEncoder
    from s3prl_amd.synth import named_config, synth_weights

    cfg = named_config("tiny_mockingjay")
    err = _create_error(_lib.make_config(cfg, dtype), _lib.make_mockingjay_config(cfg))
    assert "fp32 only" in err and dtype in err
    with pytest.raises(ValueError, match="fp32 only"):
        HipEncoder(cfg, synth_weights(cfg, 0), dtype=dtype)


def test_the_block_is_required_for_the_family_and_refused_elsewhere():
    from s3prl_amd import _lib
    from s3prl_amd.synth import named_config

    cfg = named_config("tiny_mockingjay")
    lib = _lib.load()
    h = C.c_void_p()
    tensors = (_lib.S3Tensor * 1)()
    ccfg = _lib.make_config(cfg, "fp32")
    name = b"s3enc_create_mockingjay"
    assert lib.s3enc_create(C.byref(ccfg), tensors, 0, 0, C.byref(h)) != 0 and name in lib.s3enc_last_error()
    assert lib.s3enc_create_ex(C.byref(ccfg), None, tensors, 0, 0, C.byref(h)) != 0 and name in lib.s3enc_last_error()
    cpc = _lib.make_cpc_config(named_config("tiny_cpc"))
    assert lib.s3enc_create_cpc(C.byref(ccfg), C.byref(cpc), tensors, 0, 0, C.byref(h)) != 0 and name in lib.s3enc_last_error()
    apc = _lib.make_apc_config(named_config("tiny_apc"))
    assert lib.s3enc_create_apc(C.byref(ccfg), C.byref(apc), tensors, 0, 0, C.byref(h)) != 0 and name in lib.s3enc_last_error()
    assert "null argument" in _create_error(ccfg, None)
    assert "S3ENC_MOCKINGJAY only" in _create_error(_lib.make_config(named_config("tiny_hubert"), "fp32"), _lib.make_mockingjay_config(cfg))
    assert lib.s3enc_version() == 8  # every addition is a new symbol


def test_block_follows_the_header(tmp_path):
    """s3enc_mockingjay_config: field order against the header text, size and offsets against the header compiled as C."""
    import subprocess

    from s3prl_amd import _lib

    header = open(os.path.join(ROOT, "include", "s3enc.h")).read()
    body = header[header.index("typedef struct s3enc_mockingjay_config {"):header.index("} s3enc_mockingjay_config;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = re.findall(r"(?:int32_t|float)\s+([a-z0-9_]+)(?:\[[^\]]*\])?;", body)
    assert names == [n for n, _ in _lib.S3MockingjayConfig._fields_] and names[0] == "input_dim" and names[-1] == "fbank_cmvn_eps"
    assert _lib.FAMILY["mockingjay"] == 8 and "S3ENC_MOCKINGJAY = 8" in header and "#define S3ENC_VERSION 8" in header
    assert [n for n, _ in _lib.S3Config._fields_][-1] == "dw_kernel"
    for sym in ("s3enc_create_mockingjay", "s3enc_logmel_forward", "s3enc_logmel_frame_counts", "s3enc_op_layernorm_eps", "s3enc_op_input_repr"):
        assert re.search(r"\bint " + sym + r"\(", header), sym
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "s3enc.h"\n'
                   'int main(void){printf("%zu %zu %zu %zu %zu\\n", sizeof(s3enc_mockingjay_config), '
                   'offsetof(s3enc_mockingjay_config, layer_norm_eps), offsetof(s3enc_mockingjay_config, target_level), '
                   'offsetof(s3enc_mockingjay_config, fbank_cmvn_eps), sizeof(s3enc_apc_config));return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    W = _lib.S3MockingjayConfig
    assert got == [C.sizeof(W), W.layer_norm_eps.offset, W.target_level.offset, W.fbank_cmvn_eps.offset, C.sizeof(_lib.S3ApcConfig)]


def test_frame_counts_entry_is_pythons_rule():
    """s3enc_logmel_frame_counts (host only): round(length / (n_max / T)) with halves to even, against Python on many lengths"""
    from s3prl_amd import _lib

    lib = _lib.load()
    rng = np.random.default_rng(11)
    for _ in range(40):
        B = int(rng.integers(1, 6))
        lengths = [int(v) for v in rng.integers(201, 40000, size=B)]
        for n_max in (0, max(lengths) + int(rng.integers(0, 500))):
            out = (C.c_int32 * B)()
            _lib.check(lib.s3enc_logmel_frame_counts((C.c_int64 * B)(*lengths), B, n_max, out))
            assert list(out) == R.frame_counts(lengths, n_max or None)
    out = (C.c_int32 * 2)()
    _lib.check(lib.s3enc_logmel_frame_counts((C.c_int64 * 2)(8000, 16000), 2, 0, out))
    assert list(out) == [50, 101]
    assert lib.s3enc_logmel_frame_counts((C.c_int64 * 2)(8000, 16000), 2, 9000, out) != 0 and b"n_max" in lib.s3enc_last_error()


def test_op_entries_validate_their_arguments():
    from s3prl_amd import _lib

    lib = _lib.load()
    one = C.c_void_p(256)
    ln = lambda x, g, b, eps, rows, Cc, out: lib.s3enc_op_layernorm_eps(x, g, b, eps, rows, Cc, out, None)  # noqa: E731
    assert ln(None, one, one, 1e-12, 4, 128, one) != 0 and b"null argument" in lib.s3enc_last_error()
    assert ln(one, one, one, 1e-12, 4, 130, one) != 0 and b"multiple of 4" in lib.s3enc_last_error()
    assert ln(one, one, one, 1e-12, 0, 128, one) != 0 and b"bad shape" in lib.s3enc_last_error()
    assert ln(one, one, one, -1.0, 4, 128, one) != 0 and b"eps" in lib.s3enc_last_error()
    ir = lambda F, D, rows=4, Tc=2, pos=one: lib.s3enc_op_input_repr(one, one, one, pos, Tc, one, one, 1e-12, rows, F, D, one, None)  # noqa: E731
    assert ir(16, 128, pos=None) != 0 and b"null argument" in lib.s3enc_last_error()
    assert ir(18, 128) != 0 and b"multiples of 4" in lib.s3enc_last_error()
    assert ir(16, 130) != 0 and b"multiples of 4" in lib.s3enc_last_error()
    assert ir(16, 128, Tc=0) != 0 and b"bad shape" in lib.s3enc_last_error()
    lens = (C.c_int64 * 2)(4000, 150)
    ptrs = (C.c_void_p * 2)(256, 256)
    fw = lambda lens_, nmel, cmvn, counts, n_max=0: lib.s3enc_logmel_forward(ptrs, lens_, 2, n_max, nmel, -25.0, cmvn, counts, one, 0, None)  # noqa: E731
    assert fw(lens, 16, 0, None) != 0 and b"200 samples" in lib.s3enc_last_error()
    lens[1] = 3000
    assert fw(lens, 0, 0, None) != 0 and b"n_mels" in lib.s3enc_last_error()
    assert fw(lens, 16, 1, None) != 0 and b"frame counts" in lib.s3enc_last_error()
    assert fw(lens, 16, 1, (C.c_int32 * 2)(26, 1)) != 0 and b"2..T" in lib.s3enc_last_error()
    assert fw(lens, 16, 0, None, 3999) != 0 and b"n_max" in lib.s3enc_last_error()


# ---- hub --------------------------------------------------------------------------------------------------------------------------
def test_hub_names_have_the_reference_signatures():
    import s3prl_amd.hub as amd

    ref = json.load(open(os.path.join(ROOT, "tests", "golden", "mockingjay", "reference_hub_mockingjay.json")))
    everything = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_hub.json")))["options"]
    assert ref["downsample_rate"] == 160
    checked = []
    for fam in ("mockingjay", "tera", "audio_albert"):
        for name, params in ref["hubconfs"][fam]:
            assert name in everything and name in amd.options(), name
            ours = inspect.signature(getattr(amd, name))
            assert [list(p) for p in params] == [[k, v.kind.name, repr(v.default)] for k, v in ours.parameters.items()], name
            checked.append(name)
    assert len(checked) == 28 and {"tera", "mockingjay", "audio_albert", "tera_fbankBase_T_F_AdamW_b32_200k_100hr"} <= set(checked)
    # the reference's hub lists no further name of the three families
    assert sorted(n for n in everything if n.startswith(("mockingjay", "tera", "audio_albert"))) == sorted(checked)
    reg = set(amd.options(only_registered_ckpt=True))
    assert {"tera", "tera_960hr", "mockingjay", "mockingjay_origin", "audio_albert", "audio_albert_960hr"} <= reg
    assert not {"tera_local", "tera_url", "mockingjay_local", "mockingjay_url", "audio_albert_local", "audio_albert_url"} & reg
    assert [p for p in inspect.signature(amd.mockingjay_local).parameters] == ["ckpt", "options_config", "args", "kwargs"]


def test_released_names_resolve_their_urls_through_the_cache(monkeypatch):
    import s3prl_amd.upstream.audio_albert.hubconf as ah
    import s3prl_amd.upstream.mockingjay.hubconf as mh
    import s3prl_amd.upstream.tera.hubconf as th

    seen = []
    for mod, local in ((mh, "mockingjay_local"), (th, "tera_local"), (ah, "audio_albert_local")):
        monkeypatch.setattr(mod, "_urls_to_filepaths", lambda url, refresh=False: seen.append((url, refresh)) or "/cache/" + url[-12:])
        monkeypatch.setattr(mod, local, lambda ckpt, *a, **k: ("expert", ckpt, k))
    assert th.tera(True)[1].startswith("/cache/") and seen[-1] == (
        "https://huggingface.co/s3prl/tera/resolve/main/tera_logMelBase_T_F_M_AdamW_b32_1m_960hr_drop1/states-1000000.ckpt", True)
    assert th.tera_100hr() and seen[-1] == ("https://www.dropbox.com/s/l9ryl82k64m1lsk/states-200000.ckpt?dl=1", False)
    assert mh.mockingjay() and "mockingjay_logMelLinearLarge_T_AdamW_b32_500k_360hr_drop1" in seen[-1][0]
    assert mh.mockingjay_960hr() and seen[-1][0] == "https://www.dropbox.com/s/7f9z6dzc7oix6qv/states-1000000.ckpt?dl=1"
    assert ah.audio_albert(options_config=None)[2] == {"options_config": None} and "audio_albert_logMelBase_T_share" in seen[-1][0]


def test_expert_loads_a_checkpoint_and_refuses_the_options_that_change_the_forward(tmp_path):
    """Without a GPU: construction through all three hub entries, the stride, the state count; the forward itself needs the MI355X."""
    import torch
    import yaml

    import s3prl_amd.hub as amd
    from s3prl_amd.ckpt import save_checkpoint
    from s3prl_amd.synth import named_config, synth_weights

    for name, entry in (("tiny_mockingjay_chunk", amd.tera_local), ("tiny_mockingjay_albert", amd.audio_albert_local),
                        ("tiny_mockingjay_kaldi", amd.mockingjay_local)):
        cfg = named_config(name)
        path = str(tmp_path / "c.ckpt")
        save_checkpoint(path, cfg, synth_weights(cfg, 0))
        expert = entry(path)
        assert expert.cfg == cfg and expert.get_downsample_rates("hidden_states") == 160
        assert expert.num_layers == cfg.encoder_layers + 1 and expert.hidden_sizes == [128] * expert.num_layers
        with pytest.raises(RuntimeError, match="inference-only"):
            expert([torch.zeros(4000, requires_grad=True)])
        if not torch.cuda.is_available():
            with pytest.raises(RuntimeError, match="no CPU fallback"):
                expert([torch.zeros(4000)])
    base = {"load_pretrain": "True", "no_grad": "True", "dropout": "default", "spec_aug": "False", "spec_aug_prev": "True",
            "output_hidden_states": "True", "permute_input": "False"}
    opt = str(tmp_path / "options.yaml")

    def build(**over):
        with open(opt, "w") as f:
            yaml.safe_dump({**base, **over}, f)
        return amd.mockingjay_local(path, opt)

    assert build().cfg == cfg
    for over, match in ((dict(permute_input="True"), "permute_input"), (dict(load_pretrain="False"), "load_pretrain"),
                        (dict(dropout=0.3), "dropout"), (dict(output_hidden_states="False"), "output_hidden_states")):
        with pytest.raises(NotImplementedError, match=match):
            build(**over)
    with pytest.raises(RuntimeError, match="Only one of them"):
        build(no_grad="False", spec_aug_prev="False")
    aug = build(spec_aug="True").train()
    with pytest.raises(NotImplementedError, match="spec_aug"):
        aug([torch.zeros(4000)])
