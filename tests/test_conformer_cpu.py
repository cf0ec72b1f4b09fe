"""wav2vec 2.0 Conformer encoders without a GPU: config parsing and refusals, the hub entries (cache hit and miss), the ABI 8
fields of s3enc_config, and the float64 restatement of tests/conformer_ref.py against every reference-generated fixture."""

import ctypes as C
import os
import re

import numpy as np
import pytest

from oracle import encoder_oracle as O

import conformer_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = ["conformer/" + n for n in ["conformer_relpos_tiny_pad", "conformer_rope_tiny_pad", "conformer_rope_postln_tiny_pad", "conformer_relpos_tiny_eq",
            "conformer_relpos_tiny_t49", "conformer_relpos_large_pseudo", "conformer_rope_large_pseudo"]]


def _model_cfg(**kw):
    d = dict(extractor_mode="layer_norm", encoder_layers=2, encoder_embed_dim=128, encoder_ffn_embed_dim=256,
             encoder_attention_heads=2, layer_norm_first=True, conv_pos=16, conv_pos_groups=4, activation_fn="gelu",
             layer_type="conformer", pos_enc_type="rel_pos", attn_type="espnet", depthwise_conv_kernel_size=15)
    d.update(kw)
    return d


def test_converted_and_fairseq_configs_parse():
    from s3prl_amd.config import config_from_dicts

    cfg = config_from_dicts("wav2vec2", _model_cfg(), {"normalize": True})
    assert (cfg.layer_type, cfg.pos_enc_type, cfg.attn_type, cfg.depthwise_conv_kernel_size) == ("conformer", "rel_pos", "espnet", 15)
    assert cfg.normalize and cfg.layer_norm_first

    class Choice:  # a fairseq ChoiceEnum member: the name carries the value
        name = "conformer"

    cfg = config_from_dicts("wav2vec2", _model_cfg(layer_type=Choice(), pos_enc_type="rope"))
    assert (cfg.layer_type, cfg.pos_enc_type) == ("conformer", "rope")
    assert config_from_dicts("wav2vec2", _model_cfg(layer_type="transformer")).layer_type == "transformer"


@pytest.mark.parametrize("kw, match", [
    (dict(pos_enc_type="abs"), "pos_enc_type='abs'"),
    (dict(attn_type="fairseq"), "attn_type='fairseq'"),
    (dict(attn_type=""), "attn_type=''"),
    (dict(depthwise_conv_kernel_size=30), "depthwise_conv_kernel_size"),
])
def test_config_refusals(kw, match):
    from s3prl_amd.config import config_from_dicts

    with pytest.raises(ValueError, match=re.escape(match)):
        config_from_dicts("wav2vec2", _model_cfg(**kw))


def test_feature_selection_is_refused(tmp_path):
    from s3prl_amd.ckpt import save_checkpoint
    from s3prl_amd.synth import named_config, synth_weights
    from s3prl_amd.upstream.wav2vec2.expert import UpstreamExpert

    cfg = named_config("tiny_conformer_rope")
    path = str(tmp_path / "c.pt")
    save_checkpoint(path, cfg, synth_weights(cfg, 0))
    for sel in ("fairseq_layers", "fairseq_layers_before_residual"):
        with pytest.raises(ValueError, match="empty list"):
            UpstreamExpert(path, feature_selection=sel)


def test_hub_names_load_from_the_cache_and_refuse_a_miss(tmp_path, monkeypatch):
    import s3prl_amd.hub as amd
    from s3prl_amd import download
    from s3prl_amd.ckpt import save_checkpoint
    from s3prl_amd.synth import named_config, synth_weights

    def no_fetch(url, dst):  # the conformer entries must never try the network
        raise AssertionError(f"fetch attempted: {url}")

    monkeypatch.setattr(download, "_fetch", no_fetch)
    old = download.get_dir()
    download.set_dir(tmp_path / "cache")
    try:
        for name, cfg_name in (("wav2vec2_conformer_relpos", "tiny_conformer_relpos"),
                               ("wav2vec2_conformer_rope", "tiny_conformer_rope"),
                               ("wav2vec2_conformer_large_s2st_es_voxpopuli", "tiny_conformer_rope_postln"),
                               ("wav2vec2_conformer_large_s2st_en_librilight", "tiny_conformer_relpos")):
            entry = getattr(amd, name)
            with pytest.raises(NotImplementedError, match=f"{name}: {re.escape(os.path.basename(entry.url))} is not in the download cache"):
                entry()
            with pytest.raises(RuntimeError):  # still the cache-miss contract of every other name
                entry()
            cfg = named_config(cfg_name)
            w = synth_weights(cfg, 9)
            save_checkpoint(str(download.cache_path(entry.url)), cfg, w)
            expert = entry()
            assert expert.cfg.to_dict() == cfg.to_dict()
            assert expert.cfg.layer_type == "conformer"
            k = "encoder.layers.0.conv_module.batch_norm.running_var"
            assert np.array_equal(expert._weights[k], w[k])
        with pytest.raises(NotImplementedError, match="conformer"):
            amd.wav2vec2_conformer_relpos(legacy=True)  # the legacy file is a different cache entry
    finally:
        download.set_dir(old)


def test_config_struct_fields_and_header_agree():
    from s3prl_amd import _lib
    from s3prl_amd.synth import named_config

    names = [f[0] for f in _lib.S3Config._fields_]
    assert names[-3:] == ["layer_type", "pos_enc_type", "dw_kernel"]
    assert _lib.S3Config.layer_type.offset == _lib.S3Config.mr_plain.offset + 4
    assert C.sizeof(_lib.S3Config) == _lib.S3Config.dw_kernel.offset + 4
    hdr = open(os.path.join(ROOT, "include", "s3enc.h")).read()
    body = hdr[hdr.index("typedef struct s3enc_config {"):hdr.index("} s3enc_config;")]
    assert re.findall(r"int32_t (layer_type|pos_enc_type|dw_kernel);", body) == ["layer_type", "pos_enc_type", "dw_kernel"]
    assert _lib.ABI_VERSION == 8
    for name, pe in (("tiny_conformer_relpos", 1), ("tiny_conformer_rope", 2)):
        c = _lib.make_config(named_config(name), "fp32")
        assert (c.layer_type, c.pos_enc_type, c.dw_kernel) == (1, pe, 31)
    c = _lib.make_config(named_config("tiny_wav2vec2"), "fp32")
    assert (c.layer_type, c.pos_enc_type, c.dw_kernel) == (0, 0, 0)


def test_synth_weights_name_the_reference_tensors():
    from s3prl_amd.synth import named_config, synth_weights

    cfg = named_config("wav2vec2_conformer_large_relpos")
    assert (cfg.encoder_embed_dim, cfg.encoder_attention_heads, cfg.encoder_ffn_embed_dim, cfg.encoder_layers) == (1024, 16, 4096, 24)
    w = synth_weights(named_config("tiny_conformer_relpos"), 0)
    assert w["encoder.layers.0.self_attn.pos_bias_u"].shape == (2, 64)
    assert w["encoder.layers.2.conv_module.depthwise_conv.weight"].shape == (128, 1, 31)
    assert np.all(w["encoder.layers.0.conv_module.batch_norm.running_var"] > 0.4)
    assert "encoder.layers.0.self_attn.linear_pos.weight" not in synth_weights(named_config("tiny_conformer_rope"), 0)


@pytest.mark.parametrize("name", FIXTURES)
def test_restatement_matches_the_reference_fixtures(name, golden_loader):
    meta, cfg, weights, wavs, hs, norms = golden_loader(name)
    ref = R.forward(cfg, weights, wavs)
    ts, cs = meta["t_stride"], meta["c_stride"]
    assert len(ref) == len(hs) == cfg.encoder_layers + 1
    errs = [O.rel_err(ref[l][:, ::ts, ::cs], hs[l]) for l in range(len(hs))]
    assert max(errs) < 1e-5, errs
