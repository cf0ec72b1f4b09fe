"""MAE-AST without a GPU: the float64 restatement tests/mae_ast_ref.py against every fixture the reference model produced (that pins
the yardstick of the GPU tests), the padding rule against the reference's own recorded mask sums and a hand table, the frame / state
/ downsample counts, the checkpoint reader, the hub names and signatures, the family constants and the Python-side refusals."""

import inspect
import json
import os

import numpy as np
import pytest

import mae_ast_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FP32_TOL = 1e-4
FIXTURES = ["tiny_patch_eq", "tiny_patch_pad", "tiny_frame_pad", "tiny_preln_pad", "tiny_k3x32_pad", "mae_ast_patch_pseudo",
            "mae_ast_frame_pseudo"]


def _rel(a, b):
    return float(np.linalg.norm(np.asarray(a, np.float64) - np.asarray(b, np.float64)) / np.linalg.norm(np.asarray(b, np.float64)))


# ---- the yardstick ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FIXTURES)
def test_the_float64_restatement_reproduces_the_fixture(name, golden_loader):
    meta, cfg, weights, wavs, hs, norms = golden_loader("mae_ast/" + name)
    ts, cs = meta["t_stride"], meta["c_stride"]
    assert cfg.family == "mae_ast" and len(hs) == cfg.encoder_layers == meta["n_states"]
    out = R.forward(cfg, weights, wavs, feature_dtype=np.float32)  # the features as the generator handed them to the reference
    worst = 0.0
    for l, h in enumerate(hs):
        mine = out["states"][l]
        assert list(mine.shape) == meta["shape"]
        sub = mine[:, ::ts, ::cs]
        rows = [_rel(sub[b, t], h[b, t]) for b in range(h.shape[0]) for t in range(h.shape[1])]
        worst = max(worst, _rel(sub, h), max(rows))
        assert abs(np.linalg.norm(mine) - norms[l]) / norms[l] < 0.25 * FP32_TOL
    print(f"{name}: worst of whole / row {worst:.2e} (recorded {meta['restatement_err']:.2e} / {meta['restatement_row_err']:.2e})")
    assert worst < 0.25 * FP32_TOL
    assert meta["restatement_err"] < 0.25 * FP32_TOL and meta["restatement_row_err"] < 0.25 * FP32_TOL
    assert out["frames"] == meta["fbank_frames"] and "no torchaudio run" in meta["reference"]


def test_the_fixture_set_covers_what_it_should(golden_loader):
    from s3prl_amd.synth import named_config

    metas = {n: golden_loader("mae_ast/" + n)[0] for n in FIXTURES}
    cfgs = {n: named_config(m["config"]) for n, m in metas.items()}
    assert len(set(metas["tiny_patch_eq"]["lengths"])) == 1 and metas["tiny_patch_eq"]["mask_sums"] == [0, 0]
    pad, c = metas["tiny_patch_pad"], cfgs["tiny_patch_pad"]
    assert (c.ma_kt, c.ma_kc) == (16, 16) and max(pad["fbank_frames"]) % 16 != 0
    assert any(f % 16 and f < max(pad["fbank_frames"]) and -(-f // 16) * 8 < pad["tokens"] for f in pad["fbank_frames"])  # a partly real patch
    assert any(f < max(pad["fbank_frames"]) and -(-f // 16) * 8 >= pad["tokens"] for f in pad["fbank_frames"])        # index reaches Ttok
    assert (cfgs["tiny_frame_pad"].ma_kt, cfgs["tiny_frame_pad"].ma_kc) == (2, 128)
    assert cfgs["tiny_preln_pad"].layer_norm_first and not cfgs["tiny_patch_pad"].layer_norm_first
    assert (cfgs["tiny_k3x32_pad"].ma_kt, cfgs["tiny_k3x32_pad"].ma_kc) == (3, 32)
    for n, (kt, kc, width) in {"mae_ast_patch_pseudo": (16, 16, 6144), "mae_ast_frame_pseudo": (2, 128, 768)}.items():
        c = cfgs[n]
        assert (c.ma_kt, c.ma_kc, c.encoder_embed_dim, c.encoder_layers, c.encoder_attention_heads, c.encoder_ffn_embed_dim) == \
            (kt, kc, 768, 12, 12, 3072) and metas[n]["shape"][2] == width and len(metas[n]["lengths"]) == 3 and max(metas[n]["lengths"]) <= 40000


# ---- the padding rule -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FIXTURES)
def test_padding_rule_against_the_references_recorded_mask_sums(name, golden_loader):
    meta, cfg, _, _, _, _ = golden_loader("mae_ast/" + name)
    kv = cfg.ma_key_counts(meta["lengths"])
    assert [meta["tokens"] - k for k in kv] == meta["mask_sums"]
    assert kv == R.key_counts(meta["fbank_frames"], cfg.ma_kt, cfg.ma_kc, meta["tokens"])
    nmax = max(meta["lengths"])
    assert [cfg.valid_frames(n, nmax) for n in meta["lengths"]] == meta["frames"] and cfg.num_frames(nmax) == meta["steps"]
    assert [k // cfg.ma_tokens_per_step for k in kv] == meta["frames"]


def test_padding_rule_hand_table():
    from s3prl_amd.config import mae_ast_config

    n = lambda f: 400 + 160 * (f - 1)  # samples of an utterance with f frames
    patch = mae_ast_config(16, 16, 128, 2, 2, 256, max_token_length=640)
    # F = 64 -> 4 steps, 32 tokens.  equal lengths: nothing masked; F = 33: third patch partly real -> 24 keys; F = 49: index 32 = Ttok
    assert patch.ma_key_counts([n(64), n(64)]) == [32, 32]
    assert patch.ma_key_counts([n(64), n(33), n(32), n(49), n(48), n(1)]) == [32, 24, 16, 32, 24, 8]
    # F = 70 (six frames never read): 4 steps; F = 65..70 would index 40 > Ttok = 32: masks nothing
    assert patch.ma_key_counts([n(70), n(65), n(16)]) == [32, 32, 8]
    frame = mae_ast_config(2, 128, 128, 2, 2, 256, max_token_length=640)
    assert frame.ma_key_counts([n(23), n(13), n(22), n(21), n(2)]) == [11, 7, 11, 11, 1]
    k3 = mae_ast_config(3, 32, 128, 2, 2, 256, max_token_length=640)
    assert k3.ma_key_counts([n(29), n(11), n(26), n(27)]) == [36, 16, 36, 36]


def test_frame_state_and_downsample_counts():
    from s3prl_amd.synth import named_config

    patch, frame = named_config("mae_ast_patch"), named_config("mae_ast_frame")
    assert (patch.downsample_rate, frame.downsample_rate) == (2560, 320)
    assert (patch.num_hidden_states, frame.num_hidden_states) == (12, 12)
    assert (patch.ma_tokens_per_step, frame.ma_tokens_per_step) == (8, 1) and patch.ma_pos_rows == frame.ma_pos_rows == 8192
    for nsamp in (399, 400, 559, 560, 16000, 160000, 2959, 2960):
        F = 1 + (nsamp - 400) // 160 if nsamp >= 400 else 0
        assert patch.num_frames(nsamp) == F // 16 and frame.num_frames(nsamp) == F // 2, nsamp
        # the expert's cut to len(range(0, max_len, kt * 160)) rows never binds (mae_ast/expert.py:95)
        assert patch.num_frames(nsamp) <= len(range(0, nsamp, 2560)) and frame.num_frames(nsamp) <= len(range(0, nsamp, 320))
    assert patch.valid_frames(400 + 160 * 16, 160000) == 2 and patch.valid_frames(400 + 160 * 15, 160000) == 1
    assert patch.valid_frames(160000, 160000) == patch.num_frames(160000) == 62


# ---- the checkpoint reader ----------------------------------------------------------------------------------------------------------
def test_checkpoint_reader(tmp_path):
    import torch

    from s3prl_amd.ckpt import MAE_AST_UNUSED, load_checkpoint, load_mae_ast_checkpoint, mae_ast_cfg_blocks, save_checkpoint
    from s3prl_amd.synth import mae_ast_sine_table, named_config, param_shapes, synth_weights

    cfg = named_config("tiny_mae_ast_preln")
    full = synth_weights(cfg, 5)
    # the FULL strict state dict: decoder, mask embeddings, both tables, the statistics at log-mel scale
    assert {"decoder.layers.1.fc2.weight", "decoder.layer_norm.bias", "encoder_mask_emb", "decoder_mask_emb", "layer_norm.weight",
            "final_proj_reconstruction.weight", "final_proj_classification.bias", "dec_sine_pos_embed.pe", "enc_sine_pos_embed.pe",
            "batch_norm.running_mean", "batch_norm.running_var", "batch_norm.num_batches_tracked"} <= set(full)
    assert full["enc_sine_pos_embed.pe"].shape == (1, 640, 128) and np.array_equal(full["enc_sine_pos_embed.pe"], mae_ast_sine_table(640, 128))
    assert -5 < float(full["batch_norm.running_mean"][0]) < -3 and 18 <= float(full["batch_norm.running_var"][0]) <= 22
    pe = torch.zeros(1, 640, 128)  # the reference's formula (mae_ast.py:802-812), in torch
    position = torch.arange(640).unsqueeze(1)
    div_term = torch.exp(torch.arange(0, 128, 2) * (-np.log(10000.0) / 128))
    pe[0, :, 0::2], pe[0, :, 1::2] = torch.sin(position * div_term), torch.cos(position * div_term)
    assert np.abs(full["enc_sine_pos_embed.pe"] - pe.numpy()).max() < 1e-4
    path = str(tmp_path / "mae_ast.pt")
    save_checkpoint(path, cfg, full)
    state = torch.load(path, map_location="cpu", weights_only=False)
    assert set(state) == {"cfg", "model"} and state["cfg"] == mae_ast_cfg_blocks(cfg) and state["model"]["batch_norm.num_batches_tracked"].shape == ()
    for src in (path, state):
        got_cfg, got = load_mae_ast_checkpoint(src)
        assert got_cfg == cfg and set(got) == set(param_shapes(cfg))  # the unused keys are ignored
        assert not any(k.startswith(MAE_AST_UNUSED) for k in got)
        assert got["enc_sine_pos_embed.pe"].shape == (cfg.ma_pos_rows, 128) == (640, 128)
        assert all(np.array_equal(got[k].reshape(-1), np.asarray(full[k]).reshape(-1)[:got[k].size]) for k in got)
    assert load_checkpoint(path, "mae_ast")[0] == cfg
    # pe is sliced: a table longer than 8192 rows hands over its leading 8192
    long_cfg = named_config("tiny_mae_ast")
    long_cfg = type(long_cfg)(**{**long_cfg.__dict__, "ma_max_token_length": 9000})
    sd = synth_weights(long_cfg, 6)
    got = load_mae_ast_checkpoint({"cfg": mae_ast_cfg_blocks(long_cfg), "model": sd})[1]
    assert got["enc_sine_pos_embed.pe"].shape == (8192, 128) and np.array_equal(got["enc_sine_pos_embed.pe"], sd["enc_sine_pos_embed.pe"][0, :8192])
    # an unknown key fails, a missing or mis-shaped one too
    bad = dict(state["model"])
    bad["encoder.pos_conv.0.bias"] = torch.zeros(128)
    with pytest.raises(ValueError, match="unexpected parameter encoder.pos_conv.0.bias"):
        load_mae_ast_checkpoint({"cfg": state["cfg"], "model": bad})
    bad = dict(state["model"])
    del bad["encoder.layers.2.fc1.bias"]
    with pytest.raises(ValueError, match="missing parameter encoder.layers.2.fc1.bias"):
        load_mae_ast_checkpoint({"cfg": state["cfg"], "model": bad})
    bad = dict(state["model"])
    bad["enc_sine_pos_embed.pe"] = torch.zeros(1, 100, 128)
    with pytest.raises(ValueError, match="enc_sine_pos_embed.pe has shape"):
        load_mae_ast_checkpoint({"cfg": state["cfg"], "model": bad})
    with pytest.raises(ValueError, match="required key: model is missing"):
        load_mae_ast_checkpoint({"cfg": state["cfg"]})
    with pytest.raises(ValueError, match="cfg.task has no 'sample_rate'"):
        load_mae_ast_checkpoint({"cfg": {"model": state["cfg"]["model"], "task": {"feature_dim": 128}}, "model": state["model"]})


# ---- hub names --------------------------------------------------------------------------------------------------------------------
def test_hub_names_have_the_reference_signatures():
    import s3prl_amd.hub as amd
    from s3prl_amd.upstream.mae_ast import hubconf

    ref = json.load(open(os.path.join(ROOT, "tests", "golden", "mae_ast", "reference_hub_mae_ast.json")))
    everything = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_hub.json")))["options"]
    checked = []
    for name, params in ref["hubconfs"]["mae_ast"]:
        assert name in everything and name in amd.options(), name
        ours = inspect.signature(getattr(amd, name))
        assert [list(p) for p in params] == [[k, v.kind.name, repr(v.default)] for k, v in ours.parameters.items()], name
        checked.append(name)
    assert sorted(checked) == ["mae_ast_frame", "mae_ast_local", "mae_ast_patch", "mae_ast_url"]
    assert {"mae_ast_frame", "mae_ast_patch"} <= set(amd.options(only_registered_ckpt=True))
    src = inspect.getsource(hubconf)
    for url in ("https://www.cs.utexas.edu/~harwath/model_checkpoints/mae_ast/random_frame_75_12LayerEncoder.pt",
                "https://www.cs.utexas.edu/~harwath/model_checkpoints/mae_ast/chunk_patch_75_12LayerEncoder.pt"):
        assert url in src
    assert [p[0] for p in ref["expert_init"]][:2] == ["self", "ckpt"]


def test_hub_name_is_served_from_the_cache_directory(tmp_path):
    import torch

    import s3prl_amd.hub as amd
    from s3prl_amd import download
    from s3prl_amd.ckpt import save_checkpoint
    from s3prl_amd.synth import named_config, synth_weights

    url = "https://www.cs.utexas.edu/~harwath/model_checkpoints/mae_ast/random_frame_75_12LayerEncoder.pt"
    cfg = named_config("tiny_mae_ast_frame")
    old = download.get_dir()
    download.set_dir(tmp_path)
    try:
        save_checkpoint(str(download.cache_path(url)), cfg, synth_weights(cfg, 3))
        expert = amd.mae_ast_frame()
        assert expert.cfg == cfg and expert.get_downsample_rates("hidden_states") == 320
        assert expert.num_layers == 2 and expert.hidden_sizes == [128, 128]
        assert amd.mae_ast_local(str(download.cache_path(url))).cfg == cfg
        with pytest.raises(RuntimeError, match="inference-only"):
            expert([torch.zeros(16000, requires_grad=True)])
        if not torch.cuda.is_available():
            with pytest.raises(RuntimeError, match="no CPU fallback"):
                expert([torch.zeros(16000)])
    finally:
        download.set_dir(old)


# ---- family constants and refusals --------------------------------------------------------------------------------------------------
def test_family_constant_and_the_c_block():
    from s3prl_amd import _lib
    from s3prl_amd.ckpt import mae_ast_hot_path
    from s3prl_amd.config import EncoderConfig
    from s3prl_amd.synth import named_config, synth_weights

    assert _lib.FAMILY["mae_ast"] == 13
    header = open(os.path.join(ROOT, "include", "s3enc.h")).read()
    assert "S3ENC_MAE_AST = 13" in header and "int s3enc_create_mae_ast(" in header and "int s3enc_op_patch_embed(" in header
    block = header[header.index("typedef struct s3enc_mae_ast_config {"):header.index("} s3enc_mae_ast_config;")]
    fields = [ln.split(";")[0].split()[-1] for ln in block.splitlines()[1:] if ";" in ln]
    assert fields == [f[0] for f in _lib.S3MaeAstConfig._fields_] == ["kt", "kc", "feature_dim", "bn_mean", "bn_var", "bn_eps", "pos_rows"]
    cfg = named_config("tiny_mae_ast_k3x32")
    again = EncoderConfig(**cfg.__dict__)
    again.validate()
    assert again == cfg
    w = mae_ast_hot_path("w", cfg, synth_weights(cfg, 2))
    c = _lib.make_mae_ast_config(cfg, w)
    assert (c.kt, c.kc, c.feature_dim, c.pos_rows) == (3, 32, 128, 640) and abs(c.bn_eps - 1e-5) < 1e-12
    assert c.bn_mean == float(w["batch_norm.running_mean"][0]) and c.bn_var == float(w["batch_norm.running_var"][0])
    cc = _lib.make_config(cfg, "fp32")
    assert (cc.family, cc.embed_dim, cc.heads, cc.ffn_dim, cc.encoder_layers, cc.layer_norm_first) == (13, 128, 2, 256, 2, 0)
    with pytest.raises(_lib.S3EncError, match="needs a mae_ast configuration"):
        _lib.make_mae_ast_config(named_config("tiny_byol_a"), w)


def test_python_side_refusals_by_message():
    from s3prl_amd.config import config_from_mae_ast, mae_ast_config

    tiny = dict(embed_dim=128, layers=2, heads=2, ffn=256, max_token_length=640)
    with pytest.raises(ValueError, match="enc_conv_pos=True is not built"):
        mae_ast_config(**tiny, ma_enc_conv_pos=True)
    with pytest.raises(ValueError, match=r"kernel stride \(8, 16\) must equal the kernel size \(16, 16\)"):
        mae_ast_config(**tiny, stride_t=8)
    with pytest.raises(ValueError, match=r"kernel stride \(16, 8\) must equal the kernel size \(16, 16\)"):
        mae_ast_config(**tiny, stride_c=8)
    with pytest.raises(ValueError, match="feature_dim must be 128"):
        mae_ast_config(**tiny, feature_dim=80)
    with pytest.raises(ValueError, match="ast_kernel_size_chan must be 16, 32, 64 or 128"):
        mae_ast_config(kt=16, kc=8, **tiny)
    with pytest.raises(ValueError, match="ast_kernel_size_chan must be 16, 32, 64 or 128"):
        mae_ast_config(kt=16, kc=48, **tiny)
    with pytest.raises(ValueError, match="ast_kernel_size_time must be 1..32"):
        mae_ast_config(kt=33, kc=16, **tiny)
    with pytest.raises(ValueError, match="sample_rate must be 16000, got 8000"):
        mae_ast_config(**tiny, sample_rate=8000)
    with pytest.raises(ValueError, match="must be 64 .the attention kernel's head width., got 128 / 4"):
        mae_ast_config(**{**tiny, "heads": 4})
    with pytest.raises(ValueError, match="activation_fn='relu' is not built"):
        mae_ast_config(**tiny, ma_activation="relu")
    with pytest.raises(ValueError, match="enc_sine_pos=False is not built"):
        config_from_mae_ast(dict(encoder_embed_dim=128, encoder_attention_heads=2), dict(feature_dim=128, sample_rate=16000))
