"""SSAST without a GPU: the float64 restatement tests/ssast_ref.py pinned piece by piece against torch in fp32 — nn.Conv2d for the
embedding, nn.TransformerEncoderLayer(norm_first, gelu, eps 1e-6) with in_proj = attn.qkv for a block, F.interpolate(bilinear) for
the position rule in both time branches — and its front end against oracle/fbank_oracle.py with the window swapped; the time-major
token order against the reference's f-major one; the cut; the fixtures against the restatement; the loader, the hub names, the
configuration refusals and the C block."""

import dataclasses
import inspect
import json
import os

import numpy as np
import pytest

from oracle import encoder_oracle as O
from oracle import fbank_oracle

import ssast_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SS_DIR = os.path.join(ROOT, "tests", "golden", "ssast")
FIXTURES = ["tiny_frame_cut", "tiny_frame_interp", "tiny_patch_cut", "tiny_patch_d192", "tiny_patch_eq", "tiny_patch_interp", "tiny_patch_short"]
FP32 = 2e-5  # an fp32 torch evaluation of a float64 formula at these sizes (K <= 256 sums, unit-scale values)


def _cfg_w(name="tiny_ssast_patch", seed=7):
    from s3prl_amd.synth import named_config, synth_weights

    cfg = named_config(name)
    return cfg, synth_weights(cfg, seed)


# ---- the restatement against torch ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tiny_ssast_patch", "tiny_ssast_frame"])
def test_embedding_against_conv2d(name):
    import torch

    cfg, w = _cfg_w(name)
    rng = np.random.default_rng(3)
    img = rng.standard_normal((cfg.ss_target_length, 128)).astype(np.float32)
    D = cfg.encoder_embed_dim
    conv = torch.nn.Conv2d(1, D, (cfg.ss_fshape, cfg.ss_tshape), stride=(cfg.ss_fstride, cfg.ss_tstride))
    with torch.no_grad():
        conv.weight.copy_(torch.from_numpy(w["module.v.patch_embed.proj.weight"]).sum(1, keepdim=True))
        conv.bias.copy_(torch.from_numpy(w["module.v.patch_embed.proj.bias"]))
        x = conv(torch.from_numpy(img).T[None, None])  # (1, D, f_dim, t_dim)
        assert tuple(x.shape[2:]) == (cfg.ss_f_dim, cfg.ss_t_dim)
        x = x.flatten(2).transpose(1, 2)[0]  # f-major tokens
        pre = torch.cat([torch.from_numpy(w["module.v.cls_token"])[0], torch.from_numpy(w["module.v.dist_token"])[0]])
        tok = torch.cat([pre, x]) + torch.from_numpy(R.position_rows(cfg, w).astype(np.float32))
    mine = R.embed(cfg, w, img.astype(np.float64))
    assert mine.shape == tuple(tok.shape) == (2 + cfg.ss_f_dim * cfg.ss_t_dim, D)
    assert max(O.rel_err(tok[i].numpy(), mine[i]) for i in range(len(mine))) < FP32


def test_block_against_transformer_encoder_layer():
    import torch

    cfg, w = _cfg_w()
    D, H, F = cfg.encoder_embed_dim, cfg.encoder_attention_heads, cfg.encoder_ffn_embed_dim
    layer = torch.nn.TransformerEncoderLayer(D, H, F, dropout=0.0, activation="gelu", layer_norm_eps=1e-6, batch_first=True, norm_first=True).eval()
    p = "module.v.blocks.1."
    t = lambda k: torch.from_numpy(w[p + k])
    with torch.no_grad():
        layer.self_attn.in_proj_weight.copy_(t("attn.qkv.weight"))
        layer.self_attn.in_proj_bias.copy_(t("attn.qkv.bias"))
        layer.self_attn.out_proj.weight.copy_(t("attn.proj.weight"))
        layer.self_attn.out_proj.bias.copy_(t("attn.proj.bias"))
        for mine, theirs in (("norm1", layer.norm1), ("norm2", layer.norm2), ("mlp.fc1", layer.linear1), ("mlp.fc2", layer.linear2)):
            theirs.weight.copy_(t(mine + ".weight"))
            theirs.bias.copy_(t(mine + ".bias"))
        x = torch.from_numpy(np.random.default_rng(4).standard_normal((1, 50, D)).astype(np.float32))
        want = layer(x)[0].numpy()
    got = R.block(x[0].numpy().astype(np.float64), w, "module.v.blocks.1", H)
    assert max(O.rel_err(want[i], got[i]) for i in range(50)) < FP32
    assert max(O.rel_err(want[i], R.block(x[0].numpy().astype(np.float64), w, "module.v.blocks.1", H, eps=1e-2)[i]) for i in range(50)) > 1e-3


def _torch_position_rule(pe, pf, pt, f_dim, t_dim):
    """the rule of ast_models.py:303-342 with torch's own interpolation, fp32"""
    import torch
    import torch.nn.functional as F

    D = pe.shape[1]
    g = torch.from_numpy(pe[2:].astype(np.float32)).reshape(1, pf * pt, D).transpose(1, 2).reshape(1, D, pf, pt)
    if t_dim < pt:
        lo = int(pt / 2) - int(t_dim / 2)
        g = g[:, :, :, lo:lo + t_dim]
    else:
        g = F.interpolate(g, size=(8, t_dim), mode="bilinear")
    g = F.interpolate(g, size=(f_dim, t_dim), mode="bilinear")
    return g.reshape(1, D, f_dim * t_dim).transpose(1, 2)[0].numpy()


@pytest.mark.parametrize("model_type, p_input_tdim", [("p", 1024), ("p", 80), ("p", 64), ("p", 48), ("p", 16),  # p_t_dim 64, 5, 4, 3, 1 around t_dim 4
                                                       ("f", 1024), ("f", 100), ("f", 98), ("f", 96), ("f", 60)])  # 512, 50, 49, 48, 30 around 49
def test_position_rule_against_interpolate_in_both_time_branches(model_type, p_input_tdim):
    from s3prl_amd.ckpt import ssast_hot_path
    from s3prl_amd.config import ssast_config
    from s3prl_amd.synth import synth_weights

    cfg = ssast_config(model_type=model_type, embed_dim=128, heads=2, layers=1, window_secs=0.5, p_input_tdim=p_input_tdim)
    w = synth_weights(cfg, 11)
    pf, pt = cfg.ss_pretrain_grid
    f_dim, t_dim = cfg.ss_f_dim, cfg.ss_t_dim
    want = _torch_position_rule(w["module.v.pos_embed"][0], pf, pt, f_dim, t_dim)
    mine = R.position_rows(cfg, w)
    assert np.array_equal(mine[:2], w["module.v.pos_embed"][0, :2].astype(np.float64))
    # torch computes the source coordinate (j + 0.5) * (in / out) - 0.5 in fp32: at coordinates below 64 each of its three roundings is
    # at most ulp(64) / 2 = 3.8e-6, so the interpolation weight is within 1.2e-5 of the exact one, times a neighbour difference below 3
    assert np.abs(mine[2:] - want).max() < 4e-5 and np.abs(np.diff(w["module.v.pos_embed"][0, 2:], axis=0)).max() < 3.0
    if t_dim < pt:  # the centre cut moves values, it computes none
        assert np.array_equal(R.bilinear(np.ones((1, pf, t_dim)), f_dim, t_dim), np.ones((1, f_dim, t_dim)))
    # the loader's rows: the same values, permuted to the handle's time-major order, and the prefix fold
    hot = ssast_hot_path("w", cfg, w)
    tm = mine[2:].reshape(f_dim, t_dim, -1).transpose(1, 0, 2).reshape(t_dim * f_dim, -1)
    assert np.abs(hot["pos"] - tm).max() < 1e-6
    D = cfg.encoder_embed_dim
    assert np.allclose(hot["prefix"][0], w["module.v.cls_token"].reshape(D) + w["module.v.pos_embed"][0, 0], atol=1e-7)
    assert np.allclose(hot["prefix"][1], w["module.v.dist_token"].reshape(D) + w["module.v.pos_embed"][0, 1], atol=1e-7)
    want_w = w["module.v.patch_embed.proj.weight"].sum(1).transpose(0, 2, 1).reshape(D, -1)
    assert np.array_equal(hot["patch.weight"], want_w) and hot["patch.weight"].shape == (D, 256)


def test_the_frequency_cut_branch_is_refused():
    from s3prl_amd.ckpt import ssast_position_rows
    from s3prl_amd.config import ssast_config

    with pytest.raises(ValueError, match="f_dim 12 < p_f_dim 16: the reference's frequency cut"):
        ssast_config(model_type="p", embed_dim=128, heads=2, layers=1, p_input_fdim=256)
    with pytest.raises(ValueError, match="f_dim 12 < p_f_dim 16"):
        ssast_position_rows(np.zeros((16 * 4, 8)), 16, 4, 12, 4)
    cfg, w = _cfg_w()
    with pytest.raises(ValueError, match="f_dim < p_f_dim"):
        R._position_rows(np.zeros((2 + 64, 8)), 16, 4, 12, 4)


# ---- front end -----------------------------------------------------------------------------------------------------------------------
def test_front_end_against_the_fbank_oracle_with_the_window_swapped(monkeypatch):
    monkeypatch.setattr(fbank_oracle, "povey_window", lambda n: 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n, dtype=np.float64) / (n - 1)))
    x = np.random.default_rng(5).standard_normal(8000)
    want = fbank_oracle.kaldi_fbank(x, num_mel_bins=128)
    got = R.fbank_hanning(x)
    assert got.shape == want.shape == (48, 128) and np.abs(got - want).max() < 1e-9
    assert np.abs(R.hanning(400)[[0, 399]]).max() < 1e-15 and abs(R.hanning(401)[200] - 1.0) < 1e-15


def test_the_silent_windows_constant_and_the_exact_zero_rows():
    cfg, _ = _cfg_w()
    img = R.window_image(cfg, np.zeros(cfg.ss_window_samples))
    Fw = 1 + (cfg.ss_window_samples - 400) // 160
    assert Fw == 48 < cfg.ss_target_length == 50
    const = (np.log(np.float64(np.finfo(np.float32).eps)) + np.float64(np.float32(4.2677393))) / np.float64(np.float32(4.5689974 * 2))
    assert np.all(img[:Fw] == const) and abs(const + 1.2774) < 1e-3
    assert not img[Fw:].any()
    live = R.window_image(cfg, np.random.default_rng(6).standard_normal(cfg.ss_window_samples))
    assert not live[Fw:].any() and np.abs(live[:Fw]).min() > 0
    short = R.window_image(cfg, np.concatenate([np.ones(300), np.zeros(cfg.ss_window_samples - 300)]))  # an utterance under 400 samples
    assert np.isfinite(short).all() and not np.all(short[:3] == const) and np.all(short[3:Fw] == const)


def test_windows_are_zero_padded_to_whole_windows():
    cfg, _ = _cfg_w()
    W = cfg.ss_window_samples
    wavs = [np.ones(2 * W + 1), np.ones(5)]
    win = R.windows(cfg, wavs)
    assert win.shape == (2, 3, W) and win[0, 2].sum() == 1 and win[1].sum() == 5 and not win[1, 1:].any()


# ---- token order and cut -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tiny_ssast_patch", "tiny_ssast_frame"])
def test_the_time_major_token_order_returns_the_same_states(name):
    from s3prl_amd.synth import synth_wavs

    cfg, w = _cfg_w(name)
    wavs = synth_wavs([8001, 3000], 8)
    a = R.forward(cfg, w, wavs)
    b = R.forward(cfg, w, wavs, time_major=True)
    assert all(np.abs(x - y).max() < 1e-12 * np.abs(x).max() for x, y in zip(a["states"], b["states"]))
    if cfg.ss_f_dim > 1:
        assert not np.array_equal(a["tokens"], b["tokens"])
    t0 = a["tokens"][0, 0, 2:].reshape(cfg.ss_f_dim, cfg.ss_t_dim, -1).transpose(1, 0, 2).reshape(-1, a["tokens"].shape[-1])
    assert np.array_equal(t0, b["tokens"][0, 0, 2:]) and np.array_equal(a["tokens"][0, 0, :2], b["tokens"][0, 0, :2])


@pytest.mark.parametrize("name, want", [("tiny_ssast_patch", [4, 4, 6, 8, 11]), ("tiny_ssast_frame", [49, 49, 51, 98, 101]),
                                        ("ssast_patch_base_l2", [9, 9, 11, 18, 21]), ("ssast_frame_base_l2", [99, 99, 101, 198, 201])])
def test_the_cut(name, want):
    from s3prl_amd.synth import named_config

    cfg = named_config(name)
    W = cfg.ss_window_samples
    lens = [W - 1, W, W + 1, 2 * W, 2 * W + 1]
    assert [cfg.num_frames(n) for n in lens] == [R.num_steps(cfg, n) for n in lens] == want
    assert [cfg.ss_num_windows(n) for n in lens] == [1, 1, 2, 2, 3]
    assert cfg.valid_frames(1, 2 * W + 1) == 1 and cfg.valid_frames(2 * W + 1, 2 * W + 1) == want[-1]
    assert cfg.downsample_rate == 160 * cfg.ss_tstride and cfg.num_hidden_states == cfg.encoder_layers


def test_geometry_of_the_released_models():
    from s3prl_amd.synth import named_config

    p, f = named_config("ssast_patch_base"), named_config("ssast_frame_base")
    assert (p.ss_f_dim, p.ss_t_dim, p.ss_pretrain_grid, p.ss_f_dim * p.encoder_embed_dim) == (12, 9, (8, 64), 9216)
    assert (f.ss_f_dim, f.ss_t_dim, f.ss_pretrain_grid, f.ss_f_dim * f.encoder_embed_dim) == (1, 99, (1, 512), 768)
    from s3prl_amd.config import ssast_config

    ten = ssast_config("p", window_secs=10.0), ssast_config("f", window_secs=10.0)
    assert [2 + c.ss_f_dim * c.ss_t_dim for c in ten] == [1190, 1001]
    assert [2 + c.ss_f_dim * c.ss_t_dim for c in (p, f)] == [110, 101]


# ---- fixtures ------------------------------------------------------------------------------------------------------------------------
def test_fixture_list():
    files = sorted(os.listdir(SS_DIR))
    assert [f for f in files if f.endswith(".npz")] == sorted(f"{n}.npz" for n in FIXTURES) and "reference_hub_ssast.json" in files
    assert all(os.path.getsize(os.path.join(SS_DIR, f)) < 256 * 1024 for f in files)


@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_is_the_restatements_output(name, golden_loader):
    meta, cfg, weights, wavs, hs, norms = golden_loader("ssast/" + name)
    res = R.forward(cfg, weights, wavs)["states"]
    ts, cs = meta["t_stride"], meta["c_stride"]
    assert len(hs) == cfg.encoder_layers and list(res[0].shape) == meta["shape"] and meta["steps"] == cfg.num_frames(max(meta["lengths"]))
    for l, h in enumerate(hs):
        assert O.rel_err(h, res[l][:, ::ts, ::cs]) < 1e-6 and abs(np.linalg.norm(res[l]) - norms[l]) / norms[l] < 1e-9
    assert "no run of the reference" in meta["reference"]


# ---- loader --------------------------------------------------------------------------------------------------------------------------
def test_checkpoint_file_round_trip_and_refusals(tmp_path):
    import torch

    from s3prl_amd.ckpt import SSAST_UNUSED, load_ssast_checkpoint, save_checkpoint, ssast_hot_path
    from s3prl_amd.config import ssast_config
    from s3prl_amd.synth import synth_weights

    cfg = ssast_config(model_type="p", model_size="tiny", layers=2, window_secs=0.5)
    w = synth_weights(cfg, 9)
    assert {"module.p_input_fdim", "module.p_input_tdim", "module.mask_embed", "module.cpredlayer.0.weight", "module.gpredlayer.2.bias",
            "module.v.norm.weight", "module.v.head_dist.weight"} <= set(w)
    path = str(tmp_path / "ssast.pth")
    save_checkpoint(path, cfg, w)
    state = torch.load(path, map_location="cpu", weights_only=False)
    assert state["module.p_input_tdim"].shape == () and int(state["module.p_input_tdim"]) == 1024
    got_cfg, got = load_ssast_checkpoint(path, "tiny_p", 0.5)
    assert got_cfg == cfg and not any(k.startswith(SSAST_UNUSED) for k in got)
    a, b = ssast_hot_path("w", cfg, w), ssast_hot_path("w", got_cfg, got)
    assert set(a) == set(b) and all(np.array_equal(a[k], b[k]) for k in a)
    assert set(a) == {"patch.weight", "patch.bias", "prefix", "pos"} | {f"blocks.{l}.{n}.{p}" for l in range(2) for p in ("weight", "bias")
                                                                         for n in ("norm1", "attn.qkv", "attn.proj", "norm2", "mlp.fc1", "mlp.fc2")}
    assert ssast_hot_path("w", cfg, a) is not a and set(ssast_hot_path("w", cfg, a)) == set(a)  # a prepared set passes through
    with pytest.raises(ValueError, match="model size 'base' is 768 wide"):
        load_ssast_checkpoint(state, "base_p", 0.5)
    with pytest.raises(ValueError, match="model_size must be"):
        load_ssast_checkpoint(state, "huge_p", 0.5)
    bad = dict(state)
    del bad["module.p_input_fdim"]
    with pytest.raises(ValueError, match="required key: module.p_input_fdim is missing"):
        load_ssast_checkpoint(bad, "tiny_p", 0.5)
    bad = dict(state)
    del bad["module.v.blocks.1.mlp.fc1.bias"]
    with pytest.raises(ValueError, match="missing parameter module.v.blocks.1.mlp.fc1.bias"):
        load_ssast_checkpoint(bad, "tiny_p", 0.5)
    bad = dict(state)
    bad["module.v.surprise"] = torch.zeros(1)
    with pytest.raises(ValueError, match="unexpected parameter module.v.surprise"):
        load_ssast_checkpoint(bad, "tiny_p", 0.5)
    bad = dict(state)
    bad["module.v.pos_embed"] = torch.zeros(1, 100, 192)
    with pytest.raises(ValueError, match="module.v.pos_embed has shape"):
        load_ssast_checkpoint(bad, "tiny_p", 0.5)
    with pytest.raises(ValueError, match="patch_embed.proj.weight has shape"):
        load_ssast_checkpoint(state, "tiny_f", 0.5)


# ---- hub names -----------------------------------------------------------------------------------------------------------------------
def test_hub_names_have_the_reference_signatures():
    import s3prl_amd.hub as amd
    from s3prl_amd.upstream.ssast import hubconf
    from s3prl_amd.upstream.ssast.expert import UpstreamExpert

    ref = json.load(open(os.path.join(SS_DIR, "reference_hub_ssast.json")))
    everything = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_hub.json")))["options"]
    checked = []
    for name, params in ref["hubconfs"]["ssast"]:
        assert name in everything and name in amd.options(), name
        ours = inspect.signature(getattr(amd, name))
        assert [list(p) for p in params] == [[k, v.kind.name, repr(v.default)] for k, v in ours.parameters.items()], name
        assert ref["urls"][name] in inspect.getsource(getattr(hubconf, name))
        checked.append(name)
    assert sorted(checked) == ["ssast_frame_base", "ssast_patch_base"] and set(checked) <= set(amd.options(only_registered_ckpt=True))
    ours = [[k, v.kind.name, repr(v.default)] for k, v in inspect.signature(UpstreamExpert.__init__).parameters.items()]
    assert ours[:len(ref["expert_init"])] == [list(p) for p in ref["expert_init"]]  # (then dtype and **kwargs, this package's additions)


def test_hub_name_is_served_from_the_cache_directory(tmp_path):
    import torch

    import s3prl_amd.hub as amd
    from s3prl_amd import download
    from s3prl_amd.ckpt import save_checkpoint
    from s3prl_amd.config import ssast_config
    from s3prl_amd.synth import synth_weights

    url = "https://www.dropbox.com/s/nx6nl4d4bl71sm8/SSAST-Base-Frame-400.pth?dl=1"
    cfg = ssast_config(model_type="f", layers=1, window_secs=0.5)
    old = download.get_dir()
    download.set_dir(tmp_path)
    try:
        save_checkpoint(str(download.cache_path(url)), cfg, synth_weights(cfg, 3))
        expert = amd.ssast_frame_base(window_secs=0.5)
        assert expert.cfg == cfg and expert.get_downsample_rates("hidden_states") == 160 and expert.window_secs == 0.5
        assert expert.num_layers == 1 and expert.hidden_sizes == [768]
        with pytest.raises(RuntimeError, match="inference-only"):
            expert([torch.zeros(16000, requires_grad=True)])
        if not torch.cuda.is_available():
            with pytest.raises(RuntimeError, match="no CPU fallback"):
                expert([torch.zeros(16000)])
    finally:
        download.set_dir(old)


# ---- family constants and refusals ---------------------------------------------------------------------------------------------------
def test_family_constant_and_the_c_block():
    from s3prl_amd import _lib
    from s3prl_amd.config import EncoderConfig
    from s3prl_amd.synth import named_config

    assert _lib.FAMILY["ssast"] == 18 and _lib.BLOCK_FAMILIES["ssast"].create == "s3enc_create_ssast"
    header = open(os.path.join(ROOT, "include", "s3enc.h")).read()
    assert "S3ENC_SSAST = 18" in header and "int s3enc_create_ssast(" in header and "int s3enc_op_patch_embed_strided(" in header
    block = header[header.index("typedef struct s3enc_ssast_config {"):header.index("} s3enc_ssast_config;")]
    fields = [ln.split(";")[0].split()[-1] for ln in block.splitlines()[1:] if ";" in ln]
    assert fields == [f[0] for f in _lib.S3SsastConfig._fields_] == ["fshape", "tshape", "fstride", "tstride", "window_samples",
                                                                     "target_length", "ln_eps", "pos_rows"]
    cfg = named_config("tiny_ssast_frame")
    again = EncoderConfig(**cfg.__dict__)
    again.validate()
    assert again == cfg
    c = _lib.make_ssast_config(cfg)
    assert (c.fshape, c.tshape, c.fstride, c.tstride, c.window_samples, c.target_length, c.pos_rows) == (128, 2, 128, 1, 8000, 50, 49)
    assert abs(c.ln_eps - 1e-6) < 1e-12
    cc = _lib.make_config(cfg, "fp32")
    assert (cc.family, cc.embed_dim, cc.heads, cc.ffn_dim, cc.encoder_layers, cc.layer_norm_first) == (18, 128, 2, 512, 2, 1)
    with pytest.raises(_lib.S3EncError, match="needs an ssast configuration"):
        _lib.make_ssast_config(named_config("tiny_byol_a"))
    lib = _lib.load()  # the new tuning keys, without a GPU
    for key, lo, hi in ((b"patch_strided_fused", 0, 1), (b"ssast_chunk", 1, 1 << 22)):
        assert lib.s3enc_set_tuning(key, hi + 1) != 0 and f"{key.decode()} must be {lo}..{hi}" in lib.s3enc_last_error().decode()
    assert lib.s3enc_set_tuning(b"patch_strided_fused", 1) == 0 and lib.s3enc_set_tuning(b"ssast_chunk", 65536) == 0


def test_python_side_refusals_by_message():
    from s3prl_amd.config import ssast_config

    tiny = dict(embed_dim=128, heads=2, layers=2)
    with pytest.raises(ValueError, match="model type must be 'p' or 'f'"):
        ssast_config(model_type="x", **tiny)
    with pytest.raises(ValueError, match="model size must be one of"):
        ssast_config(model_size="base_nokd")
    with pytest.raises(ValueError, match="must be 64 .the attention kernel's head width., got 128 / 4"):
        ssast_config(**{**tiny, "heads": 4})
    with pytest.raises(ValueError, match="gives 160 samples: a window must be a multiple of 4 samples and hold at least one 400-sample"):
        ssast_config(window_secs=0.01, **tiny)
    with pytest.raises(ValueError, match="gives 4001 samples: a window must be a multiple of 4"):
        ssast_config(window_secs=0.2500625, **tiny)
    with pytest.raises(ValueError, match="gives 10 image rows, fewer than one patch of 16 frames"):
        ssast_config(window_secs=0.1, **tiny)
    with pytest.raises(ValueError, match="fstride must be even"):
        dataclasses.replace(ssast_config(**tiny), ss_fstride=9).validate()
    with pytest.raises(ValueError, match="blocks are pre-LN"):
        dataclasses.replace(ssast_config(**tiny), layer_norm_first=False).validate()
    with pytest.raises(ValueError, match="more than 8192 tokens"):
        ssast_config(model_type="p", window_secs=80.0, **tiny)
