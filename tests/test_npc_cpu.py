"""NPC without a GPU: the float64 restatement of tests/npc_ref.py against every reference-generated fixture on ALL rows (the
reference masks nothing: the rows behind an utterance's frames are its values, not zeros), the state count and order, the frame
arithmetic, checkpoint reading (a wrong ``conv_mask`` included), the refusals by name (Python and s3enc_create_npc), the
configuration block against the header, the op entry's argument checks and the hub names."""

import ctypes as C
import inspect
import json
import os
import re

import numpy as np
import pytest

from oracle import encoder_oracle as O
from oracle import fbank_oracle as FO

import npc_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NAMES = ["npc_tiny_pad", "npc_tiny_eq", "npc_tiny_plain", "npc_tiny_t1", "npc_tiny_last", "npc_tiny_k9", "npc_360hr_pseudo"]
FIXTURES = ["npc/" + n for n in NAMES]
REF_PIN = 1e-6  # the project's restatement bound: a float64 restatement against the reference's fp32 outputs


@pytest.fixture(scope="module")
def restated(golden_loader):
    """npc_ref's float64 forward of every fixture, computed once"""
    cache = {}

    def get(name):
        if name not in cache:
            meta, cfg, weights, wavs, hs, norms = golden_loader(name)
            feats, lens = R.features(cfg, wavs)
            # the generator fed the reference these features ROUNDED TO fp32
            cache[name] = (R.model(cfg, weights, feats.astype(np.float32)), lens)
        return cache[name]

    return get


@pytest.mark.parametrize("name", FIXTURES)
def test_float64_restatement_matches_the_reference_on_all_rows(name, golden_loader, restated):
    meta, cfg, weights, wavs, hs, norms = golden_loader(name)
    out, lens = restated(name)
    NB = cfg.npc_blocks
    want_states = NB + 2 if cfg.npc_disable_cross_layer else 2 * NB + 1
    assert len(hs) == cfg.num_hidden_states == want_states == meta["n_states"] == len(out["hidden_states"])
    assert lens == meta["frames"] == [cfg.num_frames(n) for n in meta["lengths"]]
    ts, cs = meta["t_stride"], meta["c_stride"]
    assert meta["shape"] == [len(wavs), cfg.num_frames(max(meta["lengths"])), cfg.conv_dim]
    assert out["kinds"] == meta["kinds"]
    for l, h in enumerate(out["hidden_states"]):
        assert list(h.shape) == meta["shape"]
        assert O.rel_err(h[:, ::ts, ::cs], hs[l]) <= REF_PIN, (name, l)
        assert abs(np.linalg.norm(h) - norms[l]) / norms[l] <= REF_PIN
        for b in range(len(wavs)):  # per utterance, padded rows included; and the padded rows on their own
            assert O.rel_err(h[b, ::ts, ::cs], hs[l][b]) <= REF_PIN, (name, l, b)
            if lens[b] < h.shape[1] and ts == 1:
                assert O.rel_err(h[b, lens[b]:, ::cs], hs[l][b, lens[b]:]) <= REF_PIN, (name, l, b)
    assert max(meta["ref_fp32_err"]) <= 8e-7 and max(meta["fp32_proxy_err"]) <= 0.25e-4
    assert max(meta["saturated"]) <= 0.15 and min(meta["masked_std"]) >= 0.4
    if cfg.npc_activate == "relu":
        assert 0.2 <= min(meta["relu_zeros"]) and max(meta["relu_zeros"]) <= 0.7


@pytest.mark.parametrize("name", ["npc/npc_tiny_pad", "npc/npc_tiny_plain", "npc/npc_tiny_t1", "npc/npc_360hr_pseudo"])
def test_rows_behind_an_utterance_are_loud_from_state_0_on(name, golden_loader, restated):
    """No length masking: the feature rows behind an utterance are zeros, bias and BatchNorm make every state's rows there non-zero,
    in the reference's outputs and in the restatement alike."""
    meta, cfg, weights, wavs, hs, norms = golden_loader(name)
    out, lens = restated(name)
    T = meta["shape"][1]
    short = [b for b, n in enumerate(lens) if n < T]
    assert short and meta["pad_row_norm"] and min(meta["pad_row_norm"]) > 0.5
    for l, h in enumerate(out["hidden_states"]):
        for b in short:
            assert np.linalg.norm(h[b, lens[b]:]) > 0.1 and np.linalg.norm(hs[l][b, -(-lens[b] // meta["t_stride"]):]) > 0.1, (l, b)


def test_an_utterances_rows_depend_on_T_and_on_nothing_else_of_the_batch():
    from s3prl_amd.synth import named_config, synth_wavs, synth_weights

    cfg = named_config("tiny_npc")
    weights = synth_weights(cfg, 3)
    wavs = synth_wavs([4000, 2345, 3111], 5)
    feats, lens = R.features(cfg, wavs)
    full = R.model(cfg, weights, feats)["hidden_states"]
    alone = R.model(cfg, weights, feats[1:2])["hidden_states"]  # padded to the batch's T
    own = R.model(cfg, weights, feats[1:2, :lens[1]])["hidden_states"]  # at its own T
    for l, (a, b, c) in enumerate(zip(full, alone, own)):
        assert np.array_equal(a[1], b[0])
        # block 0 reads zero feature rows either way; from the first masked conv on the loud padded rows reach the last valid frames
        diff = np.abs(a[1, :lens[1]] - c[0]).max(axis=1)
        assert (diff.max() > 1e-3) == (l > 0), l
        assert diff[:lens[1] - cfg.npc_blocks - 7].max() < 1e-12  # ... and only the last n_blocks + 7 of them


def test_state_count_and_order():
    from s3prl_amd.synth import named_config
    from s3prl_amd.upstream.npc.expert import UpstreamExpert

    c = named_config("tiny_npc")
    assert R.state_names(c) == ["self.model.blocks[0]", "self.model.masked_convs[0]", "self.model.blocks[1]", "self.model.masked_convs[1]",
                                "self.model.blocks[2]", "self.model.masked_convs[2]", "self.model.blocks[3]", "self.model.masked_convs[3]",
                                "self.model"]
    d = named_config("tiny_npc_last")
    assert R.state_names(d) == [f"self.model.blocks[{i}]" for i in range(4)] + ["self.model.masked_convs[3]", "self.model"]
    assert (c.num_hidden_states, d.num_hidden_states, named_config("tiny_npc_k9").num_hidden_states) == (9, 6, 7)
    e = UpstreamExpert.__new__(UpstreamExpert)
    for cfg in (c, d):
        e.__dict__["cfg"] = cfg
        assert list(UpstreamExpert._states_info(e, cfg.num_hidden_states)) == R.state_names(cfg)
    assert [c.npc_mask(i) for i in range(4)] == [7, 9, 11, 13] and [len(R.live_taps(15, c.npc_mask(i))) for i in range(4)] == [8, 6, 4, 2]
    k9 = named_config("tiny_npc_k9")
    assert [len(R.live_taps(9, k9.npc_mask(i))) for i in range(3)] == [6, 4, 2]
    assert R.live_taps(15, 13) == [0, 14] and R.live_taps(15, 7) == [0, 1, 2, 3, 11, 12, 13, 14]


def test_disable_cross_layer_repeats_the_last_masked_state(golden_loader):
    meta, cfg, weights, wavs, hs, norms = golden_loader("npc/npc_tiny_last")
    assert cfg.npc_disable_cross_layer and len(hs) == cfg.npc_blocks + 2
    assert np.array_equal(hs[-1], hs[-2]) and norms[-1] == norms[-2]


def test_fixture_table():
    """The fixtures the issue names: configurations, lengths, frames."""
    from conftest import golden_meta

    from s3prl_amd.synth import named_config

    L3 = [4000, 2345, 3111]
    want = {"npc_tiny_pad": ("tiny_npc", L3, 23), "npc_tiny_eq": ("tiny_npc", [3200, 3200], 18),
            "npc_tiny_plain": ("tiny_npc_plain", L3, 23), "npc_tiny_t1": ("tiny_npc_nocmvn", [400, 2000], 11),
            "npc_tiny_last": ("tiny_npc_last", L3, 23), "npc_tiny_k9": ("tiny_npc_k9", L3, 23),
            "npc_360hr_pseudo": ("npc_360hr", [16000, 12345], 98)}
    assert sorted(want) == sorted(NAMES)
    for name, (cfg, lengths, T) in want.items():
        m = golden_meta("npc/" + name)
        assert (m["config"], m["lengths"], m["shape"][1]) == (cfg, lengths, T), name
        assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "npc", name + ".npz")) < 256 * 1024
    assert golden_meta("npc/npc_tiny_t1")["frames"] == [1, 11]  # one utterance of exactly one frame
    assert len(set(golden_meta("npc/npc_tiny_pad")["frames"])) == 3 and len(set(golden_meta("npc/npc_tiny_eq")["frames"])) == 1
    c = named_config("npc_360hr")
    assert (c.conv_dim, c.npc_blocks, c.npc_kernel_size, c.npc_mask_size, c.npc_residual, c.npc_batch_norm, c.npc_activate,
            c.npc_disable_cross_layer, c.apc_feat_dim, c.apc_window, c.apc_cmvn) == (512, 4, 15, 5, True, True, "relu", False, 80,
                                                                                    "hamming", True)
    assert c.npc_vq == dict(codebook_size=[64] * 4, code_dim=[128] * 4, gumbel_temperature=1.0)
    p = named_config("tiny_npc_plain")
    assert (p.npc_batch_norm, p.npc_activate, p.npc_residual) == (False, "tanh", False)
    k9 = named_config("tiny_npc_k9")
    assert (k9.npc_kernel_size, k9.npc_mask_size, k9.npc_blocks) == (9, 1, 3)
    assert named_config("tiny_npc").conv_dim == 64 and named_config("tiny_npc").npc_vq is not None


def test_conv1d_restatement_matches_torch_in_float64():
    import torch

    rng = np.random.default_rng(0)
    x, w, b = rng.standard_normal((2, 9, 16)), rng.standard_normal((8, 16, 15)), rng.standard_normal(8)
    for mask in (0, 7, 13):
        live = R.live_taps(15, mask)
        wm = w.copy()
        wm[:, :, [j for j in range(15) if j not in live]] = 0
        want = torch.nn.functional.conv1d(torch.from_numpy(x).transpose(1, 2), torch.from_numpy(wm), torch.from_numpy(b), padding=7)
        got = R.conv1d(x, w, b, live)
        assert np.abs(got - want.transpose(1, 2).numpy()).max() <= 1e-12


@pytest.mark.parametrize("n, T", [(160000, 998), (16000, 98), (4000, 23), (1200, 6), (400, 1), (399, 0)])
def test_frame_arithmetic(n, T):
    from s3prl_amd.synth import named_config

    for name in ("tiny_npc", "tiny_npc_last", "npc_360hr"):
        cfg = named_config(name)
        assert cfg.num_frames(n) == T == FO.num_frames(n) and cfg.num_output_frames(n) == T
        assert cfg.valid_frames(n, 160000) == T and cfg.downsample_rate == 160
    assert named_config("tiny_npc").valid_frames(2345, 4000) == 13  # the utterance's own frames; the rows behind them are not zeros


# ---- checkpoints -----------------------------------------------------------------------------------------------------------
def _config(audio=None, paras=None):
    a = dict(feat_type="fbank", feat_dim=16, frame_length=25, frame_shift=10, decode_wav=False, cmvn=True)
    a.update(audio or {})
    p = dict(kernel_size=15, mask_size=5, n_blocks=4, hidden_size=64, dropout=0.1, residual=True, batch_norm=True, activate="relu",
             disable_cross_layer=False)
    p.update(paras or {})
    return {"data": {"audio": {k: v for k, v in a.items() if v is not None}}, "model": {"paras": {k: v for k, v in p.items() if v is not None}}}


def _save(tmp_path, config, weights_of="tiny_npc", drop=None, extra=None):
    import torch

    from s3prl_amd.synth import named_config, synth_weights

    sd = {k: torch.from_numpy(v) for k, v in synth_weights(named_config(weights_of), 3).items() if k != drop}
    sd.update(extra or {})
    path = str(tmp_path / "c.pt")
    torch.save({"config": config, "model": sd}, path)
    return path


def _mask(H, k, m):
    import torch

    t = torch.ones(H, H, k)
    t[:, :, (k - m) // 2:(k - m) // 2 + m] = 0
    return t


def test_checkpoint_round_trip(tmp_path):
    import torch

    from s3prl_amd.ckpt import load_checkpoint, load_npc_checkpoint, save_checkpoint
    from s3prl_amd.config import config_from_npc
    from s3prl_amd.synth import named_config, synth_weights

    d = config_from_npc(_config(audio=dict(frame_length=None, frame_shift=None, cmvn=None, decode_wav=None),
                                paras=dict(batch_norm=None, activate=None, disable_cross_layer=None)))  # the defaults of both sides
    assert (d.apc_frame_length, d.apc_frame_shift, d.apc_cmvn, d.conv_layers) == (25.0, 10.0, True, [(64, 400, 160)])
    assert (d.npc_batch_norm, d.npc_activate, d.npc_disable_cross_layer, d.encoder_layers) == (True, "relu", False, 8)
    for name in ("tiny_npc", "tiny_npc_plain", "tiny_npc_nocmvn", "tiny_npc_last", "tiny_npc_k9", "npc_360hr"):
        cfg = named_config(name)
        weights = synth_weights(cfg, 5)
        masked = sum(cfg.npc_has_mask(i) for i in range(cfg.npc_blocks))
        assert len(weights) == cfg.npc_blocks * (12 if cfg.npc_batch_norm else 4) + 2 * masked
        path = str(tmp_path / "c.pt")
        save_checkpoint(path, cfg, weights)
        state = torch.load(path, map_location="cpu", weights_only=False)
        assert set(state) == {"config", "model"} and set(state["config"]) == {"data", "model"}  # npc/expert.py:22-26
        # what the reference's state_dict carries beside the hot path is accepted and left in the file
        state["model"]["postnet.weight"] = torch.zeros(cfg.apc_feat_dim, cfg.conv_dim)
        state["model"]["postnet.bias"] = torch.zeros(cfg.apc_feat_dim)
        state["model"]["vq_layers.0.vq_logits.weight"] = torch.zeros(32, cfg.conv_dim)
        state["model"]["blocks.0.bn1.num_batches_tracked"] = torch.tensor(7)
        for i in range(cfg.npc_blocks):
            if cfg.npc_has_mask(i):
                state["model"][f"masked_convs.{i}.conv_mask"] = _mask(cfg.conv_dim, cfg.npc_kernel_size, cfg.npc_mask(i))
        torch.save(state, path)
        cfg2, back = load_npc_checkpoint(path)
        assert cfg2 == cfg and load_checkpoint(path, "npc")[0] == cfg
        assert set(back) == set(weights) and all(np.array_equal(back[k], weights[k]) for k in weights)


def test_a_wrong_conv_mask_is_refused_by_name(tmp_path):
    from s3prl_amd.ckpt import load_npc_checkpoint

    good = {f"masked_convs.{i}.conv_mask": _mask(64, 15, 7 + 2 * i) for i in range(4)}
    load_npc_checkpoint(_save(tmp_path, _config(), extra=good))
    for bad in (_mask(64, 15, 9), _mask(64, 15, 0), _mask(64, 15, 11)[:, :, :13]):
        with pytest.raises(ValueError, match=re.escape("masked_convs.2.conv_mask is not the mask of kernel_size 15 / mask_size 5")):
            load_npc_checkpoint(_save(tmp_path, _config(), extra=dict(good, **{"masked_convs.2.conv_mask": bad})))
    one = _mask(64, 15, 11)
    one[3, 5, 0] = 0  # a single weight masked beyond the hole
    with pytest.raises(ValueError, match="masked_convs.2.conv_mask"):
        load_npc_checkpoint(_save(tmp_path, _config(), extra=dict(good, **{"masked_convs.2.conv_mask": one})))


@pytest.mark.parametrize("drop", ["blocks.0.conv.weight", "blocks.1.linear.bias", "blocks.2.bn1.running_mean", "blocks.3.bn2.running_var",
                                  "blocks.0.bn2.weight", "masked_convs.0.conv.weight", "masked_convs.3.conv.bias"])
def test_a_missing_tensor_raises(tmp_path, drop):
    from s3prl_amd.ckpt import load_npc_checkpoint

    with pytest.raises(ValueError, match=re.escape(drop)):
        load_npc_checkpoint(_save(tmp_path, _config(), drop=drop))


def test_missing_keys_are_named(tmp_path):
    import torch

    from s3prl_amd.ckpt import load_npc_checkpoint

    path = str(tmp_path / "c.pt")
    torch.save({"model": {}}, path)
    with pytest.raises(ValueError, match="config"):
        load_npc_checkpoint(path)
    torch.save({"config": _config()}, path)
    with pytest.raises(ValueError, match="model"):
        load_npc_checkpoint(path)
    with pytest.raises(ValueError, match="kernel_size"):
        load_npc_checkpoint(_save(tmp_path, _config(paras=dict(kernel_size=None))))


REFUSALS = [
    (dict(paras=dict(dim_bottleneck=32)), "dim_bottleneck=32"),
    (dict(paras=dict(kernel_size=14)), "kernel_size must be odd"),
    (dict(paras=dict(mask_size=4)), "mask_size must be odd"),
    (dict(paras=dict(mask_size=7)), "mask leaves no tap in block 3"),          # 7 + 8 = 15 of 15
    (dict(paras=dict(kernel_size=9)), "mask leaves no tap in block 1"),        # 5 + 4 = 9 of 9
    (dict(paras=dict(n_blocks=0)), "n_blocks must be 1..8"),
    (dict(paras=dict(n_blocks=9, kernel_size=31)), "n_blocks must be 1..8"),
    (dict(paras=dict(hidden_size=96)), "multiple of 64"),
    (dict(paras=dict(hidden_size=1088)), "at most 1024"),
    (dict(paras=dict(activate="gelu")), "activate='gelu'"),
    (dict(audio=dict(feat_dim=40)), "feat_dim must be a multiple of 16"),
    (dict(audio=dict(feat_type="mfcc")), "feat_type='mfcc'"),
    (dict(audio=dict(num_ceps=13)), "['num_ceps']"),
    (dict(audio=dict(frame_length=25.1)), "multiple of 4 samples"),   # 401 samples
    (dict(audio=dict(frame_shift=10.125)), "multiple of 4 samples"),  # 162 samples
]


@pytest.mark.parametrize("kw, match", REFUSALS)
def test_config_refusals(tmp_path, kw, match):
    from s3prl_amd.ckpt import load_npc_checkpoint
    from s3prl_amd.config import config_from_npc

    with pytest.raises(ValueError, match=re.escape(match)):
        config_from_npc(_config(**kw))
    with pytest.raises(ValueError, match=re.escape(match)):  # the checkpoint's own config decides
        load_npc_checkpoint(_save(tmp_path, _config(**kw)))


def test_a_mask_only_has_to_leave_a_tap_where_a_masked_conv_exists():
    from s3prl_amd.config import config_from_npc

    c = config_from_npc(_config(paras=dict(disable_cross_layer=True, mask_size=5, kernel_size=15)))
    assert c.num_hidden_states == 6
    with pytest.raises(ValueError, match="block 3"):
        config_from_npc(_config(paras=dict(disable_cross_layer=True, mask_size=7)))


def _create_error(ccfg, npc):
    from s3prl_amd import _lib

    lib = _lib.load()
    h = C.c_void_p()
    tensors = (_lib.S3Tensor * 1)()
    assert lib.s3enc_create_npc(C.byref(ccfg), C.byref(npc) if npc is not None else None, tensors, 0, 0, C.byref(h)) != 0
    assert not h.value
    return lib.s3enc_last_error().decode()


@pytest.mark.parametrize("field, value, match", [
    ("dim_bottleneck", 32, "dim_bottleneck"),
    ("kernel_size", 14, "kernel_size must be odd"),
    ("mask_size", 4, "mask_size must be odd"),
    ("mask_size", 7, "leaves no tap in block 3"),
    ("n_blocks", 0, "n_blocks must be 1..8"),
    ("n_blocks", 9, "n_blocks must be 1..8"),
    ("activate", 2, "activate"),
    ("window", 2, "window"),
    ("num_mel_bins", 40, "multiple of 16"),
    ("frame_length_ms", 25.1, "multiple of 4 samples"),
    ("frame_shift_ms", 10.125, "multiple of 4 samples"),
    ("frame_shift_ms", 20.0, "frame geometry"),
    ("disable_cross_layer", 1, "number of states"),
])
def test_the_library_refuses_by_name(field, value, match):
    """s3enc_create_npc checks the configuration before it looks for a device: the refusals are the same without a GPU."""
    from s3prl_amd import _lib
    from s3prl_amd.synth import named_config

    cfg = named_config("tiny_npc")
    ccfg, npc = _lib.make_config(cfg, "fp32"), _lib.make_npc_config(cfg)
    assert ccfg.family == 10 and ccfg.n_conv == 1 and (ccfg.conv_kernel[0], ccfg.conv_stride[0]) == (400, 160) and ccfg.encoder_layers == 8
    assert (npc.num_mel_bins, npc.frame_length_ms, npc.frame_shift_ms, npc.window, npc.cmvn, npc.hidden, npc.n_blocks, npc.kernel_size,
            npc.mask_size, npc.residual, npc.batch_norm, npc.activate, npc.disable_cross_layer, npc.dim_bottleneck) == (
        16, 25.0, 10.0, 1, 1, 64, 4, 15, 5, 1, 1, 0, 0, 0)
    setattr(npc, field, value)
    assert match in _create_error(ccfg, npc)


@pytest.mark.parametrize("width, match", [(96, "multiple of 64"), (1088, "at most 1024")])
def test_the_library_refuses_widths_the_kernel_does_not_take(width, match):
    from s3prl_amd import _lib
    from s3prl_amd.synth import named_config

    cfg = named_config("tiny_npc")
    ccfg, npc = _lib.make_config(cfg, "fp32"), _lib.make_npc_config(cfg)
    ccfg.conv_dim = ccfg.embed_dim = npc.hidden = width
    assert match in _create_error(ccfg, npc)


@pytest.mark.parametrize("dtype", ["bf16", "fp16", "fp16x2", "fp32x3"])
def test_non_fp32_modes_are_refused_with_the_mode_named(dtype):
    from s3prl_amd import _lib
    from s3prl_amd.encoder import HipEncoder
    from s3prl_amd.synth import named_config, synth_weights

    cfg = named_config("tiny_npc")
    err = _create_error(_lib.make_config(cfg, dtype), _lib.make_npc_config(cfg))
    assert "fp32 only" in err and dtype in err
    with pytest.raises(ValueError, match="fp32 only"):
        HipEncoder(cfg, synth_weights(cfg, 0), dtype=dtype)


def test_the_npc_block_is_required_for_the_family_and_refused_elsewhere():
    from s3prl_amd import _lib
    from s3prl_amd.synth import named_config

    cfg = named_config("tiny_npc")
    lib = _lib.load()
    h = C.c_void_p()
    tensors = (_lib.S3Tensor * 1)()
    ccfg = _lib.make_config(cfg, "fp32")
    assert lib.s3enc_create(C.byref(ccfg), tensors, 0, 0, C.byref(h)) != 0 and b"s3enc_create_npc" in lib.s3enc_last_error()
    assert lib.s3enc_create_ex(C.byref(ccfg), None, tensors, 0, 0, C.byref(h)) != 0 and b"s3enc_create_npc" in lib.s3enc_last_error()
    apc = _lib.make_apc_config(named_config("tiny_apc"))
    assert lib.s3enc_create_apc(C.byref(ccfg), C.byref(apc), tensors, 0, 0, C.byref(h)) != 0 and b"s3enc_create_npc" in lib.s3enc_last_error()
    assert "null argument" in _create_error(ccfg, None)
    assert "S3ENC_NPC only" in _create_error(_lib.make_config(named_config("tiny_apc"), "fp32"), _lib.make_npc_config(cfg))
    assert lib.s3enc_version() == 8  # every addition is a new symbol


def test_npc_block_follows_the_header(tmp_path):
    """s3enc_npc_config: field order against the header text, size and offsets against the header compiled as C; the blocks before
    it stay what they were."""
    import subprocess

    from s3prl_amd import _lib

    header = open(os.path.join(ROOT, "include", "s3enc.h")).read()
    body = header[header.index("typedef struct s3enc_npc_config {"):header.index("} s3enc_npc_config;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = re.findall(r"(?:int32_t|float)\s+([a-z0-9_]+)(?:\[[^\]]*\])?;", body)
    assert names == [n for n, _ in _lib.S3NpcConfig._fields_] and names[0] == "num_mel_bins" and names[-1] == "dim_bottleneck"
    assert _lib.FAMILY["npc"] == 10 and "S3ENC_NPC = 10" in header and "#define S3ENC_VERSION 8" in header
    assert [n for n, _ in _lib.S3Config._fields_][-1] == "dw_kernel"
    for sym in ("s3enc_create_npc", "s3enc_op_conv_taps"):
        assert re.search(r"\bint " + sym + r"\(", header), sym
    assert "not zeros" in header[header.index("The S3ENC_NPC family"):header.index("int s3enc_create_npc(")].replace("NOT zeros", "not zeros")
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "s3enc.h"\n'
                   'int main(void){printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(s3enc_npc_config), offsetof(s3enc_npc_config, frame_shift_ms), '
                   'offsetof(s3enc_npc_config, kernel_size), offsetof(s3enc_npc_config, dim_bottleneck), sizeof(s3enc_apc_config), '
                   'sizeof(s3enc_decoar_config));return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    W = _lib.S3NpcConfig
    assert got == [C.sizeof(W), W.frame_shift_ms.offset, W.kernel_size.offset, W.dim_bottleneck.offset, C.sizeof(_lib.S3ApcConfig),
                   C.sizeof(_lib.S3DecoarConfig)]


def test_op_entry_validates_its_arguments():
    """s3enc_op_conv_taps refuses bad arguments with a message before touching a device."""
    from s3prl_amd import _lib

    lib = _lib.load()
    one = C.c_void_p(256)

    def call(x=one, w=one, bias=one, B=2, T=5, Cc=16, N=64, k=15, mask=5, act=2, res=None, ld_res=0, dst=one, dst_pad=7, ldo=64,
             state=None, sm=None, sum_init=1, dense=0):
        rc = lib.s3enc_op_conv_taps(x, w, bias, B, T, Cc, N, k, mask, act, res, ld_res, dst, dst_pad, ldo, state, sm, sum_init, dense, None)
        return rc, lib.s3enc_last_error()

    for kw, msg in [(dict(x=None), b"null argument"), (dict(w=None), b"null argument"), (dict(dst=None), b"no destination"),
                    (dict(B=0), b"bad shape"), (dict(T=0), b"bad shape"), (dict(k=14), b"k must be odd"), (dict(k=65), b"k must be odd"),
                    (dict(mask=4), b"mask must be 0 or odd"), (dict(mask=-1), b"mask must be 0 or odd"),
                    (dict(mask=15), b"leaves no tap"), (dict(mask=17), b"leaves no tap"), (dict(Cc=24), b"multiple of 16"),
                    (dict(Cc=8), b"bad shape"), (dict(N=68, ldo=68, Cc=16, B=2, k=14), b"k must be odd"), (dict(N=66, ldo=68), b"N must be a multiple of 4"), (dict(act=3), b"act must be"), (dict(act=-1), b"act must be"),
                    (dict(ldo=60), b"ldo >= N"), (dict(ldo=66), b"multiples of 4"), (dict(dst_pad=-1), b"dst_pad"),
                    (dict(res=one, ld_res=60), b"ld_res < N"), (dict(res=one, ld_res=66), b"multiples of 4"),
                    (dict(x=C.c_void_p(260)), b"16-byte aligned"), (dict(dst=C.c_void_p(264)), b"16-byte aligned"),
                    (dict(bias=C.c_void_p(260)), b"16-byte aligned"), (dict(dst=None, state=C.c_void_p(260)), b"16-byte aligned"),
                    (dict(dst=None, sm=C.c_void_p(260)), b"16-byte aligned"), (dict(B=70000), b"B above 65535")]:
        rc, err = call(**kw)
        assert rc != 0 and msg in err, (kw, err)


def test_hub_names_have_the_reference_signatures():
    import s3prl_amd.hub as amd

    ref = json.load(open(os.path.join(ROOT, "tests", "golden", "npc", "reference_hub_npc.json")))
    everything = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_hub.json")))["options"]
    assert ref["downsample_rate"] == 160
    checked = []
    for name, params in ref["hubconfs"]["npc"]:
        assert name in everything and name in amd.options(), name
        ours = inspect.signature(getattr(amd, name))
        assert [list(p) for p in params] == [[k, v.kind.name, repr(v.default)] for k, v in ours.parameters.items()], name
        checked.append(name)
    assert sorted(checked) == ["npc", "npc_360hr", "npc_960hr", "npc_local", "npc_url"]
    reg = set(amd.options(only_registered_ckpt=True))
    assert {"npc", "npc_360hr", "npc_960hr"} <= reg and not {"npc_local", "npc_url"} & reg


def test_expert_loads_a_checkpoint_and_reports_the_reference_geometry(tmp_path):
    """Without a GPU: construction, the stride, the state count and sizes; the forward itself needs the MI355X."""
    import torch

    import s3prl_amd.hub as amd
    from s3prl_amd.ckpt import save_checkpoint
    from s3prl_amd.synth import named_config, synth_weights

    for name in ("tiny_npc", "tiny_npc_last"):
        cfg = named_config(name)
        path = str(tmp_path / "c.pt")
        save_checkpoint(path, cfg, synth_weights(cfg, 0))
        expert = amd.npc_local(path)
        n = cfg.num_hidden_states
        assert expert.cfg == cfg and expert.get_downsample_rates("hidden_states") == 160
        assert expert.num_layers == n and expert.hidden_sizes == [64] * n
        assert list(expert._states_info(n)) == R.state_names(cfg)
        wav = torch.zeros(4000, requires_grad=True)
        with pytest.raises(RuntimeError, match="inference-only"):
            expert([wav])
        if not torch.cuda.is_available():
            with pytest.raises(RuntimeError, match="no CPU fallback"):
                expert([torch.zeros(4000)])
