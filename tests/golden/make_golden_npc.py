#!/usr/bin/env python3
"""Generate the NPC fixtures under ``tests/golden/npc/`` by RUNNING THE REFERENCE (PyTorch CPU).

Run in the build container only (it imports the reference tree through ``ref_shim``):

    python tests/golden/make_golden_npc.py                 # all cases + the hub-signature fixture
    python tests/golden/make_golden_npc.py npc_tiny_pad

Same recipe and ``.npz`` meta format as ``make_golden_apc.py`` (``conftest.load_golden`` reads them as ``"npc/<case>"``): the seeded
numpy weights of ``s3prl_amd.synth.synth_weights`` are loaded into the reference ``NPC(feat_dim, **paras)`` (its ``postnet`` and
``vq_layers`` keep torch's seeded initialisation, its ``conv_mask`` buffers are its own: no hooked state depends on the former, and
the latter are what the HIP path must reproduce), saved as ``{"config", "model"}``, and the reference
``npc.expert.UpstreamExpert(ckpt).eval()(wavs)`` is recorded: ``hidden_states`` subsampled and their full-tensor norms.

The reference's front end is ``torchaudio.compliance.kaldi.fbank``, and torchaudio is not installed: the expert is built with the
placeholder module of ``ref_shim`` and its ``preprocessor`` is replaced by a module that hands out a table of features — the
float64 front end of ``tests/apc_ref.py`` on the stored waveforms, rounded to fp32.  What the fixtures pin is therefore everything
BEHIND the front end: the ConvBlocks with BatchNorm in eval mode, the masks, the sum, the hooks and their order, and — since the
reference masks nothing — every row of the padded batch.

A weight seed is skipped for the next one unless all of these hold:
  * the reference's own fp32 states are within 8e-7 of its ``.double()`` evaluation, on every state;
  * every masked state has at most 15 % of its elements with |y| > 0.99 and a standard deviation of at least 0.4 (tanh is used on
    both sides of its bend);
  * under ReLU every block state has between 20 % and 70 % exact zeros;
  * an all-fp32 numpy evaluation of ``npc_ref`` FROM THE WAVEFORMS stays within a quarter of the GPU tests' ``FP32_TOL`` = 1e-4.
"""

from __future__ import annotations

import inspect
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import npc_ref  # noqa: E402
from make_golden import _import_reference, _load  # noqa: E402
from s3prl_amd.synth import named_config, synth_wavs, synth_weights  # noqa: E402

MAX_REF_FP32_ERR = 8e-7
MAX_SATURATED, MIN_MASKED_STD = 0.15, 0.4
RELU_ZEROS = (0.20, 0.70)
MAX_FP32_PROXY_ERR = 0.25 * 1e-4
MAX_SEEDS = 40
MAX_BYTES = 256 * 1024

# name -> (config, first weight seed, wav seed, lengths, (t_stride, c_stride), dc, scale)
# 400 samples = one analysis window = ONE frame (no std over time: that case runs without CMVN); 4000 samples = 23 frames.
# There is no T < P fixture ([1200] samples = 6 frames under P = 7): the last block's mask of 13 leaves taps +-7 only, which then read
# nothing but the zero border, so that masked state is tanh(bias), constant over time — its standard deviation (0.1, the spread of
# the biases) cannot reach the 0.4 the rules above ask for, whatever the seed.  The rules stand; that shape is held to the float64
# restatement instead (tests/test_npc_cpu.py pins the restatement on the other fixtures, tests/test_npc_gpu.py runs the shape).
CASES = {
    "npc_tiny_pad": ("tiny_npc", 701, 801, [4000, 2345, 3111], (1, 1), 0.0, 1.0),
    "npc_tiny_eq": ("tiny_npc", 702, 802, [3200, 3200], (1, 1), 0.1, 0.5),
    "npc_tiny_plain": ("tiny_npc_plain", 703, 803, [4000, 2345, 3111], (1, 1), 0.0, 1.0),
    "npc_tiny_t1": ("tiny_npc_nocmvn", 704, 804, [400, 2000], (1, 1), 0.0, 1.0),
    "npc_tiny_last": ("tiny_npc_last", 706, 806, [4000, 2345, 3111], (1, 1), 0.0, 1.0),
    "npc_tiny_k9": ("tiny_npc_k9", 707, 807, [4000, 2345, 3111], (1, 1), 0.0, 1.0),
    "npc_360hr_pseudo": ("npc_360hr", 708, 808, [16000, 12345], (1, 16), 0.0, 1.0),
}


def npc_paras(cfg):
    paras = dict(kernel_size=cfg.npc_kernel_size, mask_size=cfg.npc_mask_size, n_blocks=cfg.npc_blocks, hidden_size=cfg.conv_dim,
                 dropout=0.1, residual=cfg.npc_residual, batch_norm=cfg.npc_batch_norm, activate=cfg.npc_activate,
                 disable_cross_layer=cfg.npc_disable_cross_layer)
    if cfg.npc_vq is not None:
        paras["vq"] = dict(cfg.npc_vq)
    return paras


def reference_outputs(cfg, weights, feats32, lens):
    import torch

    _import_reference()
    import torchaudio.compliance.kaldi  # noqa: F401  (the placeholder: npc/audio.py imports the name)
    from s3prl.upstream.npc.expert import UpstreamExpert
    from s3prl.upstream.npc.npc import NPC

    class Table(torch.nn.Module):
        """stands where FeatureExtractor stood: the i-th call returns the i-th utterance's features"""

        def __init__(self, table):
            super().__init__()
            self.table, self.i = table, 0

        def forward(self, wav):
            out = self.table[self.i % len(self.table)]
            self.i += 1
            return out

    torch.manual_seed(0)
    paras = npc_paras(cfg)
    audio = dict(feat_type="fbank", feat_dim=cfg.apc_feat_dim, frame_length=cfg.apc_frame_length, frame_shift=cfg.apc_frame_shift,
                 decode_wav=False, cmvn=cfg.apc_cmvn)
    model = NPC(cfg.apc_feat_dim, **paras)
    _load(model, weights)
    assert (cfg.npc_vq is not None) == any(k.startswith("vq_layers.") for k in model.state_dict())
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "ckpt.pt")
        torch.save({"config": {"data": {"audio": audio}, "model": {"paras": paras}}, "model": model.state_dict()}, path)
        expert = UpstreamExpert(path).eval()
    assert expert.get_downsample_rates("hidden_states") == 160
    table = [torch.from_numpy(feats32[b, :n].copy()) for b, n in enumerate(lens)]
    wavs = [torch.zeros(16) for _ in lens]  # the table decides; the waveforms are not read
    with torch.no_grad():
        expert.preprocessor = Table(table)
        out = expert(wavs)
        expert = expert.double()
        expert.preprocessor = Table([t.double() for t in table])
        out64 = expert(wavs)
    errs = [float(np.linalg.norm(a.numpy().astype(np.float64) - b.numpy()) / np.linalg.norm(b.numpy()))
            for a, b in zip(out["hidden_states"], out64["hidden_states"])]
    return out, errs


def rel(a, b):
    return float(np.linalg.norm(np.asarray(a, np.float64) - np.asarray(b, np.float64)) / np.linalg.norm(np.asarray(b, np.float64)))


def make_case(name: str):
    cfg_name, wseed, xseed, lengths, (ts, cs), dc, scale = CASES[name]
    cfg = named_config(cfg_name)
    wavs = synth_wavs(lengths, xseed, dc=dc, scale=scale)
    feats, lens = npc_ref.features(cfg, wavs)
    feats32 = feats.astype(np.float32)
    first = wseed
    while True:
        assert wseed < first + MAX_SEEDS, f"{name}: no weight seed in [{first}, {wseed}) meets the generator's rules"
        weights = synth_weights(cfg, wseed)
        mine = npc_ref.model(cfg, weights, feats32)
        kinds = mine["kinds"]
        sat = [float((np.abs(h) > 0.99).mean()) for h, kd in zip(mine["hidden_states"], kinds) if kd == "masked"]
        mstd = [float(h.std()) for h, kd in zip(mine["hidden_states"], kinds) if kd == "masked"]
        zeros = [float((h == 0).mean()) for h, kd in zip(mine["hidden_states"], kinds) if kd == "block"]
        ok = max(sat) <= MAX_SATURATED and min(mstd) >= MIN_MASKED_STD
        if cfg.npc_activate == "relu":
            ok = ok and RELU_ZEROS[0] <= min(zeros) and max(zeros) <= RELU_ZEROS[1]
        if ok:
            out, ref_err = reference_outputs(cfg, weights, feats32, lens)
            hs = [h.numpy() for h in out["hidden_states"]]
            proxy = [rel(a, b) for a, b in zip(npc_ref.forward_fp32(cfg, weights, wavs), hs)]
            if max(ref_err) <= MAX_REF_FP32_ERR and max(proxy) <= MAX_FP32_PROXY_ERR:
                break
            print(f"{name}: weight seed {wseed}: reference fp32 vs float64 {ref_err} (<= {MAX_REF_FP32_ERR:g}), fp32 evaluation from "
                  f"the waveforms {proxy} (<= {MAX_FP32_PROXY_ERR:g}): next seed")
        else:
            print(f"{name}: weight seed {wseed}: saturated {sat} (<= {MAX_SATURATED}), masked std {mstd} (>= {MIN_MASKED_STD}), "
                  f"relu zeros {zeros} (in {RELU_ZEROS}): next seed")
        wseed += 1
    assert "default" not in out
    assert list(out["_hidden_states_info"]) == npc_ref.state_names(cfg), out["_hidden_states_info"]
    assert len(hs) == cfg.num_hidden_states == len(kinds) and all(h.shape == hs[0].shape for h in hs)
    assert hs[0].shape[1] == cfg.num_frames(max(lengths)) == max(lens)
    if cfg.npc_disable_cross_layer:
        assert np.array_equal(hs[-1], hs[-2])
    # no length masking: the rows behind an utterance's frames are loud from state 0 on
    pad_norm = [float(np.linalg.norm(hs[0][b, n:])) for b, n in enumerate(lens) if n < hs[0].shape[1]]
    assert all(v > 0 for v in pad_norm)
    meta = dict(config=cfg_name, weight_seed=wseed, wav_seed=xseed, lengths=lengths, frames=lens, t_stride=ts, c_stride=cs, dc=dc,
                scale=scale, shape=list(hs[0].shape), reference="s3prl 0.4.18 npc/expert.py (.eval()), torch CPU fp32, table preprocessor",
                n_states=len(hs), kinds=kinds, saturated=sat, masked_std=mstd, relu_zeros=zeros, pad_row_norm=pad_norm,
                ref_fp32_err=ref_err, fp32_proxy_err=proxy)
    arrays = {f"hs{l}": np.ascontiguousarray(h[:, ::ts, ::cs]) for l, h in enumerate(hs)}
    arrays["norms"] = np.array([np.linalg.norm(h.astype(np.float64)) for h in hs])
    arrays["meta"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    os.makedirs(os.path.join(HERE, "npc"), exist_ok=True)
    path = os.path.join(HERE, "npc", f"{name}.npz")
    np.savez_compressed(path, **arrays)
    assert os.path.getsize(path) < MAX_BYTES, (path, os.path.getsize(path))
    print(f"{name}: seed {wseed}: {len(hs)} x {hs[0].shape} frames {lens} saturated {max(sat):.2f} masked std {min(mstd):.2f} relu zeros "
          f"{min(zeros):.2f}-{max(zeros):.2f} ref err {max(ref_err):.1e} fp32 proxy {max(proxy):.1e} pad rows {pad_norm} -> "
          f"{os.path.getsize(path) / 1e3:.0f} kB")


def make_hub_fixture():
    """names and signatures of the reference's npc hubconf, in reference_hub_apc.json's layout"""
    _import_reference()
    import importlib

    import torchaudio.compliance.kaldi  # noqa: F401

    mod = importlib.import_module("s3prl.upstream.npc.hubconf")
    res = {"npc": [[n, [[k, v.kind.name, repr(v.default)] for k, v in inspect.signature(f).parameters.items()]]
                   for n, f in vars(mod).items() if inspect.isfunction(f) and not n.startswith("_") and f.__module__ == mod.__name__]}
    os.makedirs(os.path.join(HERE, "npc"), exist_ok=True)
    with open(os.path.join(HERE, "npc", "reference_hub_npc.json"), "w") as f:
        json.dump(dict(reference="s3prl 0.4.18: s3prl.upstream.npc.hubconf", hubconfs=res, downsample_rate=160), f, indent=1,
                  sort_keys=True)


if __name__ == "__main__":
    names = sys.argv[1:] or list(CASES) + ["hub"]
    for n in names:
        make_hub_fixture() if n == "hub" else make_case(n)
