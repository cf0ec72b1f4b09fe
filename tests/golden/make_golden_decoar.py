#!/usr/bin/env python3
"""Generate the DeCoAR / DeCoAR-layers fixtures under ``tests/golden/decoar/`` by RUNNING THE REFERENCE (PyTorch CPU).

Run in the build container only (it imports the reference tree through ``ref_shim``):

    python tests/golden/make_golden_decoar.py                 # all cases + the hub-signature fixture
    python tests/golden/make_golden_decoar.py decoar_tiny_pad

Same recipe and ``.npz`` meta format as ``make_golden_apc.py`` (``conftest.load_golden`` reads them as ``"decoar/<case>"``): the
seeded numpy weights of ``s3prl_amd.synth.synth_weights`` are saved as the checkpoint ``{"model": state_dict}`` and the reference
expert's ``forward`` is recorded: ``hidden_states`` subsampled and their full-tensor norms.

* The reference's ``Decoar()`` hard-codes 80 / 1024 / 4.  The committed cases run the reference's own ``Decoar.forward`` / expert
  ``forward`` with its three modules replaced by narrower ``nn.Linear`` / ``nn.LSTM`` of the same kind, holding the seeded weights.
* ``decoar_pseudo`` (only when named on the command line) is the full-size pair: ONE seeded checkpoint file read by
  ``decoar.expert.UpstreamExpert`` (one state) and by ``decoar_layers.expert.UpstreamExpert`` (four states, after its own renaming
  of the tensors).  NO SEED PASSES THE RULES BELOW at that shape and no such fixture is committed: with gate pre-activations of
  standard deviation >= 1 in every layer the reference's own fp32 states of layers 1..4 are 5.6e-7, 9.6e-7, 1.5e-6 and 2.4e-6 away
  from its ``.double()`` evaluation (seeds 607..636, 48 / 33 frames), against the bound of 8e-7; weights weak enough for 8e-7 at
  layer 4 leave the gates of layers 2..4 at a standard deviation of 0.5.  The released shape is held to the float64 restatement
  instead (tests/test_decoar_gpu.py), and the reference's own modules to the narrower fixtures.

The reference's front end is ``torchaudio.compliance.kaldi.fbank``, and torchaudio is not installed: the expert is built with the
placeholder module of ``ref_shim`` and its ``preprocessor`` is replaced by a module that hands out a table of features — the
float64 front end of ``tests/decoar_ref.py`` on the stored waveforms, rounded to fp32.  What the fixtures pin is therefore
everything BEHIND the front end: the projection, packing, both LSTM stacks with their flips, the concatenation.

Every fixture must have, per layer and direction, gate pre-activations (float64) of standard deviation >= 1; the reference's own
fp32 states must be within 8e-7 of its ``.double()`` evaluation; and an all-fp32 numpy evaluation of ``decoar_ref`` FROM THE
WAVEFORMS must stay within a quarter of the GPU tests' ``FP32_TOL`` = 1e-4 of the stored states.  A weight seed that misses one of
them is skipped for the next one.
"""

from __future__ import annotations

import inspect
import json
import os
import re
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import decoar_ref  # noqa: E402
from make_golden import _import_reference  # noqa: E402
from s3prl_amd.synth import named_config, synth_wavs, synth_weights  # noqa: E402

MIN_GATE_STD = 1.0
MAX_REF_FP32_ERR = 8e-7
MAX_FP32_PROXY_ERR = 0.25 * 1e-4
MAX_SEEDS = 8  # weight seeds tried per case before giving up

# name -> (configs, first weight seed, wav seed, lengths, (t_stride, c_stride), dc, scale); a name with two configurations is ONE
# checkpoint read by both experts: "<name>" through decoar, "<name>_layers" through decoar_layers
# 560 samples = two analysis windows = 2 frames, the fewest the front end's std over time allows; 8000 / 5555 samples = 48 / 33 frames
CASES = {
    "decoar_tiny_pad": (("tiny_decoar",), 601, 701, [4000, 2345, 3111], (1, 1), 0.0, 1.0),
    "decoar_tiny_eq": (("tiny_decoar",), 602, 702, [3200, 3200], (1, 1), 0.1, 0.5),
    "decoar_tiny_t2": (("tiny_decoar",), 603, 703, [560, 2000], (1, 1), 0.0, 1.0),
    "decoar_tiny_l1": (("tiny_decoar_l1",), 604, 704, [4000, 2345, 3111], (1, 1), 0.0, 1.0),
    "decoar_layers_tiny_pad": (("tiny_decoar_layers",), 605, 705, [4000, 2345, 3111], (1, 1), 0.0, 1.0),
    "decoar_layers_tiny_h192": (("tiny_decoar_h192",), 606, 706, [4000, 2345, 3111], (1, 2), 0.0, 1.0),
}
# only when named: the full-size pair (see the module docstring: it misses the acceptance rules at every seed)
FULL_SIZE = {
    "decoar_pseudo": (("decoar", "decoar_layers"), 607, 707, [8000, 5555], (2, 8), 0.0, 1.0),
}


def layers_names(weights):
    """the checkpoint's names as the per-layer modules of decoar_layers hold them: X_lstm.Y_lN -> X_lstms.N.Y_l0"""
    out = {}
    for k, v in weights.items():
        m = re.fullmatch(r"(forward|backward)_lstm\.(\w+)_l(\d+)", k)
        out[f"{m.group(1)}_lstms.{m.group(3)}.{m.group(2)}_l0" if m else k] = v
    return out


def reference_outputs(cfg, weights, feats32, lens):
    import torch

    _import_reference()
    import torchaudio.compliance.kaldi  # noqa: F401  (the placeholder: decoar/audio.py imports the name)
    from s3prl.upstream.decoar.expert import UpstreamExpert as One
    from s3prl.upstream.decoar_layers.expert import UpstreamExpert as PerLayer

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
    H, NL, F = cfg.decoar_hidden, cfg.decoar_layers, cfg.decoar_feat_dim
    released = (H, NL, F) == (1024, 4, 80)
    sd = {k: torch.from_numpy(v.copy()) for k, v in weights.items()}
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "ckpt.pt")
        torch.save({"model": sd if released else {}}, path)
        expert = (PerLayer if cfg.decoar_per_layer else One)(path).eval()
    if not released:  # the same modules, narrower
        m = expert.model
        m.post_extract_proj = torch.nn.Linear(F, H)
        lstm = lambda n: torch.nn.LSTM(input_size=H, hidden_size=H, num_layers=n, batch_first=True, bidirectional=False)  # noqa: E731
        if cfg.decoar_per_layer:
            m.forward_lstms = torch.nn.ModuleList([lstm(1) for _ in range(NL)])
            m.backward_lstms = torch.nn.ModuleList([lstm(1) for _ in range(NL)])
            named = layers_names(sd)
        else:
            m.forward_lstm, m.backward_lstm = lstm(NL), lstm(NL)
            named = sd
        assert set(named) == set(m.state_dict()), sorted(set(named) ^ set(m.state_dict()))
        m.load_state_dict(named)
    else:
        have = expert.model.state_dict()
        named = layers_names(sd) if cfg.decoar_per_layer else sd
        assert set(named) == set(have) and all(torch.equal(have[k], named[k]) for k in named), "the expert did not load the checkpoint"
    assert expert.get_downsample_rates("hidden_states") == 160
    table = [torch.from_numpy(feats32[b, :n].copy()) for b, n in enumerate(lens)]
    wavs = [torch.zeros(16) for _ in lens]  # the table decides; the waveforms are not read
    with torch.no_grad():
        expert.preprocessor = Table(table)
        out = expert(wavs)
        expert = expert.double()
        expert.preprocessor = Table([t.double() for t in table])
        out64 = expert(wavs)
    assert out["last_hidden_state"] is out["hidden_states"][-1] and set(out) == {"hidden_states", "last_hidden_state"}
    errs = [float(np.linalg.norm(a.numpy().astype(np.float64) - b.numpy()) / np.linalg.norm(b.numpy()))
            for a, b in zip(out["hidden_states"], out64["hidden_states"])]
    return [h.numpy() for h in out["hidden_states"]], errs


def rel(a, b):
    return float(np.linalg.norm(np.asarray(a, np.float64) - np.asarray(b, np.float64)) / np.linalg.norm(np.asarray(b, np.float64)))


def make_case(name: str):
    cfg_names, wseed, xseed, lengths, (ts, cs), dc, scale = {**CASES, **FULL_SIZE}[name]
    first_seed = wseed
    cfgs = [named_config(n) for n in cfg_names]
    wavs = synth_wavs(lengths, xseed, dc=dc, scale=scale)
    feats, lens = decoar_ref.features(cfgs[0], wavs)
    feats32 = feats.astype(np.float32)
    while True:
        weights = synth_weights(cfgs[0], wseed)
        assert all(set(synth_weights(c, wseed)) == set(weights) for c in cfgs[1:])
        gate_std = decoar_ref.model(cfgs[0], weights, feats32, lens)["gate_std"]
        if min(gate_std) >= MIN_GATE_STD:
            runs = []
            for cfg in cfgs:
                hs, ref_err = reference_outputs(cfg, weights, feats32, lens)
                proxy = [rel(a, b) for a, b in zip(decoar_ref.forward_fp32(cfg, weights, wavs), hs)]
                runs.append((cfg, hs, ref_err, proxy))
            if all(max(r[2]) <= MAX_REF_FP32_ERR and max(r[3]) <= MAX_FP32_PROXY_ERR for r in runs):
                break
            print(f"{name}: weight seed {wseed}: reference fp32 vs float64 {[r[2] for r in runs]} (<= {MAX_REF_FP32_ERR:g}), fp32 "
                  f"evaluation from the waveforms {[r[3] for r in runs]} (<= {MAX_FP32_PROXY_ERR:g}): next seed")
        else:
            print(f"{name}: weight seed {wseed} has gate pre-activation std {gate_std} < {MIN_GATE_STD:g}: next seed")
        wseed += 1
        if wseed - first_seed >= MAX_SEEDS:
            raise SystemExit(f"{name}: no weight seed in {first_seed}..{wseed - 1} meets the acceptance rules; nothing written")
    os.makedirs(os.path.join(HERE, "decoar"), exist_ok=True)
    for i, (cfg, hs, ref_err, proxy) in enumerate(runs):
        out_name = name if i == 0 else name.replace("decoar", "decoar_layers", 1)
        assert len(hs) == cfg.num_hidden_states == (cfg.decoar_layers if cfg.decoar_per_layer else 1)
        assert all(h.shape == (len(lens), max(lens), 2 * cfg.decoar_hidden) for h in hs)
        assert hs[0].shape[1] == cfg.num_frames(max(lengths)) and lens == [cfg.num_frames(n) for n in lengths]
        for b, n in enumerate(lens):  # pad_packed_sequence: exactly zero behind every utterance's frames
            assert all(not h[b, n:].any() for h in hs)
        meta = dict(config=cfg_names[i], weight_seed=wseed, wav_seed=xseed, lengths=lengths, frames=lens, t_stride=ts, c_stride=cs,
                    dc=dc, scale=scale, shape=list(hs[0].shape),
                    reference=f"s3prl 0.4.18 {'decoar_layers' if cfg.decoar_per_layer else 'decoar'}/expert.py, torch CPU fp32, table "
                              "preprocessor" + ("" if cfg.decoar_hidden == 1024 else ", narrower modules of the same kind"),
                    n_states=len(hs), gate_std=gate_std, ref_fp32_err=ref_err, fp32_proxy_err=proxy)
        arrays = {f"hs{l}": np.ascontiguousarray(h[:, ::ts, ::cs]) for l, h in enumerate(hs)}
        arrays["norms"] = np.array([np.linalg.norm(h.astype(np.float64)) for h in hs])
        arrays["meta"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
        path = os.path.join(HERE, "decoar", f"{out_name}.npz")
        np.savez_compressed(path, **arrays)
        print(f"{out_name}: {len(hs)} x {hs[0].shape} frames {lens} gate std {['%.2f' % s for s in gate_std]} ref err "
              f"{max(ref_err):.1e} fp32 proxy {max(proxy):.1e} max|h| {np.abs(hs[-1]).max():.2f} -> {os.path.getsize(path) / 1e3:.0f} kB")


def make_hub_fixture():
    """names and signatures of the reference's decoar / decoar_layers hubconfs, in reference_hub_apc.json's layout"""
    _import_reference()
    import importlib

    import torchaudio.compliance.kaldi  # noqa: F401

    res = {}
    for fam in ("decoar", "decoar_layers"):
        mod = importlib.import_module(f"s3prl.upstream.{fam}.hubconf")
        res[fam] = [[n, [[k, v.kind.name, repr(v.default)] for k, v in inspect.signature(f).parameters.items()]]
                    for n, f in vars(mod).items() if inspect.isfunction(f) and not n.startswith("_") and f.__module__ == mod.__name__]
    os.makedirs(os.path.join(HERE, "decoar"), exist_ok=True)
    with open(os.path.join(HERE, "decoar", "reference_hub_decoar.json"), "w") as f:
        json.dump(dict(reference="s3prl 0.4.18: s3prl.upstream.decoar.hubconf, s3prl.upstream.decoar_layers.hubconf", hubconfs=res,
                       downsample_rate=160), f, indent=1, sort_keys=True)


if __name__ == "__main__":
    names = sys.argv[1:] or list(CASES) + ["hub"]
    for n in names:
        make_hub_fixture() if n == "hub" else make_case(n)
