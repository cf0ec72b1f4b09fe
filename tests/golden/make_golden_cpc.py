#!/usr/bin/env python3
"""Generate the modified-CPC fixtures under ``tests/golden/cpc/`` by RUNNING THE REFERENCE (PyTorch CPU).

Run in the build container only (it imports the reference tree through ``ref_shim``):

    python tests/golden/make_golden_cpc.py                 # all cases + the hub-signature fixture
    python tests/golden/make_golden_cpc.py cpc_tiny_pad

Same recipe and ``.npz`` meta format as ``make_golden_wav2vec.py`` (``conftest.load_golden`` reads them as ``"cpc/<case>"``): the
seeded numpy weights of ``s3prl_amd.synth.synth_weights`` are loaded into the reference ``CPCModel(getEncoder(args), getAR(args))``,
saved as ``{"config", "weights"}``, and the reference ``cpc.expert.UpstreamExpert(ckpt)(wavs)`` is recorded: ``hidden_states``
subsampled and their full-tensor norms.

With torch's default initialisation the recurrent output stays below 0.2 in magnitude and no gate leaves its linear range, so a
fixture would not notice a wrong sigmoid or tanh: every fixture must have, per recurrent layer, gate pre-activations (float64,
``tests/cpc_ref.py``) with a standard deviation of at least 1.  A weight seed that misses it is skipped for the next one; the seed
used and the measured values are stored in the meta.

The CPU test pins the float64 restatement to these fp32 outputs at 1e-6, which only means something while the reference's own
fp32 rounding stays below that: the reference is run a second time in ``.double()``, and a seed whose fp32 states are more than
8e-7 away from the float64 ones is skipped as well (``ref_fp32_err`` in the meta).
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

import cpc_ref  # noqa: E402
from make_golden import _import_reference, _load  # noqa: E402
from s3prl_amd.synth import named_config, synth_wavs, synth_weights  # noqa: E402

MIN_GATE_STD = 1.0
MAX_REF_FP32_ERR = 8e-7

# name -> (config, first weight seed, wav seed, lengths, (t_stride, c_stride), dc, scale)
# 159 samples = the receptive field = ONE frame: every convolution at its smallest legal input; 4000 samples = 25 frames
CASES = {
    "cpc_tiny_pad": ("tiny_cpc", 201, 301, [4000, 2345, 3111], (1, 1), 0.0, 1.0),
    "cpc_tiny_eq": ("tiny_cpc", 202, 302, [3200, 3200], (1, 1), 0.1, 0.5),
    "cpc_tiny_t1": ("tiny_cpc", 203, 303, [159, 163], (1, 1), 0.0, 1.0),
    "cpc_tiny_gru_pad": ("tiny_cpc_gru", 204, 304, [4000, 2345, 3111], (1, 1), 0.0, 1.0),
    "cpc_tiny_lstm1_pad": ("tiny_cpc_lstm1", 205, 305, [4000, 2345, 3111], (1, 1), 0.0, 1.0),
    "cpc_base_pseudo": ("cpc_base", 206, 306, [16000, 12345], (1, 4), 0.0, 1.0),
    "cpc_base_10s": ("cpc_base", 207, 307, [160000], (4, 8), 0.0, 1.0),
}


def reference_outputs(cfg, weights, wavs):
    import argparse

    import torch

    _import_reference()
    from s3prl.upstream.cpc.cpc_default_config import get_default_cpc_config
    from s3prl.upstream.cpc.expert import UpstreamExpert
    from s3prl.upstream.cpc.feature_loader import getAR, getEncoder, loadArgs
    from s3prl.upstream.cpc.model import CPCModel

    torch.manual_seed(0)
    config = dict(hiddenEncoder=cfg.conv_dim, hiddenGar=cfg.ar_hidden, arMode=cfg.ar_mode, nLevelsGRU=cfg.ar_layers)
    args = get_default_cpc_config()
    loadArgs(args, argparse.Namespace(**config))
    model = CPCModel(getEncoder(args), getAR(args))
    _load(model, weights)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "ckpt.pt")
        torch.save({"config": config, "weights": model.state_dict()}, path)
        expert = UpstreamExpert(path).eval()
        assert expert.get_downsample_rates("hidden_states") == 160
        with torch.no_grad():
            out = expert([torch.from_numpy(w.copy()) for w in wavs])
            out64 = expert.double()([torch.from_numpy(w.astype(np.float64)) for w in wavs])
    errs = [float(np.linalg.norm(a.numpy().astype(np.float64) - b.numpy()) / np.linalg.norm(b.numpy()))
            for a, b in zip(out["hidden_states"], out64["hidden_states"])]
    return out, errs


def make_case(name: str):
    cfg_name, wseed, xseed, lengths, (ts, cs), dc, scale = CASES[name]
    cfg = named_config(cfg_name)
    wavs = synth_wavs(lengths, xseed, dc=dc, scale=scale)
    while True:
        weights = synth_weights(cfg, wseed)
        gate_std = cpc_ref.forward(cfg, weights, wavs)["gate_std"]
        if min(gate_std) >= MIN_GATE_STD:
            out, ref_err = reference_outputs(cfg, weights, wavs)
            if max(ref_err) <= MAX_REF_FP32_ERR:
                break
            print(f"{name}: weight seed {wseed}: the reference's fp32 states are {ref_err} from its float64 ones > {MAX_REF_FP32_ERR:g}: next seed")
        else:
            print(f"{name}: weight seed {wseed} has gate pre-activation std {gate_std} < {MIN_GATE_STD:g}: next seed")
        wseed += 1
    assert "default" not in out
    hs = [h.numpy() for h in out["hidden_states"]]
    assert len(hs) == cfg.num_hidden_states == 2 and hs[0].shape == hs[1].shape
    assert hs[0].shape[1] == cfg.num_frames(max(lengths))
    meta = dict(config=cfg_name, weight_seed=wseed, wav_seed=xseed, lengths=lengths, t_stride=ts, c_stride=cs, dc=dc,
                scale=scale, shape=list(hs[0].shape), reference="s3prl 0.4.18 cpc/expert.py, torch CPU fp32",
                n_states=len(hs), gate_std=gate_std, ref_fp32_err=ref_err)
    arrays = {f"hs{l}": np.ascontiguousarray(h[:, ::ts, ::cs]) for l, h in enumerate(hs)}
    arrays["norms"] = np.array([np.linalg.norm(h.astype(np.float64)) for h in hs])
    arrays["meta"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    path = os.path.join(HERE, "cpc", f"{name}.npz")
    np.savez_compressed(path, **arrays)
    print(f"{name}: {len(hs)} x {hs[0].shape} gate std {['%.2f' % s for s in gate_std]} max|h| {np.abs(hs[1]).max():.2f} "
          f"-> {os.path.getsize(path) / 1e3:.0f} kB")


def make_hub_fixture():
    """names and signatures of the reference's cpc hubconf, in reference_hub_wav2vec.json's layout"""
    _import_reference()
    import importlib

    mod = importlib.import_module("s3prl.upstream.cpc.hubconf")
    res = {"cpc": [[n, [[k, v.kind.name, repr(v.default)] for k, v in inspect.signature(f).parameters.items()]]
                   for n, f in vars(mod).items() if inspect.isfunction(f) and not n.startswith("_") and f.__module__ == mod.__name__]}
    with open(os.path.join(HERE, "cpc", "reference_hub_cpc.json"), "w") as f:
        json.dump(dict(reference="s3prl 0.4.18: s3prl.upstream.cpc.hubconf", hubconfs=res, downsample_rate=160), f, indent=1,
                  sort_keys=True)


if __name__ == "__main__":
    names = sys.argv[1:] or list(CASES) + ["hub"]
    for n in names:
        make_hub_fixture() if n == "hub" else make_case(n)
