#!/usr/bin/env python3
"""Generate the DeCoAR 2.0 fixtures under ``tests/golden/decoar2/`` by RUNNING THE REFERENCE (PyTorch CPU).

Run in the build container only (it imports the reference tree through ``ref_shim``):

    python tests/golden/make_golden_decoar2.py                 # all cases + the hub-signature fixture
    python tests/golden/make_golden_decoar2.py tiny_ragged_odd

Same ``.npz`` meta format as the other generators (``conftest.load_golden`` reads them as ``"decoar2/<case>"``): the seeded numpy
weights of ``s3prl_amd.synth.synth_weights`` are saved as the checkpoint ``{"model": state_dict}`` by the product writer and the
reference's own ``UpstreamExpert.__call__`` is recorded, hooks and ``postprocess`` included: ``hidden_states`` subsampled and
their full-tensor norms.

* The reference's ``Decoar2()`` reads its widths from the module-level dict ``decoar2.args``.  The small cases narrow that dict's
  entries before the expert is built; the full-size case leaves it alone.
* The reference's front end is ``torchaudio.compliance.kaldi.fbank`` and torchaudio is not installed: a stand-in ``torchaudio`` of
  our own sits in ``sys.modules`` whose ``compliance.kaldi.fbank`` is the project's restatement (``tests/apc_ref.py::kaldi_fbank`` on
  ``oracle/fbank_oracle.py``'s framing and mel bank, float64, rounded to the waveform's dtype).  So NO torchaudio RUN stands behind
  the log-mels; the CMVN, the subsampling, ``pad_sequence``, the mask and everything behind them are the reference's own code.

A weight seed is kept only if the reference's own fp32 states are within 8e-7 of its ``.double()`` evaluation and an all-fp32 numpy
evaluation of ``tests/decoar2_ref.py`` FROM THE WAVEFORMS stays within a quarter of the GPU tests' ``FP32_TOL`` = 1e-4 of the
stored states; else the next seed is tried.  The first rule judges what make_golden_decoar.py / make_golden_apc.py judge with it,
the reference's fp32 arithmetic BEHIND the front end: the ``.double()`` run reads the features the fp32 run's own FeatureExtractor
produced.  With the CMVN inside the comparison no seed passes at any width (tried: 801..808, 1.14e-6..1.31e-6 at two layers): an fp32
CMVN of log-mels of magnitude 10 over a standard deviation of 0.3..1 is 0.8e-6..2.4e-6 away from float64 by itself.  The stored
states are the fp32 run's, front end included.
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

import apc_ref  # noqa: E402
import decoar2_ref  # noqa: E402
from s3prl_amd.ckpt import save_checkpoint  # noqa: E402
from s3prl_amd.synth import named_config, synth_wavs, synth_weights  # noqa: E402

OUT = os.path.join(HERE, "decoar2")
MAX_REF_FP32_ERR = 8e-7
MAX_FP32_PROXY_ERR = 0.25 * 1e-4
MAX_SEEDS = 8

# name -> (config, first weight seed, wav seed, lengths, (t_stride, c_stride), profile); frames F = 1 + (n - 400) // 160
CASES = {
    "tiny_ragged_odd": ("tiny_decoar2", 801, 901, [4000, 2345, 3111], (1, 1), "synthetic"),      # F 23, 13, 17: T 12, 7, 9
    "tiny_ragged_even": ("tiny_decoar2", 802, 902, [4160, 2400, 3200], (1, 1), "synthetic"),     # F 24, 13, 18: T 12, 7, 9
    "tiny_equal": ("tiny_decoar2", 803, 903, [3200, 3200], (1, 1), "synthetic"),                 # F 18: T 9
    "tiny_t1": ("tiny_decoar2", 804, 904, [560, 2000], (1, 1), "synthetic"),                     # F 2: ONE model frame beside 6
    "tiny_two_tiles": ("tiny_decoar2", 805, 905, [41999, 20000], (4, 2), "synthetic"),           # T 130: two positional-conv tiles
    "tiny_d192": ("tiny_decoar2_d192", 806, 906, [4000, 2345, 3111], (1, 2), "synthetic"),       # group width 48
    "pseudo": ("decoar2", 807, 907, [32000, 20000, 27777], (4, 16), "pretrained_like"),          # released shape and statistics
}
WANT = {"tiny_ragged_odd": lambda F, T: F[0] % 2 == 1 and len(set(T)) == 3, "tiny_ragged_even": lambda F, T: F[0] % 2 == 0 and len(set(T)) == 3,
        "tiny_equal": lambda F, T: len(set(T)) == 1, "tiny_t1": lambda F, T: F[0] == 2 and T[0] == 1, "tiny_two_tiles": lambda F, T: max(T) > 128,
        "tiny_d192": lambda F, T: True, "pseudo": lambda F, T: len(T) == 3 and max(F) <= 198}


def install_torchaudio_stand_in():
    """``torchaudio.compliance.kaldi.fbank`` = the project's restatement; every other attribute is ref_shim's placeholder."""
    import ref_shim
    import torch

    def fbank(waveform, num_mel_bins=23, sample_frequency=16000.0, window_type="povey", **kwargs):
        assert not kwargs and sample_frequency == 16000 and waveform.dim() == 2 and waveform.size(0) == 1, (kwargs, sample_frequency)
        y = apc_ref.kaldi_fbank(waveform[0].double().numpy(), num_mel_bins, 25.0, 10.0, window_type)
        return torch.from_numpy(y.astype(np.float32)).to(waveform.dtype)

    mods = {n: ref_shim._Fake(n) for n in ("torchaudio", "torchaudio.compliance", "torchaudio.compliance.kaldi")}
    mods["torchaudio"].compliance = mods["torchaudio.compliance"]
    mods["torchaudio.compliance"].kaldi = mods["torchaudio.compliance.kaldi"]
    mods["torchaudio.compliance.kaldi"].fbank = fbank
    sys.modules.update(mods)
    ref_shim.import_reference()


def reference_outputs(cfg, weights, wavs):
    """The reference expert's hidden_states in fp32 and the relative distance of each to its own ``.double()`` evaluation."""
    import torch

    install_torchaudio_stand_in()
    from s3prl.upstream.decoar2 import decoar2 as model_file
    from s3prl.upstream.decoar2.expert import UpstreamExpert

    saved = dict(model_file.args)
    model_file.args.update(encoder_embed_dim=cfg.encoder_embed_dim, encoder_layers=cfg.encoder_layers, conv_pos=cfg.conv_pos,
                           conv_pos_groups=cfg.conv_pos_groups, encoder_ffn_embed_dim=cfg.encoder_ffn_embed_dim,
                           encoder_attention_heads=cfg.encoder_attention_heads)
    try:
        torch.manual_seed(0)
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "ckpt.pt")
            extra = dict(weights, **{"mask_emb": np.zeros(cfg.encoder_embed_dim, np.float32)})  # a pre-training tensor: strict=False drops it
            save_checkpoint(path, cfg, extra)
            expert = UpstreamExpert(path).eval()
    finally:
        model_file.args.clear()
        model_file.args.update(saved)
    have = expert.model.state_dict()
    assert set(have) == set(weights), sorted(set(have) ^ set(weights))
    assert all(torch.equal(have[k], torch.from_numpy(np.asarray(v)).reshape(have[k].shape)) for k, v in weights.items()), "not loaded"
    assert expert.get_downsample_rates("hidden_states") == 320 and expert.model.encoder.layerdrop == 0.0

    class Recorder(torch.nn.Module):
        """the reference's own FeatureExtractor, its outputs kept"""

        def __init__(self, inner):
            super().__init__()
            self.inner, self.kept = inner, []

        def forward(self, wav):
            self.kept.append(self.inner(wav))
            return self.kept[-1]

    class Table(torch.nn.Module):
        """stands where FeatureExtractor stood: the i-th call returns the i-th utterance's features"""

        def __init__(self, table):
            super().__init__()
            self.table, self.i = table, 0

        def forward(self, wav):
            self.i += 1
            return self.table[(self.i - 1) % len(self.table)]

    with torch.no_grad():
        expert.preprocessor = rec = Recorder(expert.preprocessor)
        out = expert([torch.from_numpy(w.copy()) for w in wavs])
        # the .double() run reads the features the fp32 run normalised (the module docstring says why)
        expert = expert.double()
        expert.preprocessor = Table([t.double() for t in rec.kept])
        out64 = expert([torch.from_numpy(w.copy()).double() for w in wavs])
    hs, hs64 = [h.numpy() for h in out["hidden_states"]], [h.numpy() for h in out64["hidden_states"]]
    assert out["last_hidden_state"] is out["hidden_states"][-1]
    return hs, [rel(a, b) for a, b in zip(hs, hs64)], list(out["_hidden_states_info"])


def rel(a, b):
    return float(np.linalg.norm(np.asarray(a, np.float64) - np.asarray(b, np.float64)) / np.linalg.norm(np.asarray(b, np.float64)))


def make_case(name: str):
    cfg_name, wseed, xseed, lengths, (ts, cs), profile = CASES[name]
    first_seed = wseed
    cfg = named_config(cfg_name)
    F = [decoar2_ref.fbank_frames(n) for n in lengths]
    T = [cfg.num_frames(n) for n in lengths]
    assert T == [decoar2_ref.num_frames(n) for n in lengths] and WANT[name](F, T), (name, F, T)
    wavs = synth_wavs(lengths, xseed)
    while True:
        weights = synth_weights(cfg, wseed, profile)
        hs, ref_err, info = reference_outputs(cfg, weights, wavs)
        proxy = [rel(a, b) for a, b in zip(decoar2_ref.forward(cfg, weights, wavs, dtype=np.float32), hs)]
        if max(ref_err) <= MAX_REF_FP32_ERR and max(proxy) <= MAX_FP32_PROXY_ERR:
            break
        print(f"{name}: weight seed {wseed}: reference fp32 vs float64 {max(ref_err):.2e} (<= {MAX_REF_FP32_ERR:g}), fp32 evaluation from "
              f"the waveforms {max(proxy):.2e} (<= {MAX_FP32_PROXY_ERR:g}): next seed")
        wseed += 1
        if wseed - first_seed >= MAX_SEEDS:
            raise SystemExit(f"{name}: no weight seed in {first_seed}..{wseed - 1} meets the acceptance rules; nothing written")
    NL, D = cfg.encoder_layers, cfg.encoder_embed_dim
    assert len(hs) == NL + 1 == cfg.num_hidden_states and all(h.shape == (len(lengths), max(T), D) for h in hs), [h.shape for h in hs]
    assert info == [f"self.model.encoder.layers[{i}]" for i in range(NL)] + ["self.model.encoder"], info
    meta = dict(config=cfg_name, weight_seed=wseed, wav_seed=xseed, lengths=lengths, fbank_frames=F, valid=T, t_stride=ts, c_stride=cs,
                dc=0.0, scale=1.0, shape=list(hs[0].shape), profile=profile, n_states=len(hs), ref_fp32_err=ref_err, fp32_proxy_err=proxy,
                reference="s3prl 0.4.18 upstream/decoar2/expert.py::UpstreamExpert.__call__, torch CPU fp32"
                          + ("" if D == 768 else ", decoar2.args narrowed"),
                stand_in="torchaudio.compliance.kaldi.fbank = tests/apc_ref.py::kaldi_fbank (float64, rounded to fp32): no torchaudio run")
    arrays = {f"hs{l}": np.ascontiguousarray(h[:, ::ts, ::cs]) for l, h in enumerate(hs)}
    arrays["norms"] = np.array([np.linalg.norm(h.astype(np.float64)) for h in hs])
    arrays["meta"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, f"{name}.npz")
    np.savez_compressed(path, **arrays)
    print(f"{name}: {len(hs)} x {hs[0].shape} F {F} T {T} weight seed {wseed} ref err {max(ref_err):.1e} fp32 proxy {max(proxy):.1e} "
          f"max|h| {np.abs(hs[-1]).max():.2f} -> {os.path.getsize(path) / 1e3:.0f} kB")


def make_hub_fixture():
    """names and signatures of the reference's decoar2 hubconf, in reference_hub_decoar.json's layout, and the released URL"""
    import importlib

    install_torchaudio_stand_in()
    mod = importlib.import_module("s3prl.upstream.decoar2.hubconf")
    res = [[n, [[k, v.kind.name, repr(v.default)] for k, v in inspect.signature(f).parameters.items()]]
           for n, f in vars(mod).items() if inspect.isfunction(f) and not n.startswith("_") and f.__module__ == mod.__name__]
    seen = {}
    mod.decoar2_url = lambda *a, **k: seen.update(k)  # record the URL, fetch nothing
    mod.decoar2()
    os.makedirs(OUT, exist_ok=True)
    with open(os.path.join(OUT, "reference_hub_decoar2.json"), "w") as f:
        json.dump(dict(reference="s3prl 0.4.18: s3prl.upstream.decoar2.hubconf", hubconfs={"decoar2": res}, downsample_rate=320,
                       urls={"decoar2": seen["ckpt"]}), f, indent=1, sort_keys=True)
        f.write("\n")
    print("reference_hub_decoar2.json", [r[0] for r in res], seen["ckpt"])


if __name__ == "__main__":
    for n in sys.argv[1:] or list(CASES) + ["hub"]:
        make_hub_fixture() if n == "hub" else make_case(n)
