"""Writes tests/golden/lighthubert/*.npz and reference_hub_lighthubert.json by RUNNING THE REFERENCE's own LightHuBERT expert
(s3prl/upstream/lighthubert/expert.py::UpstreamExpert) on the CPU, on checkpoints written from seeds: the supernet state dict
``s3prl_amd.synth.synth_weights`` draws for the named configuration, saved by ``s3prl_amd.ckpt.save_checkpoint`` in the layout the
released files have.  Needs the reference tree (tests/golden/ref_shim.py says where); no test imports this file.

    python tools/make_lighthubert_goldens.py [case ...]

Fixture layout = tests/golden/make_golden.py's: ``meta`` (JSON: config, seeds, lengths, strides), ``hs<l>`` = state l subsampled
[:, ::t_stride, ::c_stride], ``norms`` = the Frobenius norm of every full state."""
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
OUT = os.path.join(ROOT, "tests", "golden", "lighthubert")

from s3prl_amd.ckpt import save_checkpoint  # noqa: E402
from s3prl_amd.synth import named_config, synth_wavs, synth_weights  # noqa: E402

# name -> (config, weight seed, wav seed, lengths, (t_stride, c_stride), profile)
CASES = {
    "base_ragged": ("lighthubert_base", 1, 71, [6200, 4321, 3000], (2, 8), "synthetic"),        # odd T, three ragged lengths
    "base_equal": ("lighthubert_base", 2, 72, [5840, 5840], (2, 8), "synthetic"),
    "base_two_tiles": ("lighthubert_base", 3, 73, [41999, 20000], (8, 16), "synthetic"),         # T >= 129: two pos-conv frame tiles
    "small_ragged": ("lighthubert_small", 4, 74, [6319, 3500, 4777], (2, 4), "synthetic"),
    "small_one_frame": ("lighthubert_small", 5, 75, [4000, 300], (1, 4), "synthetic"),           # one valid frame beside 12
    "stage1": ("lighthubert_stage1", 6, 76, [4500, 3333], (2, 8), "synthetic"),                  # student_hubert: the max subnet
    "base_pl": ("lighthubert_base", 7, 77, [6000, 4100], (2, 8), "pretrained_like"),
}
# what each case is there for, checked on the frame counts before anything runs: (T parity or minimum, valid frames)
WANT = {"base_ragged": lambda T, v: T % 2 == 1 and len(set(v)) == 3, "base_equal": lambda T, v: T % 2 == 0 and len(set(v)) == 1,
        "base_two_tiles": lambda T, v: T >= 129, "small_ragged": lambda T, v: len(set(v)) == 3,
        "small_one_frame": lambda T, v: min(v) == 1 and max(v) == T, "stage1": lambda T, v: True, "base_pl": lambda T, v: True}


def reference_expert(path):
    import ref_shim

    ref_shim.import_reference()
    from s3prl.upstream.lighthubert.expert import UpstreamExpert

    return UpstreamExpert(path).eval()


def make_case(name):
    import torch

    cfg_name, wseed, xseed, lengths, (ts, cs), profile = CASES[name]
    cfg = named_config(cfg_name)
    T = cfg.num_frames(max(lengths))
    valid = [cfg.valid_frames(n, max(lengths)) for n in lengths]
    assert WANT[name](T, valid), (name, T, valid)
    weights = synth_weights(cfg, wseed, profile)
    wavs = synth_wavs(lengths, xseed)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "ckpt.pt")
        save_checkpoint(path, cfg, weights)
        expert = reference_expert(path)
        assert expert.get_downsample_rates("hidden_states") == 320
        with torch.no_grad():
            out = expert([torch.from_numpy(w.copy()) for w in wavs])
    assert list(out) == ["hidden_states"]
    hs = [h.numpy() for h in out["hidden_states"]]
    assert len(hs) == 13 and hs[0].shape == (len(lengths), T, cfg.encoder_embed_dim), (len(hs), hs[0].shape)
    meta = dict(config=cfg_name, weight_seed=wseed, wav_seed=xseed, lengths=lengths, t_stride=ts, c_stride=cs, dc=0.0, scale=1.0,
                shape=list(hs[0].shape), valid=valid, profile=profile, n_states=len(hs),
                reference="s3prl 0.4.18 upstream/lighthubert/expert.py::UpstreamExpert, torch CPU fp32")
    arrays = {f"hs{l}": np.ascontiguousarray(h[:, ::ts, ::cs]) for l, h in enumerate(hs)}
    arrays["norms"] = np.array([np.linalg.norm(h.astype(np.float64)) for h in hs])
    arrays["meta"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, f"{name}.npz")
    np.savez_compressed(path, **arrays)
    print(f"{name}: {len(hs)} x {hs[0].shape} valid {valid} -> {os.path.getsize(path) / 1e3:.0f} kB")


def make_reference_hub():
    import importlib
    import inspect

    import ref_shim

    ref_shim.import_reference()
    conf = importlib.import_module("s3prl.upstream.lighthubert.hubconf")
    entries, urls = [], {}
    for name, fn in vars(conf).items():
        if name.startswith("_") or not inspect.isfunction(fn) or fn.__module__ != conf.__name__:
            continue
        entries.append([name, [[k, v.kind.name, repr(v.default)] for k, v in inspect.signature(fn).parameters.items()]])
    seen = {}
    conf.lighthubert_url = lambda ckpt, refresh=False, *a, **k: seen.setdefault("url", ckpt)  # record the URL, fetch nothing
    for name in ("lighthubert_small", "lighthubert_base", "lighthubert_stage1"):
        seen.clear()
        getattr(conf, name)()
        urls[name] = seen["url"]
    out = dict(reference="s3prl 0.4.18: s3prl.upstream.lighthubert.hubconf", hubconfs={"lighthubert": entries}, urls=urls)
    os.makedirs(OUT, exist_ok=True)
    with open(os.path.join(OUT, "reference_hub_lighthubert.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("reference_hub_lighthubert.json", len(entries), "entries")


if __name__ == "__main__":
    for n in sys.argv[1:] or (list(CASES) + ["reference_hub"]):
        make_reference_hub() if n == "reference_hub" else make_case(n)
