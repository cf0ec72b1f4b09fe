#!/usr/bin/env python3
"""Generate the SSAST fixtures under ``tests/golden/ssast/``.

    python tests/golden/make_golden_ssast.py                 # all cases
    python tests/golden/make_golden_ssast.py tiny_patch_cut
    python tests/golden/make_golden_ssast.py hub /path/to/s3prl   # the hub-signature fixture, from the reference's source text

NO RUN OF THE REFERENCE STANDS BEHIND THESE FIXTURES.  Neither timm nor torchaudio is installed here, so the reference's expert
cannot be built: the states come from the float64 restatement ``tests/ssast_ref.py`` on a ``synth.py`` checkpoint in the released
file's own key layout (``module.v.*``, the pretraining position table, ``module.p_input_fdim/tdim``, and the tensors the loader
ignores).  ``tests/test_ssast_cpu.py`` pins the restatement's pieces against torch (``nn.Conv2d``, ``nn.TransformerEncoderLayer``,
``F.interpolate``) and its front end against ``oracle/fbank_oracle.py`` with the window swapped.

Same ``.npz`` meta format as the other generators (``conftest.load_golden`` reads them as ``"ssast/<case>"``: ``n_states`` = depth,
seeds instead of weights); the states are stored as float32, sub-sampled in time and channel (``t_stride`` / ``c_stride``), with the
full tensors' norms beside them.  The hub fixture records names and signatures read off the reference's ``hubconf.py`` / ``expert.py``
with ``ast`` (they cannot be imported here), in ``reference_hub_mae_ast.json``'s layout."""

from __future__ import annotations

import ast
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))

import ssast_ref  # noqa: E402
from s3prl_amd.synth import named_config, synth_wavs, synth_weights  # noqa: E402

MAX_BYTES = 256 * 1024
W05 = 8000  # samples of a 0.5 s window

# name -> (config, weight seed, wav seed, lengths, (t_stride, c_stride), dc, scale)
CASES = {
    # 0.5 s windows, 50 tokens; the longest utterance is 2 W + 1 samples: three windows, 12 rows cut to 11; utterance 1 ends inside
    # window 1 (its window 2 is wholly silent), utterance 2 inside window 0 (two silent windows)
    "tiny_patch_cut": ("tiny_ssast_patch", 1701, 1801, [2 * W05 + 1, W05 + 900, 4000], (1, 8), 0.0, 1.0),
    # 51 tokens; W + 1 samples: two windows, 98 rows cut to 51
    "tiny_frame_cut": ("tiny_ssast_frame", 1702, 1802, [W05 + 1, 5000], (2, 1), 0.05, 0.5),
    # an utterance shorter than one 400-sample analysis window: its only window is 300 samples and zeros
    "tiny_patch_short": ("tiny_ssast_patch", 1703, 1803, [300, 7000], (1, 4), 0.0, 1.0),
    # equal lengths of exactly one window: nothing is padded, nothing is cut (4 rows of 5)
    "tiny_patch_eq": ("tiny_ssast_patch", 1703, 1804, [W05, W05], (1, 4), 0.0, 1.0),
    # the position rows interpolated in time (p_t_dim 3 < t_dim 4; 30 < 49)
    "tiny_patch_interp": ("tiny_ssast_patch_interp", 1705, 1805, [W05 + 2000, 6000], (1, 8), 0.0, 1.0),
    "tiny_frame_interp": ("tiny_ssast_frame_interp", 1706, 1806, [7000, 2 * W05], (3, 1), 0.0, 1.0),
    # D = 192 (the checkpoint's tiny width): N is no multiple of the 128-wide n-tile
    "tiny_patch_d192": ("tiny_ssast_patch_d192", 1707, 1807, [W05 + 1, 3000], (1, 8), 0.0, 1.0),
}


def make_case(name: str):
    cfg_name, wseed, xseed, lengths, (ts, cs), dc, scale = CASES[name]
    cfg = named_config(cfg_name)
    weights = synth_weights(cfg, wseed)
    wavs = synth_wavs(lengths, xseed, dc=dc, scale=scale)
    res = ssast_ref.forward(cfg, weights, wavs)
    hs = [h.astype(np.float32) for h in res["states"]]
    nmax = max(lengths)
    T = cfg.num_frames(nmax)
    nseg = cfg.ss_num_windows(nmax)
    assert all(h.shape == (len(lengths), T, cfg.ss_f_dim * cfg.encoder_embed_dim) for h in hs), [h.shape for h in hs]
    silent = [[bool(n <= s * cfg.ss_window_samples) for s in range(nseg)] for n in lengths]
    meta = dict(config=cfg_name, weight_seed=wseed, wav_seed=xseed, lengths=lengths, frames=[cfg.valid_frames(n, nmax) for n in lengths],
                steps=T, windows=nseg, tokens=2 + cfg.ss_f_dim * cfg.ss_t_dim, uncut_steps=nseg * cfg.ss_t_dim, silent_windows=silent,
                t_stride=ts, c_stride=cs, dc=dc, scale=scale, shape=list(hs[0].shape), n_states=cfg.encoder_layers,
                downsample=cfg.downsample_rate,
                reference="tests/ssast_ref.py (float64 restatement of s3prl 0.4.18 ssast/{expert,ast_models,audio}.py) on a synth.py "
                          "checkpoint in the released key layout; no run of the reference (timm and torchaudio are not installed)")
    arrays = {f"hs{l}": np.ascontiguousarray(h[:, ::ts, ::cs]) for l, h in enumerate(hs)}
    arrays["norms"] = np.array([np.linalg.norm(h.astype(np.float64)) for h in res["states"]])
    arrays["meta"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    os.makedirs(os.path.join(HERE, "ssast"), exist_ok=True)
    path = os.path.join(HERE, "ssast", f"{name}.npz")
    np.savez_compressed(path, **arrays)
    assert os.path.getsize(path) < MAX_BYTES, (path, os.path.getsize(path))
    print(f"{name}: shape {hs[0].shape} x {cfg.encoder_layers}, {nseg} windows, rows {T} of {nseg * cfg.ss_t_dim}, valid {meta['frames']} "
          f"-> {os.path.getsize(path) / 1e3:.0f} kB")


def _signature(fn: ast.FunctionDef):
    """[[name, kind, repr(default)], ...] as inspect.signature would list them"""
    empty = "<class 'inspect._empty'>"
    a = fn.args
    pos = list(a.posonlyargs) + list(a.args)
    defaults = [None] * (len(pos) - len(a.defaults)) + list(a.defaults)
    out = [[p.arg, "POSITIONAL_OR_KEYWORD", empty if d is None else repr(ast.literal_eval(d))] for p, d in zip(pos, defaults)]
    if a.vararg:
        out.append([a.vararg.arg, "VAR_POSITIONAL", empty])
    out += [[p.arg, "KEYWORD_ONLY", empty if d is None else repr(ast.literal_eval(d))] for p, d in zip(a.kwonlyargs, a.kw_defaults)]
    if a.kwarg:
        out.append([a.kwarg.arg, "VAR_KEYWORD", empty])
    return out


def make_hub_fixture(s3prl_root: str):
    """names and signatures of the reference's ssast hubconf and the expert's constructor, and the released URLs"""
    d = os.path.join(s3prl_root, "s3prl", "upstream", "ssast")
    hub = ast.parse(open(os.path.join(d, "hubconf.py")).read())
    fns = [n for n in hub.body if isinstance(n, ast.FunctionDef) and not n.name.startswith("_")]
    urls = {f.name: [c.value for c in ast.walk(f) if isinstance(c, ast.Constant) and isinstance(c.value, str) and c.value.startswith("http")][0]
            for f in fns}
    expert = ast.parse(open(os.path.join(d, "expert.py")).read())
    cls = [n for n in expert.body if isinstance(n, ast.ClassDef) and n.name == "UpstreamExpert"][0]
    init = [n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name == "__init__"][0]
    os.makedirs(os.path.join(HERE, "ssast"), exist_ok=True)
    with open(os.path.join(HERE, "ssast", "reference_hub_ssast.json"), "w") as f:
        json.dump(dict(reference="s3prl 0.4.18: s3prl.upstream.ssast.hubconf (read with ast: the module imports torchaudio and timm)",
                       hubconfs={"ssast": [[fn.name, _signature(fn)] for fn in fns]}, urls=urls, expert_init=_signature(init)), f,
                  indent=1, sort_keys=True)


if __name__ == "__main__":
    args = sys.argv[1:]
    if args[:1] == ["hub"]:
        make_hub_fixture(args[1])
    else:
        for n in args or list(CASES):
            make_case(n)
