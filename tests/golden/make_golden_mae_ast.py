#!/usr/bin/env python3
"""Generate the MAE-AST fixtures under ``tests/golden/mae_ast/`` by RUNNING THE REFERENCE (PyTorch CPU) on seeded weights and waveforms.

Run in the build container only (it imports the reference tree through ``ref_shim``):

    python tests/golden/make_golden_mae_ast.py                 # all cases + the hub-signature fixture
    python tests/golden/make_golden_mae_ast.py tiny_patch_pad

NO torchaudio RUN STANDS BEHIND THE FRONT END OF THESE FIXTURES.  torchaudio is not installed here, and the reference's expert calls
``torchaudio.compliance.kaldi.fbank``.  The generator writes a ``synth.py`` checkpoint FILE (the full strict state dict: decoder, mask
embeddings, both sinusoidal tables, BatchNorm statistics), builds the reference's ``UpstreamExpert`` on it — ``load_state_dict(...,
strict=True)`` passes — calls ``.eval()`` (otherwise the BatchNorm would use batch statistics) and replaces ONLY
``expert.wav_to_spectrogram`` with the float32 cast of ``oracle/fbank_oracle.py::kaldi_fbank(num_mel_bins=128)``.  Everything else —
``pad_sequence``, the BatchNorm, ``nn.Unfold``, ``forward_padding_mask``, the sinusoidal rows, the Transformer encoder, the reshape and
the cut — is the reference's own code.

Same ``.npz`` meta format as the other generators (``conftest.load_golden`` reads them as ``"mae_ast/<case>"``: ``n_states`` =
encoder_layers, seeds instead of weights).  The tiny cases are recorded whole; the full-size ones sub-sampled in time and channel
(``t_stride`` / ``c_stride``) with the full tensors' norms beside them.  A case is written only when the float64 restatement
``tests/mae_ast_ref.py`` stays within a quarter of the GPU tests' ``FP32_TOL`` = 1e-4 of the reference's output, whole and per
(utterance, time step) row; both figures are in the meta (``restatement_err`` / ``restatement_row_err``), next to the reference's own
``padding_mask.sum(-1)`` (``mask_sums``, recorded as data).
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

import mae_ast_ref  # noqa: E402
from oracle.fbank_oracle import kaldi_fbank  # noqa: E402
from s3prl_amd.ckpt import save_checkpoint  # noqa: E402
from s3prl_amd.synth import named_config, synth_wavs, synth_weights  # noqa: E402

FP32_TOL = 1e-4
MAX_RESTATEMENT_ERR = 0.25 * FP32_TOL
MAX_BYTES = 256 * 1024

# name -> (config, weight seed, wav seed, lengths, (t_stride, c_stride), dc, scale)
CASES = {
    # 16 x 16, equal lengths: the mask rule's fast exit; F = 51, three time steps
    "tiny_patch_eq": ("tiny_mae_ast", 1401, 1501, [8400, 8400], (1, 1), 0.0, 1.0),
    # F = 61 (61 % 16 != 0: 13 frames never read), 36 (mask index 24 = Ttok: masks nothing), 20 (second patch partly real), 16 (exact)
    "tiny_patch_pad": ("tiny_mae_ast", 1401, 1502, [10000, 6000, 3500, 2800], (1, 1), 0.0, 1.0),
    # 2 x 128: F = 23 (one frame never read), 13 (last step partly real), 22 (index 11 = Ttok)
    "tiny_frame_pad": ("tiny_mae_ast_frame", 1402, 1503, [4000, 2340, 3850], (1, 1), 0.05, 0.5),
    # layer_norm_first, three layers: F = 54, 23 (partly real), 42 (index reaches Ttok)
    "tiny_preln_pad": ("tiny_mae_ast_preln", 1403, 1504, [9000, 4000, 7000], (1, 1), 0.0, 1.0),
    # kt = 3, kc = 32: F = 29 (two frames never read), 11 (partly real), 26 (index 36 = Ttok)
    "tiny_k3x32_pad": ("tiny_mae_ast_k3x32", 1404, 1505, [5000, 2000, 4500], (1, 1), 0.0, 1.0),
    # the released shapes (their position tables cut to 1024 rows), three utterances of at most 2.5 s: F = 248, 198, 54
    "mae_ast_patch_pseudo": ("mae_ast_patch_t1024", 1405, 1506, [40000, 32001, 9000], (3, 32), 0.0, 1.0),
    "mae_ast_frame_pseudo": ("mae_ast_frame_t1024", 1406, 1507, [40000, 32001, 9000], (8, 12), 0.0, 1.0),
}


def _import_reference():
    import ref_shim

    ref_shim.import_reference(roots=("torchaudio", "omegaconf"))


def rel(a, b):
    return float(np.linalg.norm(np.asarray(a, np.float64) - np.asarray(b, np.float64)) / np.linalg.norm(np.asarray(b, np.float64)))


def reference_expert(cfg, weights, tmpdir):
    import torch

    _import_reference()
    from s3prl.upstream.mae_ast.expert import UpstreamExpert

    path = os.path.join(tmpdir, "mae_ast.pt")
    save_checkpoint(path, cfg, weights)
    expert = UpstreamExpert(path).eval()
    assert not expert.model.batch_norm.training
    expert.wav_to_spectrogram = lambda wav: torch.from_numpy(
        kaldi_fbank(wav[0].double().numpy(), num_mel_bins=expert.feature_dim).astype(np.float32))
    assert expert.get_downsample_rates("hidden_states") == cfg.downsample_rate
    seen = {}
    inner = expert.model.forward

    def spy(*a, **k):
        res = inner(*a, **k)
        seen["mask_sums"] = [int(v) for v in res["padding_mask"].sum(-1)]
        return res

    expert.model.forward = spy
    return expert, seen


def make_case(name: str):
    import torch

    cfg_name, wseed, xseed, lengths, (ts, cs), dc, scale = CASES[name]
    cfg = named_config(cfg_name)
    weights = synth_weights(cfg, wseed)
    wavs = synth_wavs(lengths, xseed, dc=dc, scale=scale)
    with tempfile.TemporaryDirectory() as tmp:
        expert, seen = reference_expert(cfg, weights, tmp)
        with torch.no_grad():
            out = expert([torch.from_numpy(w.copy()) for w in wavs])
    hs = [h.numpy() for h in out["hidden_states"]]
    NL, V, D = cfg.encoder_layers, cfg.ma_tokens_per_step, cfg.encoder_embed_dim
    Tt = cfg.num_frames(max(lengths))
    assert len(hs) == NL and all(h.shape == (len(lengths), Tt, V * D) and h.dtype == np.float32 for h in hs), [h.shape for h in hs]
    mine = mae_ast_ref.forward(cfg, weights, wavs, feature_dtype=np.float32)
    err = max(rel(m, h) for m, h in zip(mine["states"], hs))
    row_err = max(rel(m[b, t], h[b, t]) for m, h in zip(mine["states"], hs) for b in range(h.shape[0]) for t in range(Tt))
    assert err <= MAX_RESTATEMENT_ERR and row_err <= MAX_RESTATEMENT_ERR, (name, err, row_err)
    Ttok = Tt * V
    assert [Ttok - k for k in mine["kv"]] == seen["mask_sums"], (mine["kv"], seen["mask_sums"])
    valid = [cfg.valid_frames(n, max(lengths)) for n in lengths]
    meta = dict(config=cfg_name, weight_seed=wseed, wav_seed=xseed, lengths=lengths, fbank_frames=mine["frames"], frames=valid,
                steps=Tt, tokens=Ttok, mask_sums=seen["mask_sums"], t_stride=ts, c_stride=cs, dc=dc, scale=scale, shape=list(hs[0].shape),
                n_states=NL, downsample=cfg.downsample_rate,
                reference="s3prl 0.4.18 mae_ast/expert.py (.eval()), torch CPU fp32, built on a synth.py checkpoint file (strict load); "
                          "wav_to_spectrogram replaced by the float32 cast of oracle kaldi_fbank (no torchaudio run)",
                restatement_err=err, restatement_row_err=row_err)
    arrays = {f"hs{l}": np.ascontiguousarray(h[:, ::ts, ::cs]) for l, h in enumerate(hs)}
    arrays["norms"] = np.array([np.linalg.norm(h.astype(np.float64)) for h in hs])
    arrays["meta"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    os.makedirs(os.path.join(HERE, "mae_ast"), exist_ok=True)
    path = os.path.join(HERE, "mae_ast", f"{name}.npz")
    np.savez_compressed(path, **arrays)
    assert os.path.getsize(path) < MAX_BYTES, (path, os.path.getsize(path))
    print(f"{name}: shape {hs[0].shape} x {NL}, valid steps {valid}, mask sums {seen['mask_sums']}, mae_ast_ref float64 vs reference "
          f"{err:.2e} whole / {row_err:.2e} worst row -> {os.path.getsize(path) / 1e3:.0f} kB")


def make_hub_fixture():
    """names and signatures of the reference's mae_ast hubconf, in reference_hub_byol_a.json's layout"""
    _import_reference()
    import importlib

    mod = importlib.import_module("s3prl.upstream.mae_ast.hubconf")
    sig = lambda f: [[k, v.kind.name, repr(v.default)] for k, v in inspect.signature(f).parameters.items()]  # noqa: E731
    res = {"mae_ast": [[n, sig(f)] for n, f in vars(mod).items()
                       if inspect.isfunction(f) and not n.startswith("_") and f.__module__ == mod.__name__]}
    expert = importlib.import_module("s3prl.upstream.mae_ast.expert").UpstreamExpert
    os.makedirs(os.path.join(HERE, "mae_ast"), exist_ok=True)
    with open(os.path.join(HERE, "mae_ast", "reference_hub_mae_ast.json"), "w") as f:
        json.dump(dict(reference="s3prl 0.4.18: s3prl.upstream.mae_ast.hubconf", hubconfs=res, expert_init=sig(expert.__init__)), f,
                  indent=1, sort_keys=True)


if __name__ == "__main__":
    names = sys.argv[1:] or list(CASES) + ["hub"]
    for n in names:
        make_hub_fixture() if n == "hub" else make_case(n)
