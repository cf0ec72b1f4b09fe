#!/usr/bin/env python3
"""Generate the fixtures under ``tests/golden/spectral/`` by RUNNING THE REFERENCE (PyTorch CPU) on seeded waveforms.

Run in the build container only (it imports the reference tree):

    python tests/golden/make_golden_spectral.py

``stft_mag_*.npz``    the reference's ``upstream/log_stft`` expert on its two yaml settings: torch alone stands behind them.
``linear_*.npz``, ``mel_*.npz``   the reference's ``OnlinePreprocessor`` behind its baseline expert (``linear.yaml``, ``mel.yaml``).
    torchaudio is not installed, so a stand-in ``torchaudio`` module OF OUR OWN sits in ``sys.modules``: ``MFCC`` is a placeholder
    that returns zeros of the right shape (the expert never selects it), ``MelScale`` multiplies by the float32 cast of
    ``tests/spectral_ref.py::htk_bank`` exactly as torchaudio's does (``matmul(spec.transpose(-1, -2), fb).transpose(-1, -2)``) —
    so NO torchaudio RUN stands behind the ``mel`` bank; the STFT, the last-non-zero rule, the log, the CMVN, the expert's length
    ratio and ``pad_sequence`` are the reference's own code.  The meta records this (``stand_in``).
``reference_hub_spectral.json``   the signatures of the five hub entries.

The inputs are rebuilt from the meta by ``tests/spectral_ref.py::fixture_wavs``."""

from __future__ import annotations

import inspect
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import spectral_ref as R  # noqa: E402

OUT = os.path.join(HERE, "spectral")
REFERENCE = "/root/reference"

STFT_LENGTHS = [3200, 1000, 319, 257]  # 11, 4, 1, 1 frames
LOGMEL_LENGTHS = [1000, 900, 300]
# name -> meta of the inputs
PREPROC_CASES = {
    "plain": dict(lengths=LOGMEL_LENGTHS, wav_seed=4300, order=[0, 1, 2]),
    "short_first": dict(lengths=LOGMEL_LENGTHS, wav_seed=4300, order=[2, 0, 1]),  # ratio 7 / 300 > 1 / 160: the clip at T binds
    # L' = [830, 900, 300]: counts [6, 6, 2] of T = 7, so pad_sequence leaves 6 rows and the ratio is 6 / 1000
    "zero_tail": dict(lengths=LOGMEL_LENGTHS, wav_seed=4300, order=[0, 1, 2], zero_tail={"0": 170}),
    "all_zero": dict(lengths=LOGMEL_LENGTHS, wav_seed=4300, order=[0, 1, 2], zero_tail={"1": 900}),
}


def _stand_in_torchaudio():
    import torch

    class MelScale(torch.nn.Module):
        def __init__(self, sample_rate=16000, n_mels=128, n_stft=201, **kwargs):
            super().__init__()
            self.register_buffer("fb", torch.from_numpy(R.htk_bank(n_mels, n_stft, sample_rate / 2.0)).float())

        def forward(self, specgram):
            return torch.matmul(specgram.transpose(-1, -2), self.fb).transpose(-1, -2)

    class MFCC(torch.nn.Module):  # placeholder: zeros of torchaudio's shape (..., n_mfcc, 1 + L // hop)
        def __init__(self, sample_rate=16000, n_mfcc=40, melkwargs=None, **kwargs):
            super().__init__()
            self.n_mfcc, self.hop = n_mfcc, melkwargs["hop_length"]

        def forward(self, wavs):
            return wavs.new_zeros(*wavs.shape[:-1], self.n_mfcc, 1 + wavs.size(-1) // self.hop)

    class Placeholder(torch.nn.Module):
        def __init__(self, *args, **kwargs):
            super().__init__()

    ta, fn, tr, co = (types.ModuleType(n) for n in ("torchaudio", "torchaudio.functional", "torchaudio.transforms",
                                                     "torchaudio.compliance"))
    fn.compute_deltas = lambda x, *a, **k: (_ for _ in ()).throw(NotImplementedError("stand-in torchaudio"))
    tr.MelScale, tr.MFCC, tr.Spectrogram, tr.ComputeDeltas = MelScale, MFCC, Placeholder, Placeholder
    ta.functional, ta.transforms, ta.compliance = fn, tr, co
    for m in (ta, fn, tr, co):
        sys.modules[m.__name__] = m


def _save(name, meta, out):
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, meta=np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8), out=out.astype(np.float32))
    print(f"{name}: {out.shape}, {os.path.getsize(path)} bytes, restatement err {meta['restatement_err']:.2e}")


def _err(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float(np.abs(got - ref).max())


def main():
    import torch

    _stand_in_torchaudio()
    import ref_shim

    ref_shim.install(("omegaconf",))
    sys.path.insert(0, REFERENCE)
    from s3prl.upstream.baseline import expert as base_expert
    from s3prl.upstream.baseline import hubconf as base_hub
    from s3prl.upstream.log_stft import expert as stft_expert
    from s3prl.upstream.log_stft import hubconf as stft_hub
    from s3prl_amd.synth import synth_wavs

    torch.manual_seed(0)
    for name, log in (("stft_mag", False), ("log_stft_mag", True)):
        yaml_path = os.path.join(REFERENCE, "s3prl", "upstream", "log_stft", name + ".yaml")
        expert = stft_expert.UpstreamExpert(yaml_path)
        stft_expert.device  # the module-level device: cpu here
        meta = dict(lengths=STFT_LENGTHS, wav_seed=5100, log=log, settings=expert.config, reference="log_stft/expert.py, torch only")
        wavs = synth_wavs(STFT_LENGTHS, 5100)
        with torch.no_grad():
            res = expert([torch.from_numpy(w) for w in wavs])
        assert isinstance(res["last_hidden_state"], list) and len(res["last_hidden_state"]) == 1
        out = res["hidden_states"][0].numpy()
        assert out.shape == (4, 11, 257)
        meta["restatement_err"] = _err(R.stft_mag_forward(wavs, log=log), out)
        _save("stft_mag_" + ("log" if log else "lin"), meta, out)

    for kind in ("linear", "mel"):
        yaml_path = os.path.join(REFERENCE, "s3prl", "upstream", "baseline", kind + ".yaml")
        import yaml

        with open(yaml_path) as f:
            settings = yaml.safe_load(f)  # (the expert adds a `target` block to its own copy)
        expert = base_expert.UpstreamExpert(yaml_path)
        assert expert.get_downsample_rates("x") == 160
        for case, inputs in PREPROC_CASES.items():
            meta = dict(inputs, kind=kind, settings=settings, reference="baseline/expert.py + preprocessor.py",
                        stand_in="torchaudio is a stand-in module: MFCC returns zeros (never selected), MelScale multiplies by the "
                                 "float32 cast of tests/spectral_ref.py::htk_bank as torchaudio's does; no torchaudio run")
            wavs = R.fixture_wavs(meta)
            with torch.no_grad():
                out = expert([torch.from_numpy(w) for w in wavs])["hidden_states"][0].numpy()
            ref = R.preproc_forward(kind, wavs)
            meta["trimmed"] = R.trimmed_lengths(wavs)
            meta["T"], meta["counts"], meta["rows"], meta["kept"] = R.preproc_rules([len(w) for w in wavs], meta["trimmed"])
            assert out.shape[1] == max(meta["kept"])
            meta["restatement_err"] = _err(ref, out)
            _save(f"{kind}_{case}", meta, out)

    def sig(f):
        return [[k, v.kind.name, repr(v.default)] for k, v in inspect.signature(f).parameters.items()]

    hub = {"hubconfs": {"baseline": [[n, sig(getattr(base_hub, n))] for n in ("spectrogram", "mfcc", "mel", "linear")],
                        "log_stft": [["stft_mag", sig(stft_hub.stft_mag)]]},
           "output_dims": {"spectrogram": 257, "mfcc": 39, "mel": 80, "linear": 201, "stft_mag": 257},
           "downsample_rates": {"spectrogram": 160, "mfcc": 160, "mel": 160, "linear": 160, "stft_mag": 320}}
    with open(os.path.join(OUT, "reference_hub_spectral.json"), "w") as f:
        json.dump(hub, f, indent=1)


if __name__ == "__main__":
    main()
