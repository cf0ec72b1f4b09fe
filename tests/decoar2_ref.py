"""float64 numpy restatement of DeCoAR 2.0 (upstream/decoar2/{audio,decoar2,expert}.py) from the waveforms (TEST HELPER, not product
code), written from the model's definition:

* front end, per utterance: kaldi log-mel (80 bins, 25 ms / 10 ms, hamming, snip_edges), CMVN over the utterance's own F frames
  ((x - mean) / (1e-10 + unbiased std)), then rows 0, 2, 4, ...: T = ceil(F / 2);
* batch: the features zero-padded to Tmax, frames at and after T_b masked;
* model: post_extract_proj, masked rows zeroed, x + pos_conv(x), encoder.layer_norm, post-LN layers with the masked frames as padded
  keys (the reference's padding of T to a multiple of 2 adds one masked key and changes no row);
* states: the input of every layer, then the encoder output — NL + 1 of (B, Tmax, D).  Padded rows carry the reference's values.

The front end is ``apc_ref``'s (the restatement tests/test_apc_cpu.py pins), the positional conv and the layers are those of
``oracle.encoder_oracle``.  tests/test_decoar2_cpu.py holds this file to the reference-written fixtures on all rows."""

from __future__ import annotations

from typing import Dict, List

import numpy as np

import apc_ref
from oracle import encoder_oracle as O

N_MEL, SIZE, SHIFT = 80, 400, 160


def fbank_frames(n: int) -> int:
    return 0 if n < SIZE else 1 + (n - SIZE) // SHIFT


def num_frames(n: int) -> int:
    return -(-fbank_frames(n) // 2)


def logmel_cmvn(wav, dtype=np.float64) -> np.ndarray:
    """The front end in front of the subsampling: (F, 80), the CMVN over all F frames."""
    y = apc_ref.kaldi_fbank(wav, N_MEL, 25.0, 10.0, "hamming", dtype=dtype)
    return apc_ref.cmvn(y) if y.shape[0] > 0 else y


def frontend(wav, dtype=np.float64) -> np.ndarray:
    """FeatureExtractor.forward (decoar2/audio.py:69-87) on one waveform: (ceil(F / 2), 80)."""
    return logmel_cmvn(wav, dtype)[::2]


def features(wavs, dtype=np.float64, n_max=None):
    """pad_sequence of the per-utterance features (decoar2/expert.py:83-86) and their frame counts; ``n_max``: a shard of a larger
    batch, padded to that batch's frames."""
    feats = [frontend(w, dtype) for w in wavs]
    lens = [f.shape[0] for f in feats]
    T = max(lens) if n_max is None else num_frames(int(n_max))
    out = np.zeros((len(feats), T, N_MEL), dtype=dtype)
    for b, f in enumerate(feats):
        out[b, :f.shape[0]] = f
    return out, lens


def model(cfg, weights: Dict[str, np.ndarray], feats: np.ndarray, lens: List[int], dtype=np.float64) -> List[np.ndarray]:
    """Decoar2.forward behind the front end, as the expert's hooks see it."""
    assert cfg.family == "decoar2" and not cfg.layer_norm_first and cfg.pos_conv_depth == 1
    dt = np.dtype(dtype)
    W = {k: np.asarray(v).astype(dt) for k, v in weights.items()}
    x = np.asarray(feats, dtype=dt) @ W["post_extract_proj.weight"].T + W["post_extract_proj.bias"]
    for b, n in enumerate(lens):
        x[b, n:] = 0
    x = x + O.pos_conv(cfg, W, x)
    x = O.layer_norm(x, W["encoder.layer_norm.weight"], W["encoder.layer_norm.bias"])
    states = []
    for l in range(cfg.encoder_layers):
        states.append(x)
        x = O.encoder_layer(cfg, W, l, x, list(lens), None, [])
    states.append(x)
    return states


def forward(cfg, weights, wavs, n_max=None, dtype=np.float64) -> List[np.ndarray]:
    """``UpstreamExpert(ckpt)(wavs)["hidden_states"]``: NL + 1 states of (B, Tmax, D)."""
    feats, lens = features([np.asarray(w, dtype=dtype) for w in wavs], dtype, n_max)
    return model(cfg, weights, feats, lens, dtype)
