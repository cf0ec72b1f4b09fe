#!/usr/bin/env python3
"""Digest of what the encoders compute and enqueue, for comparing two builds of the library bit for bit: for every (fixture, compute
dtype, selection, sink) case the SHA-256 of every state a forward writes and the profile listing of that forward (kind, launches,
flops, bytes; the times are left out, they differ from run to run).  Two trees whose output is the same text compute the same
numbers from the same sequence of launches.  A case the library refuses prints the refusal.
usage: python tools/forward_digest.py [fixture ...] > digest.txt        (no arguments: every fixture below)
       python tools/forward_digest.py --condense digest.txt           (no GPU: one line per fixture and dtype, the SHA-256 of its lines)"""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

DTYPES = ["fp32", "fp32x3", "fp16x2", "fp16", "bf16"]
SELECTIONS = [None, "fairseq_layers", "fairseq_layers_before_residual"]
# the fixtures of tests/test_layer_schedule_gpu.py, the data2vec positional-conv stack, and one fixture of every other family
FIXTURES = ["tiny_hubert_pad", "tiny_hubert_large_pad", "tiny_wavlm_large_pad", "tiny_wavlm_pad", "tiny_wav2vec2_fsbefore", "tiny_distiller_pad",
            "tiny_multires_pad", "tiny_multires_large_pad", "tiny_multires3_pad", "mae_ast/tiny_patch_pad", "mae_ast/tiny_preln_pad",
            "mockingjay/tiny_pad", "mockingjay/tiny_albert", "mockingjay/tiny_chunk", "tiny_data2vec_pad", "lighthubert/small_ragged",
            "decoar2/tiny_ragged_odd", "conformer/conformer_relpos_tiny_pad", "conformer/conformer_rope_tiny_pad", "apc/apc_tiny_pad",
            "cpc/cpc_tiny_pad", "decoar/decoar_tiny_pad", "vggish/vggish_pad", "byol_a/byol_a_tiny_pad", "wav2vec/vq_gumbel_tiny_pad",
            "wav2vec/vq_kmeans_tiny_pad"]
TUNED = ("hubert_base_pl", "bf16")  # a post-LN 16-bit case whose fc2 is a shape of the LayerNorm 1 fold: ln1_fold x ws_inplace


def sha(t):
    a = t.detach().cpu().contiguous()
    a = a.view(dtype=__import__("torch").int16) if a.element_size() == 2 else a
    return hashlib.sha256(a.numpy().tobytes()).hexdigest()


def one(enc, dev, what, run):
    """one forward: its states' digests and its profile listing"""
    import torch

    enc.profile_reset()
    try:
        out = run()
        torch.cuda.synchronize()
    except Exception as err:  # a refusal is part of the behaviour compared
        print(f"{what}: refused: {type(err).__name__}: {err}")
        return
    states = [out] if out.dim() == 3 else list(out)
    print(f"{what}: status {enc.status()}")
    for i, s in enumerate(states):
        print(f"  state {i} {tuple(s.shape)} {str(s.dtype)[6:]} {sha(s)}")
    for p in enc.profile_read():
        print(f"  prof {p['name']} x{p['launches']} flops {p['flops']:.0f} bytes {p['bytes']:.0f}")


def cases(enc, dev, name, dtype, selections, tag=""):
    for sel in selections:
        what = f"{name} {dtype} {sel or 'hidden_states'}{tag}"
        try:
            ns = enc.num_states(sel)
        except Exception as err:
            print(f"{what}: refused: {type(err).__name__}: {err}")
            continue
        w = [(i + 1.0) / (ns * (ns + 1) / 2) for i in range(ns)]
        if ns > 2:
            w[1] = 0.0  # a state without a term
        one(enc, dev, what + " slab32", lambda: enc.forward(dev, selection=sel))
        if dtype in ("fp16x2", "fp16", "bf16"):
            one(enc, dev, what + " slab16", lambda: enc.forward(dev, selection=sel, out_dtype="fp16" if dtype == "fp16x2" else dtype))
        one(enc, dev, what + " featurize", lambda: enc.forward_featurized(dev, w, normalize=False, selection=sel))
        one(enc, dev, what + " featurize+norm", lambda: enc.forward_featurized(dev, w, normalize=True, selection=sel))


def condense(path):
    """a digest as one line per (fixture, dtype): forwards, refusals and the SHA-256 of that part of the text"""
    parts = {}
    for line in open(path):
        if not line.startswith("  "):
            key = " ".join(line.split(":")[0].split()[:2])
        parts.setdefault(key, []).append(line)
    for key, lines in parts.items():
        text = "".join(lines)
        print(f"{key}: {text.count(': status ')} forwards, {text.count(': refused: ')} refusals, {len(lines)} lines, "
              f"sha256 {hashlib.sha256(text.encode()).hexdigest()}")


def main():
    if sys.argv[1:2] == ["--condense"]:
        return condense(sys.argv[2])
    import torch

    from conftest import load_golden
    from s3prl_amd import _lib
    from s3prl_amd.encoder import HipEncoder

    for name in sys.argv[1:] or FIXTURES + [TUNED[0]]:
        meta, cfg, weights, wavs = load_golden(name)[:4]
        dev = [torch.from_numpy(np.asarray(w, np.float32)).cuda() for w in wavs]
        for dtype in DTYPES if name != TUNED[0] else [TUNED[1]]:
            try:
                enc = HipEncoder(cfg, weights, dtype=dtype)
            except Exception as err:
                print(f"{name} {dtype}: refused: {type(err).__name__}: {err}")
                continue
            enc.profile_enable(True)
            if name != TUNED[0]:
                cases(enc, dev, name, dtype, SELECTIONS)
            else:
                lib = _lib.load()
                try:
                    for fold in (1, 0):
                        for inplace in (1, 0):
                            _lib.check(lib.s3enc_set_tuning(b"ln1_fold", fold))
                            _lib.check(lib.s3enc_set_tuning(b"ws_inplace", inplace))
                            cases(enc, dev, name, dtype, SELECTIONS[:1], f" ln1_fold={fold} ws_inplace={inplace}")
                finally:
                    _lib.check(lib.s3enc_set_tuning(b"ln1_fold", 1))
                    _lib.check(lib.s3enc_set_tuning(b"ws_inplace", 1))
            enc.close()


if __name__ == "__main__":
    main()
