#!/usr/bin/env python3
"""DeCoAR 2.0 on one MI355X: the batch-wide kaldi front end beside the per-utterance one, the time of a forward in every
operand mode beside HuBERT-base's from the same session, and every mode's error on the full-size fixture.

    python tools/decoar2_bench.py [--batch 32] [--secs 10] [--rounds 9] [--steps 20] [--warmup 3] [--no-frontend] [--no-forward] [--no-errors]

Prints one JSON object:
* ``frontend``: on ONE padded batch of ``--batch`` x ``--secs`` s and one stream, ``s3enc_op_fbank_batch`` (launch_fbank_batch: one
  GEMM, one mel launch, one CMVN launch) against ``s3enc_fbank_forward_ex`` with its ``--batch`` launch_fbank calls (a memset and
  3 kernels per utterance) on the rows of the same slab, hamming window, CMVN, no deltas.  ``--rounds`` ALTERNATING rounds of
  ``--steps`` calls each, HIP events around every call; per round the median, then the median of the round medians, the ratio
  batched / per-utterance of those, the two outputs compared bit for bit, and the average shader clock over the timed region
  (``s3enc_debug_clock_sample``).  Both entries end in work the host waits for or enqueues alike; the batched entry keeps its
  workspace between calls, the per-utterance one its per-stream scratch.
* ``forward``: per model and mode the median / min / max of ``--steps`` forwards measured alternating (one forward of every handle per
  round), the per-kernel times of separate profiled rounds (``s3enc_profile_*``), HuBERT-base's conv extractor's share of its forward
  (wav_stats + gn_stats + conv0 + gemm:conv* + layernorm:feat), and DeCoAR 2.0's front end's share of its own.
* ``errors``: per operand mode the worst per-state relative error on ``tests/golden/decoar2/pseudo.npz`` (released shape,
  pretrained-like statistics, the reference's own states) beside the bound tests/test_encoder_gpu.py holds HuBERT-base's
  pretrained-like fixtures to in that mode.
``bench.py`` stays the benchmark of the flagship workload; this tool measures the DeCoAR 2.0 family only."""

import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MODES = ("fp32", "fp32x3", "fp16x2", "fp16", "bf16")
EXTRACTOR = ("wav_stats", "gn_stats", "conv0", "layernorm:feat", "layernorm:conv")


def event_ms(fn):
    import torch

    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def clock(lib, _lib, fn):
    """fn() between two clock samples: its result and the average shader clock in GHz"""
    import torch

    clk = torch.zeros((2, 3), dtype=torch.int64, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    _lib.check(lib.s3enc_debug_clock_sample(clk[0].data_ptr(), stream))
    res = fn()
    _lib.check(lib.s3enc_debug_clock_sample(clk[1].data_ptr(), stream))
    torch.cuda.synchronize()
    a, b = clk[0].cpu().tolist(), clk[1].cpu().tolist()
    return res, (round((b[0] - a[0]) / (b[1] - a[1]) * a[2] * 1e-6, 3) if b[1] != a[1] else None)


def frontend(args):
    import numpy as np
    import torch

    from s3prl_amd import _lib
    from s3prl_amd.synth import synth_wavs

    lib = _lib.load()
    B, n = args.batch, int(args.secs * 16000)
    F = 1 + (n - 400) // 160
    cfg = _lib.S3FbankConfig(16000, 80, 25.0, 10.0, 0.97, 0, 5, 1, 1e-10)
    slab = torch.from_numpy(np.stack(synth_wavs([n] * B, 1))).cuda()
    assert slab.stride(0) % 4 == 0 and slab.data_ptr() % 16 == 0
    outs = [torch.empty((B, F, 80), device="cuda") for _ in range(2)]
    ptrs = (C.c_void_p * B)(*[slab[b].data_ptr() for b in range(B)])
    lens = (C.c_int64 * B)(*([n] * B))
    dev, stream = torch.cuda.current_device(), C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def batched():
        _lib.check(lib.s3enc_op_fbank_batch(C.byref(cfg), 1, C.c_void_p(slab.data_ptr()), slab.stride(0), lens, B, 0,
                                            C.c_void_p(outs[0].data_ptr()), 0, dev, stream), "s3enc_op_fbank_batch")

    def per_utterance():
        _lib.check(lib.s3enc_fbank_forward_ex(C.byref(cfg), 1, ptrs, lens, B, C.c_void_p(outs[1].data_ptr()), F, dev, stream),
                   "s3enc_fbank_forward_ex")

    for _ in range(args.warmup):
        batched()
        per_utterance()
    torch.cuda.synchronize()

    def rounds():
        med = {"batched": [], "per_utterance": []}
        for _ in range(args.rounds):
            for name, fn in (("batched", batched), ("per_utterance", per_utterance)):
                med[name].append(statistics.median(event_ms(fn) for _ in range(args.steps)))
        return med

    med, ghz = clock(lib, _lib, rounds)
    torch.cuda.synchronize()
    same = bool(torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32)))
    mb, mp = statistics.median(med["batched"]), statistics.median(med["per_utterance"])
    return dict(batch=B, secs=args.secs, frames_per_utterance=F, rounds=args.rounds, steps_per_round=args.steps, clock_ghz=ghz,
                batched_ms=round(mb, 4), per_utterance_ms=round(mp, 4), batched_over_per_utterance=round(mb / mp, 4),
                batched_round_medians=[round(x, 4) for x in med["batched"]],
                per_utterance_round_medians=[round(x, 4) for x in med["per_utterance"]], outputs_bit_identical=same,
                spectrum_workspace_mb=round(B * F * 2 * 257 * 4 / 1e6, 1))


def forward(args):
    import torch

    from s3prl_amd import _lib
    from s3prl_amd.encoder import HipEncoder
    from s3prl_amd.synth import named_config, synth_wavs, synth_weights

    lib = _lib.load()
    B, n = args.batch, int(args.secs * 16000)
    cfgs = {"decoar2": named_config("decoar2"), "hubert_base": named_config("hubert_base")}
    wavs = [torch.from_numpy(w).cuda() for w in synth_wavs([n] * B, 1)]
    handles = {}
    for model, cfg in cfgs.items():
        w = synth_weights(cfg, 0)
        for mode in (MODES if model == "decoar2" else ("fp32",)):
            handles[f"{model}/{mode}"] = (HipEncoder(cfg, w, dtype=mode, check="off"),
                                          torch.empty((cfg.num_hidden_states, B, cfg.num_frames(n), cfg.encoder_embed_dim), device="cuda"))

    def one_round(ms=None):
        for name, (enc, out) in handles.items():
            t = event_ms(lambda: enc.forward(wavs, out=out))
            if ms is not None:
                ms[name].append(t)

    for _ in range(args.warmup):
        one_round()
    torch.cuda.synchronize()
    ms = {name: [] for name in handles}
    _, ghz = clock(lib, _lib, lambda: [one_round(ms) for _ in range(args.steps)])
    res = dict(batch=B, secs=args.secs, steps=args.steps, warmup=args.warmup, clock_ghz=ghz, frames={m: c.num_frames(n) for m, c in cfgs.items()})
    for enc, _ in handles.values():
        enc.profile_reset()
        enc.profile_enable(1)
    prof = 3
    for _ in range(prof):
        one_round()
    for name, (enc, _) in handles.items():
        ents = enc.profile_read()
        enc.profile_enable(0)
        k = {e["name"]: round(e["ms"] / prof, 4) for e in ents}
        ent = dict(ms_median=round(statistics.median(ms[name]), 3), ms_min=round(min(ms[name]), 3), ms_max=round(max(ms[name]), 3), kernels_ms=k)
        if name.startswith("hubert_base"):
            ent["conv_extractor_ms"] = round(sum(v for kn, v in k.items() if kn in EXTRACTOR or kn.startswith("gemm:conv")), 3)
        else:
            ent["front_end_ms"] = round(k.get("decoar2_stage", 0.0) + k.get("decoar2_fbank", 0.0), 4)
        res[name] = ent
        enc.close()
    hb = res["hubert_base/fp32"]
    res["hubert_base_minus_extractor_ms"] = round(hb["ms_median"] - hb["conv_extractor_ms"], 3)
    return res


def errors(args):
    import numpy as np
    import torch

    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from conftest import load_golden
    from test_encoder_gpu import FP32_TOL, PL_16BIT_TOL

    from oracle import encoder_oracle as O
    from s3prl_amd import _lib
    from s3prl_amd.encoder import HipEncoder

    bound = dict(PL_16BIT_TOL, fp32x3=FP32_TOL, fp32=FP32_TOL)
    meta, cfg, weights, wavs, golden, norms = load_golden("decoar2/pseudo")
    ts, cs = meta["t_stride"], meta["c_stride"]
    dev = [torch.from_numpy(w).cuda() for w in wavs]
    out = {}
    for mode in MODES:
        enc = HipEncoder(cfg, weights, dtype=mode)
        hs = enc.forward(dev).cpu().numpy()
        status = enc.status()
        enc.close()
        errs = [O.rel_err(hs[l][:, ::ts, ::cs], golden[l]) for l in range(hs.shape[0])]
        out[mode] = dict(bound=bound[mode], worst_state=float(f"{max(errs):.3e}"), last_state=float(f"{errs[-1]:.3e}"),
                         finite=bool(np.isfinite(hs).all()), status=status, meets_bound=bool(max(errs) < bound[mode] and np.isfinite(hs).all()))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--secs", type=float, default=10.0)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-frontend", action="store_true")
    ap.add_argument("--no-forward", action="store_true")
    ap.add_argument("--no-errors", action="store_true")
    args = ap.parse_args()
    if args.steps < 10 or args.rounds < 3:
        ap.error("--steps must be at least 10 and --rounds at least 3 (the median of fewer runs is not a measurement)")

    import torch

    if not torch.cuda.is_available():
        raise SystemExit("decoar2_bench needs the MI355X: there is no CPU fallback and no CPU timing")
    res = {}
    if not args.no_errors:
        res["errors"] = errors(args)
    if not args.no_frontend:
        res["frontend"] = frontend(args)
    if not args.no_forward:
        res["forward"] = forward(args)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
