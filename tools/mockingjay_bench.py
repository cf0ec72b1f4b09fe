#!/usr/bin/env python3
"""Mockingjay / TERA / AudioALBERT on one MI355X: the time of a forward, per-kernel times, the front end beside its HBM floor.

    python tools/mockingjay_bench.py [--config tera_base] [--batch 32] [--secs 10,10,15] [--steps 20] [--warmup 3]

Prints one JSON object:
* per entry of ``--secs`` the median / min / max of ``--steps`` forwards, measured ALTERNATING — one forward of every entry per round,
  HIP events around each, after ``--warmup`` untimed rounds — so that clock drift hits every entry alike; a length listed twice (the
  default lists 10 s twice) gives the run-to-run spread; 15 s is T = 1501 > sequence_length = 1500: the chunked path (751 + 750);
* the per-kernel times of separate profiled forwards of every distinct length (``s3enc_profile_*``), the time of one Transformer
  layer (everything but the front end, the input representation and the state emission, over the layer count), and the front end
  (decibel scale + pad, DFT GEMM, mel / log, CMVN) beside its derived HBM floor: PCM in, the padded signal written and read, the
  spectrum written and read, the features written, read and written by the CMVN, at the measured float4 copy rate of 6.29 TB/s.
``bench.py`` stays the benchmark of the flagship workload; this tool measures the Mockingjay family only."""

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_COPY_BYTES_PER_S = 6.29e12  # MI355X: measured float4 copy


def frontend_floor_bytes(B, n, T, n_mels):
    sig = B * (n + 400)
    return 4.0 * (B * n * 2          # PCM: read by the rms pass and by the pad pass
                  + sig * 2          # the padded signal: written, read by the GEMM (the overlap is served by the caches)
                  + B * T * 402 * 2  # the spectrum: written, read
                  + B * T * n_mels * 4)  # the features: written by mel / log, read twice and written once by the two-pass CMVN


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="tera_base")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--secs", default="10,10,15")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    if args.steps < 20:
        ap.error("--steps must be at least 20 (the median of fewer forwards is not a measurement)")

    import torch

    from s3prl_amd.encoder import HipEncoder
    from s3prl_amd.synth import named_config, synth_wavs, synth_weights

    if not torch.cuda.is_available():
        raise SystemExit("mockingjay_bench needs the MI355X: there is no CPU fallback and no CPU timing")
    dev = torch.device("cuda", 0)
    cfg = named_config(args.config)
    weights = synth_weights(cfg, 0)
    B, D, NL = args.batch, cfg.encoder_embed_dim, cfg.encoder_layers
    secs = [float(s) for s in args.secs.split(",")]
    encs, outs, wavs, frames = [], [], [], []
    for s in secs:  # one handle per entry
        n = int(s * 16000)
        encs.append(HipEncoder(cfg, weights, check="off"))
        wavs.append([torch.from_numpy(w).to(dev) for w in synth_wavs([n] * B, 1)])
        frames.append(cfg.num_frames(n))
        outs.append(torch.empty((NL + 1, B, frames[-1], D), device=dev))
    for _ in range(args.warmup):
        for enc, w, out in zip(encs, wavs, outs):
            enc.forward(w, out=out)
    torch.cuda.synchronize()
    ms = [[] for _ in secs]
    for _ in range(args.steps):  # alternating: one forward of every entry per round
        for i, (enc, w, out) in enumerate(zip(encs, wavs, outs)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            enc.forward(w, out=out)
            b.record()
            b.synchronize()
            ms[i].append(a.elapsed_time(b))
    entries, seen = [], {}
    prof_steps = 5
    for i, s in enumerate(secs):
        T = frames[i]
        sizes = [T] if not cfg.mj_sequence_length or T <= cfg.mj_sequence_length else None
        if sizes is None:
            n0 = -(-T // cfg.mj_sequence_length)
            tc = -(-T // n0)
            sizes = [min(tc, T - k) for k in range(0, T, tc)]
        ent = dict(secs=s, frames=T, chunks=sizes, ms_median=round(statistics.median(ms[i]), 3), ms_min=round(min(ms[i]), 3),
                   ms_max=round(max(ms[i]), 3), finite=bool(torch.isfinite(outs[i]).all()))
        if s not in seen:
            enc = encs[i]
            enc.profile_reset()
            enc.profile_enable(1)
            for _ in range(prof_steps):
                enc.forward(wavs[i], out=outs[i])
            seen[s] = {e["name"]: dict(ms_per_forward=round(e["ms"] / prof_steps, 4), launches_per_forward=e["launches"] // prof_steps)
                       for e in enc.profile_read()}
            enc.profile_enable(0)
            k = seen[s]
            ent["kernels"] = k
            front = k.get("mj_logmel") or k.get("mj_fbank")
            outside = sum(k[name]["ms_per_forward"] for name in ("mj_logmel", "mj_fbank", "gemm:mj_in", "emit_state") if name in k)
            ln = k.get("layernorm_eps", {}).get("ms_per_forward", 0.0)
            total = sum(v["ms_per_forward"] for v in k.values())
            # the input representation's LayerNorm is one of 2 NL + 1 launches of the same kernel
            ent["ms_per_layer_profiled"] = round((total - outside - ln / (2 * NL + 1)) / NL, 4)
            if front and cfg.mj_frontend == "mel":
                floor_ms = frontend_floor_bytes(B, int(s * 16000), T, cfg.mj_input_dim) / HBM_COPY_BYTES_PER_S * 1e3
                ent["frontend_ms"] = front["ms_per_forward"]
                ent["frontend_hbm_floor_ms"] = round(floor_ms, 4)
                ent["frontend_over_floor"] = round(front["ms_per_forward"] / floor_ms, 2)
        entries.append(ent)
    res = dict(config=args.config, batch=B, steps=args.steps, warmup=args.warmup, entries=entries)
    same = [e["ms_median"] for e in entries if e["secs"] == secs[0]]
    if len(same) >= 2:
        res["same_length_spread_ms"] = round(max(same) - min(same), 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
