#!/usr/bin/env python3
"""LightHuBERT on one MI355X in exact fp32: the time of a forward per subnet, the per-kernel split, HuBERT-base from the same
session as the yardstick, and the positional conv at group widths 40 and 24 against the 48- and 32-wide launches that zero-padding
would use instead.

    python tools/lighthubert_bench.py [--batch 32] [--secs 10] [--steps 20] [--warmup 3] [--prof-rounds 5]

Prints one JSON object:
* ``forward``: per model (``lighthubert_base`` 640 wide, ``lighthubert_small`` 384, ``hubert_base`` 768, and ``hubert_512``: a HuBERT
  encoder 512 wide — the shape of the small supernet's largest subnet and the home of ``posconv_kernel<32>`` at D = 512) the median /
  min / max of ``--steps`` forwards measured ALTERNATING — one forward of every model per round, HIP events around each, after
  ``--warmup`` untimed rounds — so that clock drift hits every model alike, the FLOPs the kernels report and both ratios to
  HuBERT-base (time and FLOPs);
* ``kernels``: the per-kernel times (``s3enc_profile_*``: HIP events around every launch) of ``--prof-rounds`` further alternating
  rounds;
* ``posconv``: from those profiled rounds the positional conv's time per launch at B x T frames, K = 128, G = 16 for the four group
  widths, the two ratios the narrow kernel is held to (40 over 48, 24 over 32: at most 1 means it beats zero-padding) and its share
  of the fp32 MFMA peak counting only useful FLOPs (2 B T D Dg K over 157.3 TFLOP/s);
* ``clock_ghz``: the average shader clock over the timed region (``s3enc_debug_clock_sample``).
``bench.py`` stays the benchmark of the flagship workload; this tool measures the LightHuBERT family only."""

import argparse
import dataclasses
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FP32_MFMA_PEAK = 157.3e12  # v_mfma_f32_16x16x4_f32, 256 CUs at 2.4 GHz


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--secs", type=float, default=10.0)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--prof-rounds", type=int, default=5)
    args = ap.parse_args()
    if args.steps < 20:
        ap.error("--steps must be at least 20 (the median of fewer forwards is not a measurement)")

    import torch

    from s3prl_amd import _lib
    from s3prl_amd.encoder import HipEncoder
    from s3prl_amd.synth import named_config, synth_wavs, synth_weights

    if not torch.cuda.is_available():
        raise SystemExit("lighthubert_bench needs the MI355X: there is no CPU fallback and no CPU timing")
    dev = torch.device("cuda", 0)
    hb = named_config("hubert_base")
    h512 = dataclasses.replace(hb, encoder_embed_dim=512, encoder_attention_heads=8, encoder_ffn_embed_dim=2048)
    models = {"lighthubert_base": named_config("lighthubert_base"), "lighthubert_small": named_config("lighthubert_small"),
              "hubert_base": hb, "hubert_512": h512}
    n, B = int(args.secs * 16000), args.batch
    encs, outs, wavs = {}, {}, {}
    for name, cfg in models.items():
        cfg.validate()
        encs[name] = HipEncoder(cfg, synth_weights(cfg, 0), dtype="fp32", check="off")
        T = cfg.num_frames(n)
        outs[name] = torch.empty((cfg.num_hidden_states, B, T, cfg.encoder_embed_dim), device=dev)
        wavs[name] = [torch.from_numpy(w).to(dev) for w in synth_wavs([n] * B, 1)]
    lib = _lib.load()
    stream = torch.cuda.current_stream(dev).cuda_stream
    clk = torch.zeros((2, 3), dtype=torch.int64, device=dev)

    def round_of_forwards(ms=None):
        for name, enc in encs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            enc.forward(wavs[name], out=outs[name])
            b.record()
            b.synchronize()
            if ms is not None:
                ms[name].append(a.elapsed_time(b))

    for _ in range(args.warmup):
        round_of_forwards()
    torch.cuda.synchronize()
    ms = {name: [] for name in encs}
    _lib.check(lib.s3enc_debug_clock_sample(clk[0].data_ptr(), stream))
    for _ in range(args.steps):
        round_of_forwards(ms)
    _lib.check(lib.s3enc_debug_clock_sample(clk[1].data_ptr(), stream))
    torch.cuda.synchronize()
    a, b = clk[0].cpu().tolist(), clk[1].cpu().tolist()
    ghz = (b[0] - a[0]) / (b[1] - a[1]) * a[2] * 1e-6 if b[1] != a[1] else None

    for enc in encs.values():
        enc.profile_reset()
        enc.profile_enable(1)
    for _ in range(args.prof_rounds):
        round_of_forwards()
    kernels, flops = {}, {}
    for name, enc in encs.items():
        ents = enc.profile_read()
        enc.profile_enable(0)
        kernels[name] = {e["name"]: dict(ms_per_step=round(e["ms"] / args.prof_rounds, 4), launches_per_step=e["launches"] // args.prof_rounds,
                                         **({"tflops": round(e["flops"] / (e["ms"] * 1e-3) / 1e12, 1)} if e["flops"] and e["ms"] > 0 else {}))
                         for e in ents}
        flops[name] = sum(e["flops"] for e in ents) / args.prof_rounds

    med = {name: statistics.median(v) for name, v in ms.items()}
    forward = {name: dict(embed_dim=models[name].encoder_embed_dim, ms_median=round(med[name], 3), ms_min=round(min(ms[name]), 3),
                          ms_max=round(max(ms[name]), 3), gflop_per_step=round(flops[name] / 1e9, 1),
                          time_over_hubert_base=round(med[name] / med["hubert_base"], 4),
                          flop_over_hubert_base=round(flops[name] / flops["hubert_base"], 4)) for name in encs}
    T = models["hubert_base"].num_frames(n)
    pc = {}
    for name, cfg in models.items():
        D, dg = cfg.encoder_embed_dim, cfg.encoder_embed_dim // cfg.conv_pos_groups
        t = kernels[name]["posconv"]["ms_per_step"]
        useful = 2.0 * B * T * D * dg * cfg.conv_pos
        pc[f"dg{dg}"] = dict(model=name, D=D, ms=t, useful_gflop=round(useful / 1e9, 2), useful_tflops=round(useful / (t * 1e-3) / 1e12, 1),
                             share_of_fp32_mfma_peak=round(useful / (t * 1e-3) / FP32_MFMA_PEAK, 3))
    pc["dg40_over_dg48"] = round(pc["dg40"]["ms"] / pc["dg48"]["ms"], 4)
    pc["dg24_over_dg32"] = round(pc["dg24"]["ms"] / pc["dg32"]["ms"], 4)
    print(json.dumps(dict(batch=B, secs=args.secs, frames=T, steps=args.steps, warmup=args.warmup, prof_rounds=args.prof_rounds,
                          clock_ghz=round(ghz, 3) if ghz else None, forward=forward, posconv=pc, kernels=kernels)))


if __name__ == "__main__":
    main()
