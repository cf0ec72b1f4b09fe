#!/usr/bin/env python3
"""VGGish on one MI355X: the time of a forward, per-kernel times with the convolutions' share of the fp32-MFMA roofline, and torch's
modules for scale.

    python tools/vggish_bench.py [--config vggish] [--batch 32] [--secs 10] [--steps 20] [--warmup 3] [--no-torch]

Prints one JSON object:
* the median / min / max of ``--steps`` forwards of TWO handles of the same configuration and of the same model as torch-ROCm ``nn``
  modules (``Conv2d``, ``MaxPool2d``, ``Linear``, fp32, fed the log-mel examples our front end produced: torch has no part of the
  reference's numpy front end on the GPU), measured ALTERNATING — one forward of every entry per round, HIP events around each, after
  ``--warmup`` untimed rounds — so that clock drift hits every entry alike; the two handles give the run-to-run spread that a
  difference has to exceed;
* the per-kernel times of separate profiled forwards (``s3enc_profile_*``): front end, first layer, each convolution, each Linear,
  the ReLU passes and the quantiser, with launches, FLOPs, TFLOP/s and, for the convolutions, the fraction of ``--peak-tflops``
  (155: the fp32-MFMA peak, DESIGN §4's roofline denominator);
* torch's per-layer times of the same modules (HIP events around every module, a run of its own).
``bench.py`` stays the benchmark of the flagship workload; this tool measures the VGGish family only."""

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def torch_model(cfg, weights, dev):
    """VGG's features and embeddings as torch's own nn modules, fp32, on the GPU (channel-first, as the reference runs them)."""
    import torch

    nn = torch.nn
    mods, cin = [], 1
    for i, (ch, pool) in enumerate(cfg.vg_layers):
        conv = nn.Conv2d(cin, ch, 3, padding=1)
        conv.weight.data = torch.from_numpy(weights[f"features.{cfg.vg_seq_index(i)}.weight"])
        conv.bias.data = torch.from_numpy(weights[f"features.{cfg.vg_seq_index(i)}.bias"])
        mods.append((f"conv{i}" + ("+pool" if pool else ""), nn.Sequential(conv, nn.ReLU(True), *([nn.MaxPool2d(2, 2)] if pool else []))))
        cin = ch

    class Flatten(nn.Module):
        def forward(self, x):  # vggish.py:34-39
            return x.transpose(1, 3).transpose(1, 2).contiguous().view(x.size(0), -1)

    mods.append(("flatten", Flatten()))
    for j, i in enumerate((0, 2, 4)):
        w = weights[f"embeddings.{i}.weight"]
        lin = nn.Linear(w.shape[1], w.shape[0])
        lin.weight.data, lin.bias.data = torch.from_numpy(w), torch.from_numpy(weights[f"embeddings.{i}.bias"])
        mods.append((f"fc{j}", nn.Sequential(lin, nn.ReLU(True))))
    mods = [(n, m.to(dev).eval()) for n, m in mods]

    def forward(x, times=None):
        with torch.no_grad():
            for name, m in mods:
                if times is not None:
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                x = m(x)
                if times is not None:
                    b.record()
                    times.setdefault(name, []).append((a, b))
        return x

    return forward


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="vggish")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--secs", type=float, default=10.0)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--peak-tflops", type=float, default=155.0)
    ap.add_argument("--no-torch", action="store_true")
    args = ap.parse_args()
    if args.steps < 20:
        ap.error("--steps must be at least 20 (the median of fewer forwards is not a measurement)")

    import torch

    from s3prl_amd.encoder import HipEncoder
    from s3prl_amd.synth import named_config, synth_wavs, synth_weights

    if not torch.cuda.is_available():
        raise SystemExit("vggish_bench needs the MI355X: there is no CPU fallback and no CPU timing")
    dev = torch.device("cuda", 0)
    cfg = named_config(args.config)
    weights = synth_weights(cfg, 0)
    n = int(args.secs * 16000)
    B = args.batch
    wavs = [torch.from_numpy(w).to(dev) for w in synth_wavs([n] * B, 1)]
    E, D = cfg.num_frames(n), cfg.vg_fc[2]
    encs = [HipEncoder(cfg, weights, check="off") for _ in range(2)]
    outs = [torch.empty((1, B, E, D), device=dev) for _ in encs]
    entries = [("ours", lambda i=i: encs[i].forward(wavs, out=outs[i])) for i in range(2)]
    if not args.no_torch:
        encs[0].forward(wavs, out=outs[0])
        logmel = torch.from_numpy(encs[0].debug_tap("logmel")).to(dev).view(B * E, cfg.vg_example_frames + 2, cfg.vg_num_mel_bins + 2)
        x = logmel[:, 1:-1, 1:-1].unsqueeze(1).contiguous()  # (B E, 1, frames, bands), as the reference feeds its model
        fwd = torch_model(cfg, weights, dev)
        entries.append(("torch_modules", lambda: fwd(x)))
    for _ in range(args.warmup):
        for _, f in entries:
            f()
    torch.cuda.synchronize()
    ms = [[] for _ in entries]
    for _ in range(args.steps):  # alternating: one forward of every entry per round
        for i, (_, f) in enumerate(entries):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            b.synchronize()
            ms[i].append(a.elapsed_time(b))
    res = dict(config=args.config, batch=B, secs=args.secs, examples=B * E, steps=args.steps, warmup=args.warmup,
               same_values_both_handles=bool((outs[0] == outs[1]).all()),
               entries=[dict(name=name, ms_median=round(statistics.median(m), 3), ms_min=round(min(m), 3), ms_max=round(max(m), 3))
                        for (name, _), m in zip(entries, ms)])
    res["same_form_spread_ms"] = round(abs(res["entries"][0]["ms_median"] - res["entries"][1]["ms_median"]), 3)

    prof_steps = 5
    enc = encs[0]
    enc.profile_reset()
    enc.profile_enable(1)
    for _ in range(prof_steps):
        enc.forward(wavs, out=outs[0])
    kernels = {}
    for e in enc.profile_read():
        k = dict(ms_per_step=round(e["ms"] / prof_steps, 4), launches_per_step=e["launches"] // prof_steps)
        if e.get("flops"):
            k["gflop_per_step"] = round(e["flops"] / prof_steps / 1e9, 2)
            tf = e["flops"] / (e["ms"] * 1e-3) / 1e12 if e["ms"] > 0 else None
            k["tflops"] = round(tf, 1) if tf else None
            if e["name"].startswith("conv2d3x3:L") and tf:
                k["fraction_of_fp32_mfma_peak"] = round(tf / args.peak_tflops, 3)
        kernels[e["name"]] = k
    enc.profile_enable(0)
    res["kernels"] = kernels
    conv = [v for k, v in kernels.items() if k.startswith("conv2d3x3:L")]
    if conv and sum(v["ms_per_step"] for v in conv) > 0:
        res["conv_layers_fraction_of_fp32_mfma_peak"] = round(
            sum(v["gflop_per_step"] for v in conv) / sum(v["ms_per_step"] for v in conv) / args.peak_tflops, 3)  # GFLOP / ms = TFLOP/s
    if not args.no_torch:
        times = {}
        for _ in range(prof_steps):
            fwd(x, times)
        torch.cuda.synchronize()
        res["torch_layers_ms"] = {k: round(statistics.median(a.elapsed_time(b) for a, b in v), 4) for k, v in times.items()}
        res["torch_modules_over_our_forward"] = round(res["entries"][2]["ms_median"] / res["entries"][0]["ms_median"], 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
