#!/usr/bin/env python3
"""NPC on one MI355X: the time of a forward, per-kernel times, both forms of the masked convolutions, and torch's modules for scale.

    python tools/npc_bench.py [--config npc_360hr] [--batch 32] [--secs 10] [--steps 20] [--warmup 3] [--forms 1,1,0] [--no-torch]

Prints one JSON object:
* per entry of ``--forms`` (the tuning key ``npc_skip_taps``: 1 = the masked convolutions walk their two runs of live taps only,
  0 = the same kernel over all k taps on weights with zeros in the hole) the median / min / max of ``--steps`` forwards, measured
  ALTERNATING — one forward of every entry per round, HIP events around each, after ``--warmup`` untimed rounds — so that clock
  drift hits every entry alike; an entry listed twice (the default lists 1 twice) gives the run-to-run spread that a difference
  between the two forms has to exceed;
* the per-kernel times of separate profiled forwards of every distinct entry (``s3enc_profile_*``): the three convolution shapes
  with their launches, FLOPs and TFLOP/s;
* the same modules (``conv1d``, ``batch_norm`` in eval mode, the activations, the masked weights multiplied out) in torch-ROCm fp32
  on the same GPU, on unit-variance features.
``bench.py`` stays the benchmark of the flagship workload; this tool measures the NPC family only."""

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def torch_model(cfg, weights, dev):
    """NPC's blocks from torch's own functions, fp32, on the GPU (channel-first, as the reference runs them)."""
    import torch

    F = torch.nn.functional
    g = {k: torch.from_numpy(v).to(dev) for k, v in weights.items()}
    act = torch.relu if cfg.npc_activate == "relu" else torch.tanh
    k = cfg.npc_kernel_size
    for i in range(cfg.npc_blocks):
        if cfg.npc_has_mask(i):
            m, w = cfg.npc_mask(i), g[f"masked_convs.{i}.conv.weight"].clone()
            w[:, :, (k - m) // 2:(k - m) // 2 + m] = 0
            g[f"masked_convs.{i}.masked"] = w

    def bn(y, p):
        return F.batch_norm(y, g[p + ".running_mean"], g[p + ".running_var"], g[p + ".weight"], g[p + ".bias"], False, 0.1, 1e-5)

    def forward(x):
        with torch.no_grad():
            x, feat = x.transpose(1, 2), None
            for i in range(cfg.npc_blocks):
                p = f"blocks.{i}."
                y = F.conv1d(x, g[p + "conv.weight"], g[p + "conv.bias"], padding=1)
                y = act(bn(y, p + "bn1") if cfg.npc_batch_norm else y)
                y = F.conv1d(y, g[p + "linear.weight"], g[p + "linear.bias"])
                y = bn(y, p + "bn2") if cfg.npc_batch_norm else y
                x = act(y + x if (cfg.npc_residual and i > 0) else y)
                if cfg.npc_has_mask(i):
                    mk = torch.tanh(F.conv1d(x, g[f"masked_convs.{i}.masked"], g[f"masked_convs.{i}.conv.bias"], padding=(k - 1) // 2))
                    feat = mk if feat is None else feat + mk
            return feat

    return forward


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="npc_360hr")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--secs", type=float, default=10.0)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--forms", default="1,1,0")
    ap.add_argument("--no-torch", action="store_true")
    args = ap.parse_args()
    if args.steps < 20:
        ap.error("--steps must be at least 20 (the median of fewer forwards is not a measurement)")

    import torch

    from s3prl_amd import _lib
    from s3prl_amd.encoder import HipEncoder
    from s3prl_amd.synth import named_config, synth_wavs, synth_weights

    if not torch.cuda.is_available():
        raise SystemExit("npc_bench needs the MI355X: there is no CPU fallback and no CPU timing")
    dev = torch.device("cuda", 0)
    cfg = named_config(args.config)
    weights = synth_weights(cfg, 0)
    n = int(args.secs * 16000)
    B = args.batch
    wavs = [torch.from_numpy(w).to(dev) for w in synth_wavs([n] * B, 1)]
    T, H, NS = cfg.num_frames(n), cfg.conv_dim, cfg.num_hidden_states
    lib = _lib.load()
    forms = [int(s) for s in args.forms.split(",")]
    encs, outs = [], []
    for f in forms:  # one handle per entry, each with its own tuning
        enc = HipEncoder(cfg, weights, check="off")
        _lib.check(lib.s3enc_set_handle_tuning(enc._h, b"npc_skip_taps", f), "s3enc_set_handle_tuning")
        encs.append(enc)
        outs.append(torch.empty((NS, B, T, H), device=dev))
    for _ in range(args.warmup):
        for enc, out in zip(encs, outs):
            enc.forward(wavs, out=out)
    torch.cuda.synchronize()
    ms = [[] for _ in forms]
    for _ in range(args.steps):  # alternating: one forward of every entry per round
        for i, (enc, out) in enumerate(zip(encs, outs)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            enc.forward(wavs, out=out)
            b.record()
            b.synchronize()
            ms[i].append(a.elapsed_time(b))
    same = [bool((outs[0] == o).all()) for o in outs]

    entries, seen = [], {}
    prof_steps = 5
    for i, f in enumerate(forms):
        ent = dict(npc_skip_taps=f, ms_median=round(statistics.median(ms[i]), 3), ms_min=round(min(ms[i]), 3), ms_max=round(max(ms[i]), 3),
                   same_values_as_first=same[i])
        if f not in seen:
            enc = encs[i]
            enc.profile_reset()
            enc.profile_enable(1)
            for _ in range(prof_steps):
                enc.forward(wavs, out=outs[i])
            seen[f] = {}
            for e in enc.profile_read():
                k = dict(ms_per_step=round(e["ms"] / prof_steps, 4), launches_per_step=e["launches"] // prof_steps)
                if e.get("flops"):
                    k["gflop_per_step"] = round(e["flops"] / prof_steps / 1e9, 2)
                    k["tflops"] = round(e["flops"] / (e["ms"] * 1e-3) / 1e12, 1) if e["ms"] > 0 else None
                seen[f][e["name"]] = k
            enc.profile_enable(0)
            ent["kernels"] = seen[f]
        entries.append(ent)
    res = dict(config=args.config, batch=B, secs=args.secs, frames=T, states=NS, steps=args.steps, warmup=args.warmup, entries=entries)
    base = [e["ms_median"] for e in entries if e["npc_skip_taps"] == forms[0]]
    if len(base) >= 2:
        res["same_form_spread_ms"] = round(max(base) - min(base), 3)
    if not args.no_torch:
        fwd = torch_model(cfg, weights, dev)
        x = torch.randn((B, T, cfg.apc_feat_dim), device=dev)  # unit variance, like the CMVN'd log-mel features
        for _ in range(args.warmup):
            fwd(x)
        torch.cuda.synchronize()
        tms = []
        for _ in range(args.steps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fwd(x)
            b.record()
            b.synchronize()
            tms.append(a.elapsed_time(b))
        res["torch_modules_ms_median"] = round(statistics.median(tms), 3)
        res["torch_modules_over_our_forward"] = round(statistics.median(tms) / entries[0]["ms_median"], 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
