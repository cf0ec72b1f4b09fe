#!/usr/bin/env python3
"""APC on one MI355X: the time of a forward, per-kernel times, both forms of the length-aware recurrence, and torch's GRU for scale.

    python tools/apc_bench.py [--config apc_360hr] [--batch 32] [--secs 10] [--steps 20] [--warmup 3] [--splits 0,0,8,4] [--no-torch]

Prints one JSON object:
* per entry of ``--splits`` (the tuning key ``rnn_split``: 0 = one launch per layer, S = the step-split form with S workgroups per
  utterance) the median / min / max of ``--steps`` forwards, measured ALTERNATING — one forward of every entry per round, HIP events
  around each, after ``--warmup`` untimed rounds — so that clock drift hits every entry alike; an entry listed twice (the default
  lists 0 twice) gives the run-to-run spread that a difference between two forms has to exceed;
* the per-kernel times of separate profiled forwards of every distinct entry (``s3enc_profile_*``), the recurrence's microseconds
  per step beside the floor derived from streaming W_hh from L2 once per step (3 H^2 * 4 bytes at 34.5 TB/s / 256 CUs for the
  one-launch form; a 1 / S slice of it for the step form);
* ``torch.nn.GRU`` layers (with the residual additions) on the same features on the same GPU.
``bench.py`` stays the benchmark of the flagship workload; this tool measures the APC family only."""

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

L2_BYTES_PER_S_PER_CU = 34.5e12 / 256  # MI355X: ~34.5 TB/s of L2 bandwidth over 256 CUs


def torch_model(cfg, weights, dev):
    """The GRU stack from torch's own layers, fp32, on the GPU (equal lengths: packing is the identity)."""
    import torch

    H = cfg.conv_dim
    layers = []
    for l in range(cfg.apc_layers):
        g = torch.nn.GRU(cfg.apc_feat_dim if l == 0 else H, H, batch_first=True).to(dev)
        with torch.no_grad():
            for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"):
                getattr(g, f"{n}_l0").copy_(torch.from_numpy(weights[f"rnn_layers.{l}.{n}_l0"]).to(dev))
        g.flatten_parameters()
        layers.append(g)

    def forward(x):
        with torch.no_grad():
            outs = []
            for l, g in enumerate(layers):
                y = g(x)[0]
                x = y + x if (cfg.apc_residual and l > 0) else y
                outs.append(x)
            return outs

    return forward


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="apc_360hr")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--secs", type=float, default=10.0)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--splits", default="0,0,8")
    ap.add_argument("--no-torch", action="store_true")
    args = ap.parse_args()
    if args.steps < 20:
        ap.error("--steps must be at least 20 (the median of fewer forwards is not a measurement)")

    import torch

    from s3prl_amd import _lib
    from s3prl_amd.encoder import HipEncoder
    from s3prl_amd.synth import named_config, synth_wavs, synth_weights

    if not torch.cuda.is_available():
        raise SystemExit("apc_bench needs the MI355X: there is no CPU fallback and no CPU timing")
    dev = torch.device("cuda", 0)
    cfg = named_config(args.config)
    weights = synth_weights(cfg, 0)
    n = int(args.secs * 16000)
    B = args.batch
    wavs = [torch.from_numpy(w).to(dev) for w in synth_wavs([n] * B, 1)]
    T, H = cfg.num_frames(n), cfg.conv_dim
    lib = _lib.load()
    splits = [int(s) for s in args.splits.split(",")]
    encs, outs = [], []
    for S in splits:  # one handle per entry, each with its own tuning
        enc = HipEncoder(cfg, weights, check="off")
        _lib.check(lib.s3enc_set_handle_tuning(enc._h, b"rnn_split", S), "s3enc_set_handle_tuning")
        encs.append(enc)
        outs.append(torch.empty((3, B, T, H), device=dev))
    for _ in range(args.warmup):
        for enc, out in zip(encs, outs):
            enc.forward(wavs, out=out)
    torch.cuda.synchronize()
    ms = [[] for _ in splits]
    for _ in range(args.steps):  # alternating: one forward of every entry per round
        for i, (enc, out) in enumerate(zip(encs, outs)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            enc.forward(wavs, out=out)
            b.record()
            b.synchronize()
            ms[i].append(a.elapsed_time(b))
    same_bits = [bool(torch.equal(outs[0], o)) for o in outs]

    floor_us = 3 * H * H * 4 / L2_BYTES_PER_S_PER_CU * 1e6
    entries, seen = [], {}
    prof_steps = 5
    for i, S in enumerate(splits):
        ent = dict(rnn_split=S, ms_median=round(statistics.median(ms[i]), 3), ms_min=round(min(ms[i]), 3), ms_max=round(max(ms[i]), 3),
                   same_bits_as_first=same_bits[i])
        if S not in seen:
            enc = encs[i]
            enc.profile_reset()
            enc.profile_enable(1)
            for _ in range(prof_steps):
                enc.forward(wavs, out=outs[i])
            seen[S] = {e["name"]: dict(ms_per_step=round(e["ms"] / prof_steps, 4), launches_per_step=e["launches"] // prof_steps)
                       for e in enc.profile_read()}
            enc.profile_enable(0)
            rnn = seen[S].get("rnn_gru_len")
            ent["kernels"] = seen[S]
            ent["rnn_us_per_step"] = round(rnn["ms_per_step"] * 1e3 / (cfg.apc_layers * T), 3) if rnn else None
            ent["rnn_l2_stream_floor_us_per_step"] = round(floor_us / max(S, 1), 3)
        entries.append(ent)
    res = dict(config=args.config, batch=B, secs=args.secs, frames=T, steps=args.steps, warmup=args.warmup, entries=entries)
    base = [e["ms_median"] for e in entries if e["rnn_split"] == 0]
    if len(base) >= 2:
        res["one_launch_spread_ms"] = round(max(base) - min(base), 3)
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
        res["torch_gru_stack_ms_median"] = round(statistics.median(tms), 3)
        res["torch_gru_stack_over_our_forward"] = round(statistics.median(tms) / entries[0]["ms_median"], 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
