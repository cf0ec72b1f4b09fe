#!/usr/bin/env python3
"""Modified CPC on one MI355X: the time of a forward, per-kernel times, and the recurrent kernel against its L2-stream floor.

    python tools/cpc_bench.py [--config cpc_base] [--batch 32] [--secs 10] [--steps 20] [--warmup 3] [--no-torch]

Prints one JSON object: the median of ``--steps`` forwards (HIP events around each, after ``--warmup`` untimed ones) with the
average shader clock of the timed region, the per-kernel times of separate profiled forwards (``s3enc_profile_*``), the recurrent
kernel's microseconds per step beside the floor derived from streaming W_hh from L2 once per step (gates * H * H * 4 bytes at
34.5 TB/s / 256 CUs per workgroup), and — the yardstick — the same model built from ``torch.nn.Conv1d`` / ``nn.LSTM`` / ``nn.GRU``
on the same GPU.  ``bench.py`` stays the benchmark of the flagship workload; this tool measures the CPC family only."""

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

L2_BYTES_PER_S_PER_CU = 34.5e12 / 256  # MI355X: ~34.5 TB/s of L2 bandwidth over 256 CUs


def torch_model(cfg, weights, dev):
    """The reference architecture from torch's own layers (channel norm with the unbiased variance), fp32, on the GPU."""
    import torch

    class ChannelNorm(torch.nn.Module):
        def __init__(self, g, b):
            super().__init__()
            self.g, self.b = torch.nn.Parameter(g), torch.nn.Parameter(b)

        def forward(self, x):
            return (x - x.mean(1, keepdim=True)) * torch.rsqrt(x.var(1, keepdim=True) + 1e-5) * self.g + self.b

    t = lambda n: torch.from_numpy(weights[n]).to(dev)  # noqa: E731
    layers, cin = [], 1
    for i, ((C, k, s), p) in enumerate(zip(cfg.conv_layers, cfg.conv_pads)):
        conv = torch.nn.Conv1d(cin, C, k, stride=s, padding=p).to(dev)
        with torch.no_grad():
            conv.weight.copy_(t(f"gEncoder.conv{i}.weight"))
            conv.bias.copy_(t(f"gEncoder.conv{i}.bias"))
        layers += [conv, ChannelNorm(t(f"gEncoder.batchNorm{i}.weight"), t(f"gEncoder.batchNorm{i}.bias")), torch.nn.ReLU()]
        cin = C
    enc = torch.nn.Sequential(*layers)
    ar = (torch.nn.LSTM if cfg.ar_mode == "LSTM" else torch.nn.GRU)(cfg.conv_dim, cfg.ar_hidden, num_layers=cfg.ar_layers,
                                                                    batch_first=True).to(dev)
    with torch.no_grad():
        for l in range(cfg.ar_layers):
            for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"):
                getattr(ar, f"{n}_l{l}").copy_(t(f"gAR.baseNet.{n}_l{l}"))
    ar.flatten_parameters()

    def forward(padded):
        with torch.no_grad():
            z = enc(padded.unsqueeze(1)).transpose(1, 2).contiguous()
            return z, ar(z)[0]

    return forward


def timed(fn, steps, warmup):
    """per-call milliseconds (HIP events) of `steps` calls after `warmup` untimed ones"""
    import torch

    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="cpc_base")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--secs", type=float, default=10.0)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-torch", action="store_true")
    args = ap.parse_args()
    if args.steps < 20:
        ap.error("--steps must be at least 20 (the median of fewer forwards is not a measurement)")

    import numpy as np
    import torch

    from oracle import encoder_oracle as O
    from s3prl_amd import _lib
    from s3prl_amd.encoder import HipEncoder
    from s3prl_amd.synth import named_config, synth_wavs, synth_weights

    if not torch.cuda.is_available():
        raise SystemExit("cpc_bench needs the MI355X: there is no CPU fallback and no CPU timing")
    dev = torch.device("cuda", 0)
    cfg = named_config(args.config)
    weights = synth_weights(cfg, 0)
    n = int(args.secs * 16000)
    B = args.batch
    wavs = [torch.from_numpy(w).to(dev) for w in synth_wavs([n] * B, 1)]
    T, H = cfg.num_frames(n), cfg.ar_hidden
    G = 4 if cfg.ar_mode == "LSTM" else 3
    enc = HipEncoder(cfg, weights, check="off")
    out = torch.empty((2, B, T, H), device=dev)
    lib = _lib.load()
    clk = torch.zeros((2, 3), dtype=torch.int64, device=dev)
    cs = torch.cuda.current_stream(dev).cuda_stream
    for _ in range(args.warmup):
        enc.forward(wavs, out=out)
    torch.cuda.synchronize()
    _lib.check(lib.s3enc_debug_clock_sample(clk[0].data_ptr(), cs))
    ms = timed(lambda: enc.forward(wavs, out=out), args.steps, 0)
    _lib.check(lib.s3enc_debug_clock_sample(clk[1].data_ptr(), cs))
    torch.cuda.synchronize()
    a, b = clk[0].cpu().tolist(), clk[1].cpu().tolist()
    ghz = (b[0] - a[0]) / (b[1] - a[1]) * a[2] * 1e-6 if a[2] > 0 and b[2] == a[2] and b[1] > a[1] else None

    prof_steps = 5
    enc.profile_reset()
    enc.profile_enable(1)
    for _ in range(prof_steps):
        enc.forward(wavs, out=out)
    kernels = {e["name"]: dict(ms_per_step=round(e["ms"] / prof_steps, 4), launches_per_step=e["launches"] // prof_steps)
               for e in enc.profile_read()}
    enc.profile_enable(0)
    rnn = next((v for k, v in kernels.items() if k.startswith("rnn_")), None)
    floor_us = G * H * H * 4 / L2_BYTES_PER_S_PER_CU * 1e6
    res = dict(config=args.config, batch=B, secs=args.secs, frames=T, steps=args.steps, warmup=args.warmup,
               ms_median=round(statistics.median(ms), 3), ms_min=round(min(ms), 3), ms_max=round(max(ms), 3),
               clock_ghz=round(ghz, 3) if ghz else None, kernels=kernels,
               rnn_us_per_step=round(rnn["ms_per_step"] * 1e3 / (cfg.ar_layers * T), 3) if rnn else None,
               rnn_l2_stream_floor_us_per_step=round(floor_us, 3))
    if not args.no_torch:
        fwd = torch_model(cfg, weights, dev)
        padded = torch.stack(wavs)
        tms = timed(lambda: fwd(padded), args.steps, args.warmup)
        z, c = fwd(padded)
        res["torch_ms_median"] = round(statistics.median(tms), 3)
        res["torch_over_ours"] = round(statistics.median(tms) / statistics.median(ms), 3)
        res["rel_err_vs_torch"] = [O.rel_err(out[0].cpu().numpy(), z.cpu().numpy()), O.rel_err(out[1].cpu().numpy(), c.cpu().numpy())]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
