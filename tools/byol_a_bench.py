#!/usr/bin/env python3
"""BYOL-A on one MI355X: the time of a forward in its forms, per-kernel times with the convolutions' share of the fp32-MFMA roofline,
and torch's modules (``torch.stft`` front end included) for scale.

    python tools/byol_a_bench.py [--config byol_a_2048] [--batch 32] [--secs 10] [--steps 20] [--warmup 3] [--no-torch]

Prints one JSON object:
* the median / min / max of ``--steps`` forwards of FOUR handles of the same configuration and weights — two with the default tuning
  (their difference is the run-to-run spread a comparison has to exceed), one with ``melspec_fft = 0`` (the front end as an
  overlapping-row GEMM), one with ``conv2d_n64 = 0`` (conv2 / conv3 on the 128-wide n-tile) — and of the same model as torch-ROCm
  modules, measured ALTERNATING: one forward of every entry per round, HIP events around each, after ``--warmup`` untimed rounds;
* per-kernel times of separate profiled forwards of the default, the GEMM-form and the 128-wide handle (``s3enc_profile_*``), with
  FLOPs, TFLOP/s and, for the MFMA convolutions, the fraction of ``--peak-tflops`` (155: the fp32-MFMA peak, DESIGN §4's roofline
  denominator); the front end's TFLOP/s counts the arithmetic of its own form.
``bench.py`` stays the benchmark of the flagship workload; this tool measures the BYOL-A family only."""

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def torch_model(cfg, weights, dev):
    """the reference's forward as torch's own ops on the GPU, fp32: segments -> torch.stft -> mel -> log -> norm -> AudioNTT2020"""
    import numpy as np
    import torch

    import byol_a_ref as R

    nn = torch.nn
    d, window, stride = cfg.conv_layers[0]
    feats, cin = [], 1
    for k in (0, 4, 8):
        conv, bn = nn.Conv2d(cin, 64, 3, padding=1), nn.BatchNorm2d(64)
        conv.weight.data, conv.bias.data = torch.from_numpy(weights[f"features.{k}.weight"]), torch.from_numpy(weights[f"features.{k}.bias"])
        bn.weight.data, bn.bias.data = torch.from_numpy(weights[f"features.{k + 1}.weight"]), torch.from_numpy(weights[f"features.{k + 1}.bias"])
        bn.running_mean.data = torch.from_numpy(weights[f"features.{k + 1}.running_mean"])
        bn.running_var.data = torch.from_numpy(weights[f"features.{k + 1}.running_var"])
        feats += [conv, bn, nn.ReLU(), nn.MaxPool2d(2, 2)]
        cin = 64
    features = nn.Sequential(*feats).to(dev).eval()
    fc0, fc3 = nn.Linear(512, d), nn.Linear(d, d)
    fc0.weight.data, fc0.bias.data = torch.from_numpy(weights["fc.0.weight"]), torch.from_numpy(weights["fc.0.bias"])
    fc3.weight.data, fc3.bias.data = torch.from_numpy(weights["fc.3.weight"]), torch.from_numpy(weights["fc.3.bias"])
    fc = nn.Sequential(fc0, nn.ReLU(), fc3, nn.ReLU()).to(dev).eval()
    fb = torch.from_numpy(R.mel_bank(np.float32)).to(dev)
    win = torch.hann_window(1024, device=dev)
    eps = torch.finfo(torch.float).eps

    def forward(wavs, times=None):
        def timed(name, f):
            if times is None:
                return f()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            y = f()
            b.record()
            times.setdefault(name, []).append((a, b))
            return y

        with torch.no_grad():
            n_max = max(len(w) for w in wavs)
            starts = list(range(0, n_max, stride))
            padded = torch.stack([torch.nn.functional.pad(w, (0, starts[-1] + window - len(w))) for w in wavs])
            segs = torch.stack([padded[:, s:s + window] for s in starts], dim=1).reshape(-1, window)  # (B S, window)

            def front():
                spec = torch.stft(segs, 1024, 160, 1024, window=win, center=True, pad_mode="reflect", return_complex=True).abs().pow(2.0)
                mel = torch.matmul(spec.transpose(1, 2), fb).transpose(1, 2)  # (B S, 64, frames)
                return (((mel + eps).log() - R.MEAN) / R.STD).unsqueeze(1)

            x = timed("front_end", front)
            x = timed("features", lambda: features(x))

            def head():
                y = x.permute(0, 3, 2, 1)
                y = fc(y.reshape(y.shape[0], y.shape[1], -1))
                return (y.max(dim=1).values + y.mean(dim=1)).reshape(len(wavs), len(starts), -1)

            return timed("fc_and_tail", head)

    return forward


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="byol_a_2048")
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

    from s3prl_amd import _lib
    from s3prl_amd.encoder import HipEncoder
    from s3prl_amd.synth import named_config, synth_wavs, synth_weights

    if not torch.cuda.is_available():
        raise SystemExit("byol_a_bench needs the MI355X: there is no CPU fallback and no CPU timing")
    dev = torch.device("cuda", 0)
    cfg = named_config(args.config)
    weights = synth_weights(cfg, 0)
    n = int(args.secs * 16000)
    B = args.batch
    wavs = [torch.from_numpy(w).to(dev) for w in synth_wavs([n] * B, 1)]
    S, D = cfg.num_frames(n), cfg.conv_layers[0][0]
    forms = [("default", {}), ("default_again", {}), ("melspec_gemm", {b"melspec_fft": 0}), ("conv_n128", {b"conv2d_n64": 0})]
    encs = []
    for _, keys in forms:
        enc = HipEncoder(cfg, weights, check="off")
        for k, v in keys.items():
            _lib.check(_lib.load().s3enc_set_handle_tuning(enc._h, k, v), "s3enc_set_handle_tuning")
        encs.append(enc)
    outs = [torch.empty((1, B, S, D), device=dev) for _ in encs]
    entries = [(name, lambda i=i: encs[i].forward(wavs, out=outs[i])) for i, (name, _) in enumerate(forms)]
    if not args.no_torch:
        fwd = torch_model(cfg, weights, dev)
        entries.append(("torch_modules", lambda: fwd(wavs)))
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
    rel = lambda a, b: float((a.double() - b.double()).norm() / b.double().norm())  # noqa: E731
    res = dict(config=args.config, batch=B, secs=args.secs, segments=B * S, steps=args.steps, warmup=args.warmup,
               same_bits_both_default_handles=bool((outs[0] == outs[1]).all()), same_bits_n128=bool((outs[0] == outs[3]).all()),
               gemm_form_rel_diff=rel(outs[2], outs[0]),
               entries=[dict(name=name, ms_median=round(statistics.median(m), 3), ms_min=round(min(m), 3), ms_max=round(max(m), 3),
                             ms_all=[round(v, 3) for v in m]) for (name, _), m in zip(entries, ms)])
    res["same_form_spread_ms"] = round(abs(res["entries"][0]["ms_median"] - res["entries"][1]["ms_median"]), 3)
    if not args.no_torch:
        res["torch_rel_diff"] = rel(fwd(wavs), outs[0][0])

    prof_steps = 5
    res["kernels"] = {}
    for idx in (0, 2, 3):
        enc = encs[idx]
        enc.profile_reset()
        enc.profile_enable(1)
        for _ in range(prof_steps):
            enc.forward(wavs, out=outs[idx])
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
        res["kernels"][forms[idx][0]] = kernels
    if not args.no_torch:
        times = {}
        for _ in range(prof_steps):
            fwd(wavs, times)
        torch.cuda.synchronize()
        res["torch_parts_ms"] = {k: round(statistics.median(a.elapsed_time(b) for a, b in v), 4) for k, v in times.items()}
        res["torch_modules_over_our_forward"] = round(res["entries"][-1]["ms_median"] / res["entries"][0]["ms_median"], 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
