#!/usr/bin/env python3
"""BYOL-S on one MI355X: the time of a forward in its forms, per-kernel times with the convolutions' share of the fp32-MFMA roofline
per layer shape, the gate on conv2d.hip's general instantiation, and torch's modules for scale.

    python tools/byol_s_bench.py [--config byol_s_resnetish34] [--batch 32] [--secs 10] [--steps 10] [--warmup 2] [--no-torch]
    python tools/byol_s_bench.py --gate-run OUT.json          # under `rocprofv3 --kernel-trace`: the two conv entries, alternating
    python tools/byol_s_bench.py --gate-parse OUT.json TRACE_DIR

The first form prints one JSON object:
* the median / min / max of ``--steps`` forwards of handles of the same configuration and weights — two with the default tuning
  (their difference is the run-to-run spread a comparison has to exceed), one with the other stem form (``stem_fused``), and one per
  ``--chunks`` value of ``byol_s_chunk`` — and of the same network as torch-ROCm modules in fp32, eager (the front end and the
  statistics as torch ops too), measured ALTERNATING: one forward of every entry per round, HIP events around each, after
  ``--warmup`` untimed rounds;
* per-kernel times of a separate profiled forward of the default handle (``s3enc_profile_*``), with FLOPs counted from the shapes,
  TFLOP/s and, for the MFMA convolutions, the fraction of ``--peak-tflops`` (155: the fp32-MFMA peak, DESIGN §4's roofline
  denominator), one entry per layer shape.
The gate: ``s3enc_op_conv2d_res`` at k = 3, stride 1, no residual (the GEN instantiation) against ``s3enc_op_conv2d3x3_affine`` (the
instantiation every earlier family runs) on VGGish's and BYOL-A's un-pooled layer shapes, the same call alternating; every call is
exactly one dispatch of ``conv2d3x3_kernel``, so ``--gate-parse`` reads the kernels' own durations off the trace in call order.
``bench.py`` stays the benchmark of the flagship workload; this tool measures the BYOL-S family only."""

import argparse
import ctypes as C
import glob
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

# (name, H, W, Cin, Cout, examples): the un-pooled 3 x 3 / stride-1 layers of VGGish (32 x 10 s: 320 examples) and BYOL-A (320 segments)
GATE_SHAPES = [("vggish conv2", 48, 32, 64, 128, 320), ("vggish conv3_1", 24, 16, 128, 256, 320), ("vggish conv3_2", 24, 16, 256, 256, 320),
               ("vggish conv4_1", 12, 8, 256, 512, 320), ("vggish conv4_2", 12, 8, 512, 512, 320),
               ("byol_a conv2", 50, 32, 64, 64, 320), ("byol_a conv3", 25, 16, 64, 64, 320)]
GATE_ROUNDS = 10


def torch_model(cfg, weights, dev):
    """the reference's forward as torch's own ops on the GPU, fp32, eager: windows -> torch.stft -> mel -> log -> batch statistics ->
    the network (nn.Conv2d / nn.BatchNorm2d in eval mode / nn.MaxPool2d)"""
    import numpy as np
    import torch

    import byol_a_ref as RA

    nn = torch.nn
    F = nn.functional
    _, window, step = cfg.conv_layers[0]
    t = lambda k: torch.from_numpy(weights[k]).to(dev)  # noqa: E731

    def bn(name, c):
        m = nn.BatchNorm2d(c)
        m.weight.data, m.bias.data, m.running_mean.data, m.running_var.data = t(name + ".weight"), t(name + ".bias"), t(name + ".running_mean"), t(name + ".running_var")
        return m.to(dev).eval()

    def conv(name, cin, cout, k, stride, bias=False):
        m = nn.Conv2d(cin, cout, k, stride=stride, padding=(k - 1) // 2, bias=bias)
        m.weight.data = t(name + ".weight")
        if bias:
            m.bias.data = t(name + ".bias")
        return m.to(dev).eval()

    if cfg.bs_network == "default":
        feats, cin = [], 1
        for k in (0, 4, 8):
            feats += [conv(f"features.{k}", cin, 64, 3, 1, True), bn(f"features.{k + 1}", 64), nn.ReLU(), nn.MaxPool2d(2, 2)]
            cin = 64
        features = nn.Sequential(*feats)
        fc0, fc3 = nn.Linear(512, 2048), nn.Linear(2048, 2048)
        fc0.weight.data, fc0.bias.data, fc3.weight.data, fc3.bias.data = t("fc.0.weight"), t("fc.0.bias"), t("fc.3.weight"), t("fc.3.bias")
        fc = nn.Sequential(fc0, nn.ReLU(), fc3, nn.ReLU()).to(dev).eval()

        def net(x):
            x = features(x).permute(0, 3, 2, 1)
            n, T, D, Cc = x.shape
            x = fc(x.reshape(n, T, D * Cc))
            return x.mean(1) + x.amax(1)
    else:
        stem = nn.Sequential(conv("conv1", 1, 64, 7, 1), bn("bn1", 64), nn.ReLU(), nn.MaxPool2d(3, 2, 1))
        blocks, cin = [], 64
        for L, nblk in enumerate(cfg.bs_blocks):
            planes = 64 << L
            for b in range(nblk):
                pre, stride = f"layer{L + 1}.{b}", 2 if (L > 0 and b == 0) else 1
                down = None
                if pre + ".downsample.0.weight" in weights:
                    down = nn.Sequential(conv(pre + ".downsample.0", cin, planes, 1, stride), bn(pre + ".downsample.1", planes))
                blocks.append((nn.Sequential(conv(pre + ".conv1", cin, planes, 3, stride), bn(pre + ".bn1", planes), nn.ReLU(),
                                             conv(pre + ".conv2", planes, planes, 3, 1), bn(pre + ".bn2", planes)), down))
                cin = planes

        def net(x):
            x = stem(x)
            for body, down in blocks:
                x = torch.relu(body(x) + (x if down is None else down(x)))
            x = x.permute(0, 3, 2, 1)
            n, T, D, Cc = x.shape
            x = x.reshape(n, T, D * Cc)
            return x.mean(1) + x.amax(1)

    fb = torch.from_numpy(RA.mel_bank(np.float32)).to(dev)
    win = torch.hann_window(400, device=dev)
    eps = torch.finfo(torch.float).eps

    def forward(wavs, chunk=512):
        with torch.no_grad():
            x = torch.nn.utils.rnn.pad_sequence(wavs, batch_first=True)
            x = F.pad(x, (window // 2, window - window // 2))
            frames = x.unfold(1, window, step)  # (B, S, window)
            B, S = frames.shape[:2]
            frames = frames.reshape(B * S, window)
            spec = torch.stft(frames, 1024, 160, 400, window=win, center=True, pad_mode="reflect", return_complex=True).abs().pow(2.0)
            lm = (torch.matmul(spec.transpose(1, 2), fb).transpose(1, 2) + eps).log()  # (N, 64, frames)
            mean, std = lm.mean() / len(lm), lm.std() / len(lm)
            lm = ((lm - mean) / std).unsqueeze(1)
            out = torch.cat([net(lm[i:i + chunk]) for i in range(0, len(lm), chunk)])  # serab.py's BATCH_SIZE-style chunks: bounded memory
            return out.reshape(B, S, -1)

    return forward


def stats_of(ms):
    return dict(median=round(statistics.median(ms), 4), min=round(min(ms), 4), max=round(max(ms), 4))


def forward_bench(args):
    import numpy as np
    import torch

    from s3prl_amd import _lib
    from s3prl_amd.encoder import HipEncoder
    from s3prl_amd.synth import named_config, synth_wavs, synth_weights

    cfg = named_config(args.config)
    weights = synth_weights(cfg, 7)
    n = int(args.secs * 16000)
    wavs = [torch.from_numpy(w).cuda() for w in synth_wavs([n] * args.batch, 11)]
    lib = _lib.load()
    entries = {}

    def handle(name, **tuning):
        enc = HipEncoder(cfg, weights)
        for k, v in tuning.items():
            _lib.check(lib.s3enc_set_handle_tuning(enc._h, k.encode(), v), "s3enc_set_handle_tuning")
        entries[name] = (lambda e=enc: e.forward(wavs), enc)

    handle("default")
    handle("default_again")
    if cfg.bs_network == "resnetish":
        handle("stem_fused", stem_fused=1)
    for ch in args.chunks:
        handle(f"chunk_{ch}", byol_s_chunk=ch)
    if not args.no_torch:
        tm = torch_model(cfg, weights, torch.device("cuda"))
        entries["torch_eager_fp32"] = (lambda: tm(wavs), None)
    times = {k: [] for k in entries}
    for r in range(args.warmup + args.steps):
        for name, (fn, _) in entries.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            out = fn()
            b.record()
            torch.cuda.synchronize()
            if r >= args.warmup:
                times[name].append(a.elapsed_time(b))
    S = cfg.num_frames(n)
    res = dict(config=args.config, batch=args.batch, secs=args.secs, windows=args.batch * S, steps=args.steps,
               forward_ms={k: stats_of(v) for k, v in times.items()})
    base = entries["default"][0]().clone()
    res["bits_equal_across_forms"] = {k: bool(torch.equal(fn(), base)) for k, (fn, e) in entries.items() if e is not None}
    if not args.no_torch:
        tt = entries["torch_eager_fp32"][0]()
        res["torch_vs_ours_rel"] = float((tt - base[0]).norm() / base[0].norm())
    # per-kernel times of one profiled forward of the default handle
    enc = entries["default"][1]
    enc.profile_enable(True)
    enc.profile_reset()
    enc.forward(wavs)
    torch.cuda.synchronize()
    prof = enc.profile_read()
    enc.profile_enable(False)
    total = sum(p["ms"] for p in prof)
    kernels = []
    for p in sorted(prof, key=lambda p: -p["ms"]):
        tf = p["flops"] / (p["ms"] * 1e9) if p["ms"] > 0 else 0.0
        ent = dict(name=p["name"], launches=p["launches"], ms=round(p["ms"], 4), share=round(p["ms"] / total, 4), gflop=round(p["flops"] / 1e9, 2),
                   tflops=round(tf, 2))
        if p["name"].startswith(("conv2d:", "conv2d3x3:L")):
            ent["of_fp32_mfma_peak"] = round(tf / args.peak_tflops, 3)
        kernels.append(ent)
    res["profiled_forward_ms"] = round(total, 3)
    conv = [k for k in kernels if "of_fp32_mfma_peak" in k]
    if conv:
        res["conv_gflop"] = round(sum(k["gflop"] for k in conv), 1)
        res["conv_ms"] = round(sum(k["ms"] for k in conv), 3)
        res["conv_of_fp32_mfma_peak"] = round(sum(k["gflop"] for k in conv) / sum(k["ms"] for k in conv) / args.peak_tflops, 3)
    res["kernels"] = kernels
    for _, e in entries.values():
        if e is not None:
            e.close()
    print(json.dumps(res))


def gate_run(path):
    import numpy as np
    import torch

    from s3prl_amd import _lib

    lib = _lib.load()
    calls = []
    ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    for name, H, W, Cin, N, nb in GATE_SHAPES:
        rng = np.random.default_rng(H + N)
        xb = torch.zeros((nb, H + 2, W + 2, Cin), device="cuda")
        xb[:, 1:H + 1, 1:W + 1] = torch.randn((nb, H, W, Cin), device="cuda")
        w = np.ascontiguousarray(rng.standard_normal((N, Cin, 3, 3)) / np.sqrt(9 * Cin), dtype=np.float32)
        sc, sh = torch.ones(N, device="cuda"), torch.zeros(N, device="cuda")
        outs = [torch.empty((nb, H, W, N), device="cuda") for _ in range(2)]
        for r in range(GATE_ROUNDS + 2):
            _lib.check(lib.s3enc_op_conv2d3x3_affine(ptr(xb), C.c_void_p(w.ctypes.data), None, ptr(sc), ptr(sh), nb, H, W, Cin, N, 1, 0, 0,
                                                     ptr(outs[0]), 0, N, None), "affine")
            calls.append([name, "ext", r])
            _lib.check(lib.s3enc_op_conv2d_res(ptr(xb), C.c_void_p(w.ctypes.data), None, ptr(sc), ptr(sh), None, nb, H, W, Cin, N, 3, 1, 1,
                                               ptr(outs[1]), 0, N, None), "res")
            calls.append([name, "gen", r])
        torch.cuda.synchronize()
        assert torch.equal(outs[0], outs[1]), name
    with open(path, "w") as f:
        json.dump(calls, f)
    print(f"{len(calls)} calls")


def gate_parse(path, trace_dir):
    import csv

    calls = json.load(open(path))
    rows = []
    for f in glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True):
        rows += [r for r in csv.DictReader(open(f)) if "conv2d3x3_kernel" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    assert len(rows) == len(calls), (len(rows), len(calls))
    out = {}
    for (name, form, r), row in zip(calls, rows):
        gen = "Lb1ELb1E" in row["Kernel_Name"] or "true, true" in row["Kernel_Name"]
        assert gen == (form == "gen"), (name, form, row["Kernel_Name"])
        if r >= 2:  # two warm-up rounds
            out.setdefault(name, {}).setdefault(form, []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    res = []
    for name, H, W, Cin, N, nb in GATE_SHAPES:
        ext, gen = out[name]["ext"], out[name]["gen"]
        flop = 2.0 * nb * H * W * N * 9 * Cin
        spread = max(ext) - min(ext)
        res.append(dict(shape=name, H=H, W=W, Cin=Cin, Cout=N, examples=nb, ext_us=stats_of(ext), gen_us=stats_of(gen),
                        ext_spread_us=round(spread, 3), gen_minus_ext_median_us=round(statistics.median(gen) - statistics.median(ext), 3),
                        within_spread=bool(statistics.median(gen) - statistics.median(ext) <= spread),
                        ext_of_peak=round(flop / statistics.median(ext) / 1e6 / 155.0, 3), gen_of_peak=round(flop / statistics.median(gen) / 1e6 / 155.0, 3)))
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="byol_s_resnetish34")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--secs", type=float, default=10.0)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--chunks", type=int, nargs="*", default=[])
    ap.add_argument("--peak-tflops", type=float, default=155.0)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--gate-run")
    ap.add_argument("--gate-parse", nargs=2)
    args = ap.parse_args()
    if args.gate_run:
        gate_run(args.gate_run)
    elif args.gate_parse:
        gate_parse(*args.gate_parse)
    else:
        forward_bench(args)
