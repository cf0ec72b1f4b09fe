#!/usr/bin/env python3
"""SSAST on one MI355X: the time of a forward from the waveforms with the fused and the two-step strided patch embedding, per-kernel
times (front end, embedding in both forms, emit), HuBERT-base fp32 from the same session with the average shader clock, and a plain
fp32 torch restatement for scale.

    python tools/ssast_bench.py [--configs ssast_patch_base,ssast_frame_base] [--windows 1,10] [--batch 32] [--secs 10] [--steps 20]
                                [--warmup 3] [--no-torch] [--out profiles/ssast_fp32.md]

Prints one JSON object and writes the same figures as a markdown report to ``--out``.  Per (configuration, window_secs):
* the median / min / max of ``--steps`` forwards of THREE handles of the same weights — two with the default tuning (their difference
  is the run-to-run spread a comparison has to exceed) and one with ``patch_strided_fused = 0`` (gather + tile GEMM + position add) —
  and of the same model as torch-ROCm ops in fp32 (windows, a kaldi fbank restated with ``torch.fft.rfft``, ``conv2d``, the blocks with
  ``scaled_dot_product_attention``), measured ALTERNATING: one forward of every entry per round, HIP events around each, after
  ``--warmup`` untimed rounds;
* per-kernel times of separate profiled forwards (``s3enc_profile_*``) of the fused and the two-step handle.
Then HuBERT-base fp32 at the same batch, with the average shader clock over its timed region (``s3enc_debug_clock_sample``).
``bench.py`` stays the benchmark of the flagship workload; this tool measures the SSAST family only."""

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def torch_model(cfg, weights, dev):
    """the reference's forward as torch's own ops on the GPU, fp32, equal-length batches"""
    import numpy as np
    import torch

    import ssast_ref as R
    from oracle import fbank_oracle as F

    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
    window = t(R.hanning(400))
    banks = t(F.mel_banks(128, 512, 16000.0))
    D, H = cfg.encoder_embed_dim, cfg.encoder_attention_heads
    W, TL, f_dim, t_dim = cfg.ss_window_samples, cfg.ss_target_length, cfg.ss_f_dim, cfg.ss_t_dim
    cw = t(weights["module.v.patch_embed.proj.weight"].sum(1, keepdims=True))
    cb = t(weights["module.v.patch_embed.proj.bias"])
    pos = t(R.position_rows(cfg, weights))
    pre = t(np.concatenate([weights["module.v.cls_token"][0], weights["module.v.dist_token"][0]]))
    blocks = [{k: t(weights[f"module.v.blocks.{l}.{k}"]) for k in ("norm1.weight", "norm1.bias", "attn.qkv.weight", "attn.qkv.bias",
                                                                   "attn.proj.weight", "attn.proj.bias", "norm2.weight", "norm2.bias",
                                                                   "mlp.fc1.weight", "mlp.fc1.bias", "mlp.fc2.weight", "mlp.fc2.bias")}
              for l in range(cfg.encoder_layers)]
    lin, lnf = torch.nn.functional.linear, torch.nn.functional.layer_norm
    eps = torch.finfo(torch.float).eps

    def forward(wavs):
        with torch.no_grad():
            n = wavs[0].numel()
            nseg = -(-n // W)
            x = torch.zeros((len(wavs), nseg * W), device=dev)
            x[:, :n] = torch.stack(wavs)
            fr = x.reshape(-1, W).unfold(1, 400, 160)
            fr = fr - fr.mean(dim=2, keepdim=True)
            fr = fr - 0.97 * torch.cat([fr[:, :, :1], fr[:, :, :-1]], dim=2)
            spec = torch.fft.rfft(fr * window, n=512, dim=2)
            y = (torch.log(torch.clamp((spec.real ** 2 + spec.imag ** 2) @ banks.T, min=eps)) + 4.2677393) / (4.5689974 * 2)
            img = torch.zeros((y.shape[0], TL, 128), device=dev)
            img[:, :y.shape[1]] = y
            tok = torch.nn.functional.conv2d(img.transpose(1, 2).unsqueeze(1), cw, cb, stride=(cfg.ss_fstride, cfg.ss_tstride))
            h = torch.cat([pre.expand(tok.shape[0], -1, -1), tok.flatten(2).transpose(1, 2)], dim=1) + pos
            out = []
            for L in blocks:
                B, T, _ = h.shape
                q, k, v = lin(lnf(h, (D,), L["norm1.weight"], L["norm1.bias"], 1e-6), L["attn.qkv.weight"],
                              L["attn.qkv.bias"]).view(B, T, 3, H, 64).permute(2, 0, 3, 1, 4)
                o = torch.nn.functional.scaled_dot_product_attention(q, k, v).transpose(1, 2).reshape(B, T, D)
                h = h + lin(o, L["attn.proj.weight"], L["attn.proj.bias"])
                g = lin(lnf(h, (D,), L["norm2.weight"], L["norm2.bias"], 1e-6), L["mlp.fc1.weight"], L["mlp.fc1.bias"])
                h = h + lin(torch.nn.functional.gelu(g), L["mlp.fc2.weight"], L["mlp.fc2.bias"])
                s = h[:, 2:].reshape(len(wavs), nseg, f_dim, t_dim, D).transpose(2, 3).reshape(len(wavs), nseg * t_dim, f_dim * D)
                out.append(s[:, :cfg.num_frames(n)])
            return torch.stack(out)

    return forward


def timed_rounds(entries, args, torch):
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
    return [dict(name=nm, ms_median=round(statistics.median(m), 3), ms_min=round(min(m), 3), ms_max=round(max(m), 3))
            for (nm, _), m in zip(entries, ms)]


def profiled(enc, run, steps=5):
    enc.profile_reset()
    enc.profile_enable(1)
    for _ in range(steps):
        run()
    kernels = {}
    for e in enc.profile_read():
        k = dict(ms_per_step=round(e["ms"] / steps, 4), launches_per_step=e["launches"] // steps)
        if e.get("flops") and e["ms"] > 0:
            k["tflops"] = round(e["flops"] / (e["ms"] * 1e-3) / 1e12, 1)
        kernels[e["name"]] = k
    enc.profile_enable(0)
    return kernels


def measure(name, secs_w, args, torch, dev):
    import dataclasses

    from s3prl_amd import _lib
    from s3prl_amd.ckpt import ssast_hot_path
    from s3prl_amd.encoder import HipEncoder
    from s3prl_amd.synth import named_config, synth_wavs, synth_weights

    cfg = dataclasses.replace(named_config(name), ss_window_secs=float(secs_w))
    cfg.validate()
    released = synth_weights(cfg, 0)
    weights = ssast_hot_path("synthetic weights", cfg, released)
    n = int(args.secs * 16000)
    B, NL = args.batch, cfg.encoder_layers
    wavs = [torch.from_numpy(w).to(dev) for w in synth_wavs([n] * B, 1)]
    T, width = cfg.num_frames(n), cfg.ss_f_dim * cfg.encoder_embed_dim
    forms = [("fused", {}), ("fused_again", {}), ("two_step", {b"patch_strided_fused": 0})]
    encs = []
    for _, keys in forms:
        enc = HipEncoder(cfg, weights, check="off")
        for k, v in keys.items():
            _lib.check(_lib.load().s3enc_set_handle_tuning(enc._h, k, v), "s3enc_set_handle_tuning")
        encs.append(enc)
    outs = [torch.empty((NL, B, T, width), device=dev) for _ in encs]
    entries = [(nm, lambda i=i: encs[i].forward(wavs, out=outs[i])) for i, (nm, _) in enumerate(forms)]
    if not args.no_torch:
        fwd = torch_model(cfg, released, dev)
        entries.append(("torch_ops_fp32", lambda: fwd(wavs)))
    rel = lambda a, b: float((a.double() - b.double()).norm() / b.double().norm())  # noqa: E731
    res = dict(config=name, window_secs=secs_w, batch=B, secs=args.secs, windows=B * cfg.ss_num_windows(n),
               tokens_per_window=2 + cfg.ss_f_dim * cfg.ss_t_dim, rows=T, steps=args.steps, warmup=args.warmup,
               entries=timed_rounds(entries, args, torch))
    res["same_bits_both_fused_handles"] = bool((outs[0] == outs[1]).all())
    res["two_step_rel_diff"] = rel(outs[2], outs[0])
    res["same_form_spread_ms"] = round(abs(res["entries"][0]["ms_median"] - res["entries"][1]["ms_median"]), 3)
    if not args.no_torch:
        res["torch_rel_diff"] = rel(fwd(wavs), outs[0])
        res["torch_over_our_forward"] = round(res["entries"][-1]["ms_median"] / res["entries"][0]["ms_median"], 3)
    res["kernels"] = {forms[i][0]: profiled(encs[i], lambda i=i: encs[i].forward(wavs, out=outs[i])) for i in (0, 2)}
    for enc in encs:
        enc.close()
    return res


def hubert_line(args, torch, dev):
    from s3prl_amd import _lib
    from s3prl_amd.encoder import HipEncoder
    from s3prl_amd.synth import named_config, synth_wavs, synth_weights

    lib = _lib.load()
    cfg = named_config("hubert_base")
    enc = HipEncoder(cfg, synth_weights(cfg, 0), check="off")
    n = int(args.secs * 16000)
    wavs = [torch.from_numpy(w).to(dev) for w in synth_wavs([n] * args.batch, 1)]
    out = torch.empty((cfg.num_hidden_states, args.batch, cfg.num_frames(n), cfg.encoder_embed_dim), device=dev)
    clk = torch.zeros((2, 3), dtype=torch.int64, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    for _ in range(args.warmup):
        enc.forward(wavs, out=out)
    _lib.check(lib.s3enc_debug_clock_sample(clk[0].data_ptr(), stream))
    entry = timed_rounds([("hubert_base_fp32", lambda: enc.forward(wavs, out=out))], dataclass_like(args, warmup=0), torch)[0]
    _lib.check(lib.s3enc_debug_clock_sample(clk[1].data_ptr(), stream))
    torch.cuda.synchronize()
    a, b = clk[0].cpu().tolist(), clk[1].cpu().tolist()
    entry["clock_ghz"] = round((b[0] - a[0]) / (b[1] - a[1]) * a[2] * 1e-6, 3) if b[1] != a[1] else None
    enc.close()
    return entry


def dataclass_like(args, **kw):
    ns = argparse.Namespace(**vars(args))
    for k, v in kw.items():
        setattr(ns, k, v)
    return ns


def report(results, hubert, args):
    out = ["# SSAST, exact fp32, one MI355X", "",
           f"`python tools/ssast_bench.py --batch {args.batch} --secs {args.secs:g} --steps {args.steps} --warmup {args.warmup}`: "
           f"{args.batch} x {args.secs:g} s from the waveforms, synthetic weights in the released key layout, forwards of every entry "
           "alternating, HIP events, medians.", ""]
    if hubert:
        out += [f"HuBERT-base fp32 in the same session: {hubert['ms_median']} ms (min {hubert['ms_min']}, max {hubert['ms_max']}) at an average "
                f"shader clock of {hubert['clock_ghz']} GHz.", ""]
    for r in results:
        out += [f"## {r['config']}, window_secs = {r['window_secs']:g} ({r['windows']} windows of {r['tokens_per_window']} tokens, {r['rows']} state rows)",
                "", "| entry | median ms | min | max |", "|---|---|---|---|"]
        out += [f"| {e['name']} | {e['ms_median']} | {e['ms_min']} | {e['ms_max']} |" for e in r["entries"]]
        out += ["", f"Two handles of the same form differ by {r['same_form_spread_ms']} ms (the spread a comparison has to exceed); their bits are "
                f"{'equal' if r['same_bits_both_fused_handles'] else 'NOT equal'}.  Two-step form vs fused, whole states: {r['two_step_rel_diff']:.2e}."]
        if "torch_rel_diff" in r:
            out += [f"torch-ROCm fp32 ops (a stated baseline, not a target): {r['torch_over_our_forward']} x our forward; states differ by "
                    f"{r['torch_rel_diff']:.2e}."]
        for form in ("fused", "two_step"):
            out += ["", f"| kernel ({form} handle) | ms / forward | launches | TFLOP/s |", "|---|---|---|---|"]
            out += [f"| {k} | {v['ms_per_step']} | {v['launches_per_step']} | {v.get('tflops', '')} |" for k, v in r["kernels"][form].items()]
        out.append("")
    return "\n".join(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="ssast_patch_base,ssast_frame_base")
    ap.add_argument("--windows", default="1,10")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--secs", type=float, default=10.0)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--no-hubert", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ssast_fp32.md"))
    args = ap.parse_args()
    if args.steps < 20:
        ap.error("--steps must be at least 20 (the median of fewer forwards is not a measurement)")

    import torch

    if not torch.cuda.is_available():
        raise SystemExit("ssast_bench needs the MI355X: there is no CPU fallback and no CPU timing")
    dev = torch.device("cuda", 0)
    hubert = None if args.no_hubert else hubert_line(args, torch, dev)
    results = [measure(name, float(w), args, torch, dev) for name in args.configs.split(",") for w in args.windows.split(",")]
    with open(args.out, "w") as f:
        f.write(report(results, hubert, args))
    print(json.dumps(dict(hubert_base_fp32=hubert, results=results)))


if __name__ == "__main__":
    main()
