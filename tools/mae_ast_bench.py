#!/usr/bin/env python3
"""MAE-AST on one MI355X: the time of a forward with the fused and the two-step patch embedding, per-kernel times, the patch kernel
against its two bounds, the front end's share, and a plain fp32 torch restatement for scale.

    python tools/mae_ast_bench.py [--configs mae_ast_patch,mae_ast_frame] [--batch 32] [--secs 10] [--steps 20] [--warmup 3]
                                  [--no-torch] [--out profiles/mae_ast_fp32.md]

Prints one JSON object and writes the same figures as a markdown report to ``--out``.  Per configuration:
* the median / min / max of ``--steps`` forwards of THREE handles of the same weights — two with the default tuning (their
  difference is the run-to-run spread a comparison has to exceed) and one with ``patch_embed_fused = 0`` (gather + tile GEMM +
  position add) — and of the same model as torch-ROCm ops in fp32 (a kaldi fbank restated with ``torch.fft.rfft`` included),
  measured ALTERNATING: one forward of every entry per round, HIP events around each, after ``--warmup`` untimed rounds;
* per-kernel times of separate profiled forwards (``s3enc_profile_*``) of the fused and the two-step handle;
* the patch kernel's ``2 M K N`` FLOPs and algorithmic bytes (the image rows it reads, the weights, the position rows, the tokens it
  writes) over its time, against ``--peak-tflops`` (155: the fp32-MFMA peak, DESIGN §4's roofline denominator) and ``--hbm-tbs``
  (8.0 TB/s): the larger of the two times is its bound;
* the per-utterance fbank launches' share of the forward.
The position tables are cut to 1024 rows (``max_token_length``): a 10 s batch needs 496 / 499 of them.
``bench.py`` stays the benchmark of the flagship workload; this tool measures the MAE-AST family only."""

import argparse
import dataclasses
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def torch_model(cfg, weights, dev):
    """the reference's forward as torch's own ops on the GPU, fp32, equal-length batches: kaldi fbank (frames, DC removal,
    pre-emphasis, povey window, rfft, mel, log) -> BatchNorm x 0.5 -> unfold -> Linear + position rows -> Transformer layers"""
    import numpy as np
    import torch

    from oracle import fbank_oracle as F

    nn = torch.nn
    t = lambda name: torch.from_numpy(np.ascontiguousarray(weights[name])).to(dev)
    size, shift, padded = F.frame_params(25.0, 10.0)
    window = torch.from_numpy(F.povey_window(size).astype(np.float32)).to(dev)
    banks = torch.from_numpy(F.mel_banks(128, padded, F.SAMPLE_RATE).astype(np.float32)).to(dev)
    kt, kc, D, H = cfg.ma_kt, cfg.ma_kc, cfg.encoder_embed_dim, cfg.encoder_attention_heads
    mean, var = float(weights["batch_norm.running_mean"].reshape(-1)[0]), float(weights["batch_norm.running_var"].reshape(-1)[0])
    unfold = nn.Unfold(kernel_size=(kt, kc), stride=(kt, kc))
    pe = t("enc_sine_pos_embed.pe").reshape(-1, D)
    eps = torch.finfo(torch.float).eps

    layers = []
    for l in range(cfg.encoder_layers):
        p = f"encoder.layers.{l}"
        layers.append({k: t(f"{p}.{k}") for k in ("self_attn.q_proj.weight", "self_attn.q_proj.bias", "self_attn.k_proj.weight",
                                                 "self_attn.k_proj.bias", "self_attn.v_proj.weight", "self_attn.v_proj.bias",
                                                 "self_attn.out_proj.weight", "self_attn.out_proj.bias", "self_attn_layer_norm.weight",
                                                 "self_attn_layer_norm.bias", "fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias",
                                                 "final_layer_norm.weight", "final_layer_norm.bias")})
    pw, pb = t("post_extract_proj.weight"), t("post_extract_proj.bias")
    eg, eb = t("encoder.layer_norm.weight"), t("encoder.layer_norm.bias")
    lin, lnf = torch.nn.functional.linear, torch.nn.functional.layer_norm

    def attn(x, L):
        B, T, _ = x.shape
        q = lin(x, L["self_attn.q_proj.weight"], L["self_attn.q_proj.bias"]).view(B, T, H, 64).transpose(1, 2)
        k = lin(x, L["self_attn.k_proj.weight"], L["self_attn.k_proj.bias"]).view(B, T, H, 64).transpose(1, 2)
        v = lin(x, L["self_attn.v_proj.weight"], L["self_attn.v_proj.bias"]).view(B, T, H, 64).transpose(1, 2)
        o = torch.nn.functional.scaled_dot_product_attention(q, k, v).transpose(1, 2).reshape(B, T, D)
        return lin(o, L["self_attn.out_proj.weight"], L["self_attn.out_proj.bias"])

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
            def front():
                w = torch.stack(wavs)
                fr = w.unfold(1, size, shift)
                fr = fr - fr.mean(dim=2, keepdim=True)
                fr = fr - 0.97 * torch.cat([fr[:, :, :1], fr[:, :, :-1]], dim=2)
                spec = torch.fft.rfft(fr * window, n=padded, dim=2)
                return torch.log(torch.clamp((spec.real ** 2 + spec.imag ** 2) @ banks.T, min=eps))

            feats = timed("fbank", front)

            def embed():
                x = (feats - mean) / (var + cfg.ma_bn_eps) ** 0.5 * 0.5
                tok = lin(unfold(x.unsqueeze(1)).transpose(-1, -2), pw, pb)
                return tok + pe[:tok.shape[1]]

            x = timed("embed", embed)

            def encoder():
                h, out = x, []
                if not cfg.layer_norm_first:
                    h = lnf(h, (D,), eg, eb)
                for L in layers:
                    g1, b1, g2, b2 = (L["self_attn_layer_norm.weight"], L["self_attn_layer_norm.bias"], L["final_layer_norm.weight"],
                                      L["final_layer_norm.bias"])
                    ffn = lambda y: lin(torch.nn.functional.gelu(lin(y, L["fc1.weight"], L["fc1.bias"])), L["fc2.weight"], L["fc2.bias"])
                    if cfg.layer_norm_first:
                        h = h + attn(lnf(h, (D,), g1, b1), L)
                        h = h + ffn(lnf(h, (D,), g2, b2))
                    else:
                        h = lnf(h + attn(h, L), (D,), g1, b1)
                        h = lnf(h + ffn(h), (D,), g2, b2)
                    out.append(h)
                return torch.stack(out)

            return timed("encoder", encoder)

    return forward


def measure(name, args, torch, dev):
    from s3prl_amd import _lib
    from s3prl_amd.ckpt import mae_ast_hot_path
    from s3prl_amd.encoder import HipEncoder
    from s3prl_amd.synth import named_config, synth_wavs, synth_weights

    cfg = dataclasses.replace(named_config(name), ma_max_token_length=1024)
    weights = mae_ast_hot_path("synthetic weights", cfg, synth_weights(cfg, 0))
    n = int(args.secs * 16000)
    B = args.batch
    wavs = [torch.from_numpy(w).to(dev) for w in synth_wavs([n] * B, 1)]
    Tt, V, D, K = cfg.num_frames(n), cfg.ma_tokens_per_step, cfg.encoder_embed_dim, cfg.ma_kt * cfg.ma_kc
    NL = cfg.encoder_layers
    forms = [("fused", {}), ("fused_again", {}), ("two_step", {b"patch_embed_fused": 0})]
    encs = []
    for _, keys in forms:
        enc = HipEncoder(cfg, weights, check="off")
        for k, v in keys.items():
            _lib.check(_lib.load().s3enc_set_handle_tuning(enc._h, k, v), "s3enc_set_handle_tuning")
        encs.append(enc)
    outs = [torch.empty((NL, B, Tt, V * D), device=dev) for _ in encs]
    entries = [(nm, lambda i=i: encs[i].forward(wavs, out=outs[i])) for i, (nm, _) in enumerate(forms)]
    if not args.no_torch:
        fwd = torch_model(cfg, weights, dev)
        entries.append(("torch_ops_fp32", lambda: fwd(wavs)))
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
    M = B * Tt * V
    res = dict(config=name, kt=cfg.ma_kt, kc=cfg.ma_kc, batch=B, secs=args.secs, tokens=M, steps=args.steps, warmup=args.warmup,
               same_bits_both_fused_handles=bool((outs[0] == outs[1]).all()), two_step_rel_diff=rel(outs[2], outs[0]),
               entries=[dict(name=nm, ms_median=round(statistics.median(m), 3), ms_min=round(min(m), 3), ms_max=round(max(m), 3))
                        for (nm, _), m in zip(entries, ms)])
    res["same_form_spread_ms"] = round(abs(res["entries"][0]["ms_median"] - res["entries"][1]["ms_median"]), 3)
    if not args.no_torch:
        res["torch_rel_diff"] = rel(fwd(wavs).reshape(NL, B, Tt, V * D), outs[0])
        res["torch_over_our_forward"] = round(res["entries"][-1]["ms_median"] / res["entries"][0]["ms_median"], 3)
    prof_steps = 5
    res["kernels"] = {}
    for idx in (0, 2):
        enc = encs[idx]
        enc.profile_reset()
        enc.profile_enable(1)
        for _ in range(prof_steps):
            enc.forward(wavs, out=outs[idx])
        kernels = {}
        for e in enc.profile_read():
            k = dict(ms_per_step=round(e["ms"] / prof_steps, 4), launches_per_step=e["launches"] // prof_steps)
            if e.get("flops") and e["ms"] > 0:
                k["gflop_per_step"] = round(e["flops"] / prof_steps / 1e9, 2)
                k["tflops"] = round(e["flops"] / (e["ms"] * 1e-3) / 1e12, 1)
            kernels[e["name"]] = k
        enc.profile_enable(0)
        res["kernels"][forms[idx][0]] = kernels
    fused = res["kernels"]["fused"]
    total = sum(k["ms_per_step"] for k in fused.values())
    res["kernel_sum_ms"] = round(total, 3)
    res["fbank_share_of_kernel_time"] = round(fused["mae_fbank"]["ms_per_step"] / total, 3)
    pk = fused["patch_embed"]
    flops = 2.0 * M * K * D
    nbytes = 4.0 * (B * Tt * cfg.ma_kt * 128 + D * K + min(Tt * V, 1024) * D + M * D)
    t_mfma, t_hbm, t = flops / (args.peak_tflops * 1e12) * 1e3, nbytes / (args.hbm_tbs * 1e12) * 1e3, pk["ms_per_step"]
    res["patch_kernel"] = dict(ms=t, gflop=round(flops / 1e9, 3), mbytes=round(nbytes / 1e6, 2), tflops=round(flops / (t * 1e-3) / 1e12, 1),
                               tb_per_s=round(nbytes / (t * 1e-3) / 1e12, 3), ms_at_mfma_peak=round(t_mfma, 4), ms_at_hbm_peak=round(t_hbm, 4),
                               bound="fp32 MFMA" if t_mfma >= t_hbm else "HBM", share_of_bound=round(max(t_mfma, t_hbm) / t, 3),
                               two_step_ms=res["kernels"]["two_step"]["patch_embed_two_step"]["ms_per_step"])
    if not args.no_torch:
        times = {}
        for _ in range(prof_steps):
            fwd(wavs, times)
        torch.cuda.synchronize()
        res["torch_parts_ms"] = {k: round(statistics.median(a.elapsed_time(b) for a, b in v), 4) for k, v in times.items()}
    for enc in encs:
        enc.close()
    return res


def report(results, args):
    out = ["# MAE-AST, exact fp32, one MI355X", "",
           f"`python tools/mae_ast_bench.py --batch {args.batch} --secs {args.secs:g} --steps {args.steps} --warmup {args.warmup}`: "
           f"{args.batch} x {args.secs:g} s, synthetic weights, forwards of every entry alternating, HIP events, medians.", ""]
    for r in results:
        out += [f"## {r['config']} (kt = {r['kt']}, kc = {r['kc']}; {r['tokens']} tokens)", "", "| entry | median ms | min | max |", "|---|---|---|---|"]
        out += [f"| {e['name']} | {e['ms_median']} | {e['ms_min']} | {e['ms_max']} |" for e in r["entries"]]
        out += ["", f"Two handles of the same form differ by {r['same_form_spread_ms']} ms (the spread a comparison has to exceed); their bits are "
                f"{'equal' if r['same_bits_both_fused_handles'] else 'NOT equal'}.  Two-step form vs fused, whole states: {r['two_step_rel_diff']:.2e}."]
        if "torch_rel_diff" in r:
            out += [f"torch-ROCm fp32 ops (a stated baseline, not a target): {r['torch_over_our_forward']} x our forward; states differ by "
                    f"{r['torch_rel_diff']:.2e}; parts {r['torch_parts_ms']} ms."]
        p = r["patch_kernel"]
        out += ["", f"Patch kernel: {p['ms']} ms for {p['gflop']} GFLOP and {p['mbytes']} MB: {p['tflops']} TFLOP/s, {p['tb_per_s']} TB/s.  At the "
                f"fp32-MFMA peak ({args.peak_tflops:g} TFLOP/s) it would take {p['ms_at_mfma_peak']} ms, at {args.hbm_tbs:g} TB/s {p['ms_at_hbm_peak']} ms: "
                f"bound by {p['bound']}, at {p['share_of_bound']} of that bound.  The two-step form (gather + GEMM + position add) takes "
                f"{p['two_step_ms']} ms.", "",
                f"Per-utterance fbank launches: {r['fbank_share_of_kernel_time']} of the forward's kernel time ({r['kernel_sum_ms']} ms).", "",
                "| kernel (fused handle) | ms / forward | launches | GFLOP | TFLOP/s |", "|---|---|---|---|---|"]
        out += [f"| {k} | {v['ms_per_step']} | {v['launches_per_step']} | {v.get('gflop_per_step', '')} | {v.get('tflops', '')} |"
                for k, v in r["kernels"]["fused"].items()]
        out.append("")
    return "\n".join(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="mae_ast_patch,mae_ast_frame")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--secs", type=float, default=10.0)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--peak-tflops", type=float, default=155.0)
    ap.add_argument("--hbm-tbs", type=float, default=8.0)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mae_ast_fp32.md"))
    args = ap.parse_args()
    if args.steps < 20:
        ap.error("--steps must be at least 20 (the median of fewer forwards is not a measurement)")

    import torch

    if not torch.cuda.is_available():
        raise SystemExit("mae_ast_bench needs the MI355X: there is no CPU fallback and no CPU timing")
    dev = torch.device("cuda", 0)
    results = [measure(name, args, torch, dev) for name in args.configs.split(",")]
    with open(args.out, "w") as f:
        f.write(report(results, args))
    print(json.dumps(results))


if __name__ == "__main__":
    main()
