#!/usr/bin/env python3
"""The plain signal features (`spectrogram`, `mfcc`, `mel`, `linear`, `stft_mag` with and without log) on one MI355X in exact fp32:
the time of a forward of 32 x 10 s per name, the per-kernel split, the achieved bandwidth of the HBM-bound kernels against the
bytes they must move, and torch-ROCm eager on the same inputs where torch alone can compute the feature (`stft_mag`, `linear`).

    python tools/spectral_bench.py [--batch 32] [--secs 10] [--steps 20] [--warmup 3] [--bands-log LOG] [--out profiles/spectral_upstreams_fp32.md]

Every contender runs once per round, ALTERNATING, HIP events around each, after ``--warmup`` untimed rounds; the median of
``--steps`` rounds is reported, next to the average shader clock over the timed region (``s3enc_debug_clock_sample``, as ``bench.py``
prints it).  The per-kernel times come from ``torch.profiler`` over three further forwards per name.  ``--bands-log``: the output
of ``pytest -s tests/test_spectral_gpu.py tests/test_fuzz_spectral_gpu.py``; the worst ``SPECTRAL_BAND`` figure of every band goes
into the report.  Prints one JSON object and writes the markdown report.  ``bench.py`` stays the benchmark of the flagship workload."""

import argparse
import collections
import json
import os
import re
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def eager_stft_mag(torch, wavs, log):
    """|torch.stft(512 / 320 / 512, periodic hann, centred, reflect)| per utterance, (T, 257), zero-padded: torch alone."""
    window = torch.hann_window(512, device=wavs[0].device)
    feats = []
    for w in wavs:
        x = torch.stft(w, n_fft=512, hop_length=320, win_length=512, window=window, center=True, pad_mode="reflect", normalized=False,
                       return_complex=True).abs().transpose(0, 1)
        feats.append(torch.log(torch.clamp(x, min=1e-8)) if log else x)
    return torch.nn.utils.rnn.pad_sequence(feats, batch_first=True)


def eager_linear(torch, wavs):
    """log(|STFT|^2 + 1e-10) of the zero-padded batch (400 / 160, periodic hann, centred), the CMVN over the frames up to each
    utterance's last non-zero sample, the rows the length ratio keeps: torch alone."""
    lengths = [len(w) for w in wavs]
    batch = torch.nn.utils.rnn.pad_sequence(wavs, batch_first=True)
    trimmed = []
    for row in batch:
        nz = row.nonzero()
        trimmed.append(batch.size(-1) if len(nz) == 0 else nz[:, -1].max().item() + 1)
    spec = torch.stft(batch, n_fft=400, hop_length=160, win_length=400, window=torch.hann_window(400, device=batch.device), center=True,
                      pad_mode="reflect", normalized=False, onesided=True, return_complex=True)
    feats = (spec.abs().pow(2) + 1e-10).log()
    rate = batch.size(-1) / feats.size(-1)
    rows = []
    for f, n in zip(feats, trimmed):
        f = f[:, :round(n / rate)]
        rows.append(((f - f.mean(dim=-1, keepdim=True)) / (f.std(dim=-1, keepdim=True) + 1e-10)).transpose(0, 1))
    feats = torch.nn.utils.rnn.pad_sequence(rows, batch_first=True)
    ratio = feats.size(1) / lengths[0]
    return torch.nn.utils.rnn.pad_sequence([f[:round(n * ratio)] for f, n in zip(feats, lengths)], batch_first=True)


def worst_bands(path):
    """SPECTRAL_BAND lines -> {band: worst figure}."""
    worst = collections.defaultdict(float)
    pats = [("linear domain, share of the band", r"linear ([0-9.e+-]+) of its band"), ("log domain, share of the band", r"log ([0-9.e+-]+) of its band"),
            ("fraction of bins left out", r"left out ([0-9.e+-]+)"), ("spectrogram energy, share of the band", r"energy ([0-9.e+-]+) of its band"),
            ("CMVN against the float64 CMVN of the device's features, absolute", r"cmvn ([0-9.e+-]+)"),
            ("mfcc whole path, absolute", r"whole path ([0-9.e+-]+)"), ("against the reference's output, relative norm", r"against the reference ([0-9.e+-]+)"),
            ("mfcc / fuzz coefficients, share of the band", r"mfcc[^:]*: ([0-9.e+-]+) of its band")]
    with open(path) as f:
        for line in f:
            if "SPECTRAL_BAND" not in line:
                continue
            for name, pat in pats:
                m = re.search(pat, line)
                if m:
                    worst[name] = max(worst[name], float(m.group(1)))
            m = re.search(r"c, delta, delta-delta ([0-9.e+-]+) ([0-9.e+-]+) ([0-9.e+-]+) of their band", line)
            if m:
                for k, v in zip(("mfcc c", "mfcc delta", "mfcc delta-delta"), m.groups()):
                    worst[k + ", share of the band"] = max(worst[k + ", share of the band"], float(v))
    return dict(worst)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--secs", type=float, default=10.0)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--bands-log", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spectral_upstreams_fp32.md"))
    args = ap.parse_args()

    import torch

    import s3prl_amd.hub as hub
    from s3prl_amd import _lib
    from s3prl_amd.synth import synth_wavs
    from s3prl_amd.upstream.log_stft.hubconf import LOG_STFT_MAG, STFT_MAG

    assert torch.cuda.is_available(), "needs the MI355X"
    dev = torch.device("cuda:0")
    B, n = args.batch, int(args.secs * 16000)
    wavs = [torch.from_numpy(w).to(dev) for w in synth_wavs([n] * B, 1)]
    experts = {"spectrogram": hub.spectrogram(), "mfcc": hub.mfcc(), "mel": hub.mel(), "linear": hub.linear(),
               "stft_mag": hub.stft_mag(STFT_MAG), "stft_mag_log": hub.stft_mag(LOG_STFT_MAG), "fbank": hub.fbank()}
    runs = {name: (lambda e=e: e(wavs)) for name, e in experts.items()}
    runs["eager stft_mag"] = lambda: eager_stft_mag(torch, wavs, False)
    runs["eager stft_mag_log"] = lambda: eager_stft_mag(torch, wavs, True)
    runs["eager linear"] = lambda: eager_linear(torch, wavs)
    # the eager restatements compute what ours do
    for ours, eager in (("stft_mag", "eager stft_mag"), ("stft_mag_log", "eager stft_mag_log"), ("linear", "eager linear")):
        a, b = runs[ours]()["hidden_states"][0], runs[eager]()
        assert a.shape == b.shape and float((a - b).norm() / b.norm()) < 1e-4, (ours, a.shape, b.shape)

    lib = _lib.load()
    stream = torch.cuda.current_stream(dev).cuda_stream
    clk = torch.zeros((2, 3), dtype=torch.int64, device=dev)

    def one_round(ms=None):
        for name, fn in runs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if ms is not None:
                ms[name].append(a.elapsed_time(b))

    for _ in range(args.warmup):
        one_round()
    torch.cuda.synchronize()
    ms = {name: [] for name in runs}
    _lib.check(lib.s3enc_debug_clock_sample(clk[0].data_ptr(), stream))
    for _ in range(args.steps):
        one_round(ms)
    _lib.check(lib.s3enc_debug_clock_sample(clk[1].data_ptr(), stream))
    torch.cuda.synchronize()
    a, b = clk[0].cpu().tolist(), clk[1].cpu().tolist()
    ghz = (b[0] - a[0]) / (b[1] - a[1]) * a[2] * 1e-6 if b[1] != a[1] else None
    forward = {name: dict(ms_median=round(statistics.median(v), 3), ms_min=round(min(v), 3), ms_max=round(max(v), 3)) for name, v in ms.items()}

    # per kernel: torch.profiler over three forwards of each of ours
    kernels, note = {}, None
    try:
        from torch.profiler import ProfilerActivity, profile

        for name in experts:
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                for _ in range(3):
                    runs[name]()
                torch.cuda.synchronize()
            rows = {}
            for e in prof.key_averages():
                us = getattr(e, "device_time_total", None) or getattr(e, "cuda_time_total", 0)
                if us > 0:
                    rows[e.key[:90]] = dict(ms_per_forward=round(us / 3e3, 4), launches_per_forward=e.count // 3)
            kernels[name] = rows
    except Exception as exc:  # the profiler is an optional extra of the torch build
        note = f"per-kernel times not measured: {type(exc).__name__}: {exc}"

    # the HBM-bound kernels: the bytes they must move per forward of the whole batch
    T_kaldi, T_stft, T_pre = 1 + (n - 400) // 160, 1 + n // 320, 1 + n // 160
    must_move = {
        ("spectrogram", "spectrum_rows"): B * T_kaldi * 257 * 12,        # re | im read once, the bins written once
        ("spectrogram", "frame_energy"): B * (n * 4 + T_kaldi * 4),      # every sample once (the overlap is served by the caches)
        ("stft_mag", "spectrum_rows"): B * T_stft * 257 * 12,
        ("stft_mag_log", "spectrum_rows"): B * T_stft * 257 * 12,
        ("linear", "spectrum_rows"): B * T_pre * 201 * 12,
        ("linear", "last_nonzero"): B * n * 4,
        ("mel", "last_nonzero"): B * n * 4,
    }
    bandwidth = {}
    for (name, key), nbytes in must_move.items():
        hit = [v for k, v in kernels.get(name, {}).items() if key in k]
        if hit:
            t = sum(v["ms_per_forward"] for v in hit)
            bandwidth[f"{name}: {key}"] = dict(mbytes=round(nbytes / 1e6, 2), ms=round(t, 4), gb_per_s=round(nbytes / (t * 1e-3) / 1e9, 1) if t > 0 else None,
                                               launches=sum(v["launches_per_forward"] for v in hit))
    versus = {ours: round(forward[ours]["ms_median"] / forward[eager]["ms_median"], 3)
              for ours, eager in (("stft_mag", "eager stft_mag"), ("stft_mag_log", "eager stft_mag_log"), ("linear", "eager linear"))}
    bands = worst_bands(args.bands_log) if args.bands_log else {}
    result = dict(batch=B, secs=args.secs, steps=args.steps, warmup=args.warmup, clock_ghz=round(ghz, 3) if ghz else None, forward=forward,
                  ours_over_eager=versus, bandwidth=bandwidth, kernels=kernels, bands=bands, note=note)
    print(json.dumps(result))

    lines = ["# The plain signal features in exact fp32 on one MI355X", "",
             f"`tools/spectral_bench.py`: {B} x {args.secs:g} s at 16 kHz, the median of {args.steps} alternating rounds after {args.warmup} "
             f"untimed ones, one session; average shader clock over the timed region {result['clock_ghz']} GHz.", "",
             "## ms per batch", "", "| contender | median | min | max |", "|---|---|---|---|"]
    lines += [f"| {k} | {v['ms_median']} | {v['ms_min']} | {v['ms_max']} |" for k, v in forward.items()]
    lines += ["", "## Against torch-ROCm eager on the same inputs (ours / eager; at most 1 is the condition)", ""]
    for k, v in versus.items():
        lines.append(f"- `{k}`: {v}" + ("" if v <= 1.0 else "  **slower than eager**"))
    lines += ["", "## The HBM-bound kernels: achieved bandwidth against the bytes they must move", "",
              "| kernel | MB | ms | GB/s | launches |", "|---|---|---|---|---|"]
    lines += [f"| {k} | {v['mbytes']} | {v['ms']} | {v['gb_per_s']} | {v['launches']} |" for k, v in bandwidth.items()]
    lines += ["", "## ms per forward and per kernel (torch.profiler, three forwards)", ""]
    if note:
        lines.append(note)
    for name, rows in kernels.items():
        lines += [f"### {name}", "", "| kernel | ms | launches |", "|---|---|---|"]
        lines += [f"| `{k}` | {v['ms_per_forward']} | {v['launches_per_forward']} |" for k, v in sorted(rows.items(), key=lambda kv: -kv[1]["ms_per_forward"])]
        lines.append("")
    if bands:
        lines += ["## The worst observed value of every band (tests/test_spectral_gpu.py, tests/test_fuzz_spectral_gpu.py)", ""]
        lines += [f"- {k}: {v:g}" for k, v in sorted(bands.items())]
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
