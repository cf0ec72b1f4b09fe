#!/usr/bin/env python3
"""DeCoAR on one MI355X: the time of a forward, per-kernel times, and the batch-shared LSTM step beside the per-utterance kernels.

    python tools/decoar_bench.py [--config decoar] [--batch 32] [--secs 10] [--steps 20] [--warmup 3] [--no-family] [--no-ops]

Prints one JSON object:
* ``family``: the median / min / max of ``--steps`` forwards of the released shape (HIP events around each, after ``--warmup``
  untimed ones), the per-kernel times of separate profiled forwards (``s3enc_profile_*``), the milliseconds per LSTM layer (both
  directions) and the recurrent step's microseconds (``rnnb_lstm`` / (layers * T): one launch runs both directions);
* ``ops``: at H = 512 and H = 1024, B = ``--batch``, the microseconds per time step of ``s3enc_op_lstm_bidir`` (both directions per
  launch) and — at H = 512, where they can still run an LSTM — of ``s3enc_op_rnn_len`` in its one-launch (``rnn_split`` 0) and
  step-split (``rnn_split`` 8) forms (ONE direction).  The op entries pack and upload W_hh and synchronise, so a step's time is the
  DIFFERENCE of the medians at two sequence lengths over the difference of the lengths: what does not depend on T cancels.
  ``bidir_us_per_step_and_direction`` (half a launch) is what stands beside the older kernels' figures.
* the derived floors next to them, labelled as derived: the fp32 matrix pipe (2 * 2 * B' * 4 H * H FLOP per step at 157.3 TFLOP/s,
  B' = B rounded up to a 32-wide tile) and the L2 reads of a step — W_hh once, 16 H^2 bytes per direction, and h once per
  workgroup, H / 8 x B' x H x 4 bytes per direction — at 34.5 TB/s.
``bench.py`` stays the benchmark of the flagship workload; this tool measures the DeCoAR family only."""

import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

L2_BYTES_PER_S = 34.5e12   # MI355X: ~34.5 TB/s of aggregate L2 bandwidth
F32_MATRIX_FLOPS = 157.3e12


def timed(fn, steps, warmup):
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


def family(args):
    import torch

    from s3prl_amd.encoder import HipEncoder
    from s3prl_amd.synth import named_config, synth_wavs, synth_weights

    dev = torch.device("cuda", 0)
    cfg = named_config(args.config)
    n, B = int(args.secs * 16000), args.batch
    wavs = [torch.from_numpy(w).to(dev) for w in synth_wavs([n] * B, 1)]
    T, H, NL = cfg.num_frames(n), cfg.decoar_hidden, cfg.decoar_layers
    enc = HipEncoder(cfg, synth_weights(cfg, 0), check="off")
    out = torch.empty((cfg.num_hidden_states, B, T, 2 * H), device=dev)
    ms = timed(lambda: enc.forward(wavs, out=out), args.steps, args.warmup)
    prof_steps = 3
    enc.profile_reset()
    enc.profile_enable(1)
    for _ in range(prof_steps):
        enc.forward(wavs, out=out)
    kernels = {e["name"]: dict(ms_per_forward=round(e["ms"] / prof_steps, 4), launches_per_forward=e["launches"] // prof_steps)
               for e in enc.profile_read()}
    enc.profile_enable(0)
    rnn = kernels["rnnb_lstm"]["ms_per_forward"]
    gin = kernels["gemm:decoar_in"]["ms_per_forward"]
    Bp = -(-B // 32) * 32
    return dict(config=args.config, batch=B, secs=args.secs, frames=T, hidden=H, layers=NL, steps=args.steps, warmup=args.warmup,
                ms_median=round(statistics.median(ms), 3), ms_min=round(min(ms), 3), ms_max=round(max(ms), 3), kernels=kernels,
                ms_per_layer=round((rnn + gin) / NL, 3), rnn_ms_per_layer=round(rnn / NL, 3),
                rnn_us_per_step=round(rnn * 1e3 / (NL * T), 3),
                derived_matrix_floor_us_per_step=round(2 * 2 * Bp * 4 * H * H / F32_MATRIX_FLOPS * 1e6, 3),
                derived_l2_stream_floor_us_per_step=round(2 * (16 * H * H + Bp * H * H / 2) / L2_BYTES_PER_S * 1e6, 3))


def ops(args):
    import numpy as np
    import torch

    from s3prl_amd import _lib

    lib = _lib.load()
    B, T1, T2 = args.batch, 64, 320
    res = []
    for H in (512, 1024):
        rng = np.random.default_rng(H)
        w = (rng.standard_normal((2, 4 * H, H)) * (1.5 / np.sqrt(H))).astype(np.float32)
        wp = [C.c_void_p(np.ascontiguousarray(w[d]).ctypes.data) for d in range(2)]
        pre = (2.0 * torch.randn((2, B, T2, 4 * H), device="cuda"))
        ent = dict(H=H, B=B, lengths=[T1, T2])

        def bidir(T):
            p = pre[:, :, :T].contiguous()
            out = torch.empty((B, T, 2 * H), device="cuda")
            ln = (C.c_int32 * B)(*([T] * B))

            def run():
                _lib.check(lib.s3enc_op_lstm_bidir(C.c_void_p(p[0].data_ptr()), C.c_void_p(p[1].data_ptr()), wp[0], wp[1],
                                                   C.cast(ln, C.c_void_p), B, T, H, 4 * H, C.c_void_p(out.data_ptr()), 2 * H, None),
                           "s3enc_op_lstm_bidir")
            return statistics.median(timed(run, args.steps, args.warmup))

        def rnn_len(T, split):
            p = pre[0, :, :T].contiguous()
            out = torch.empty((B, T, H), device="cuda")
            ln = (C.c_int32 * B)(*([T] * B))

            def run():
                _lib.check(lib.s3enc_op_rnn_len(0, C.c_void_p(p.data_ptr()), wp[0], None, C.cast(ln, C.c_void_p), None, 0, B, T, H, 4 * H,
                                                C.c_void_p(out.data_ptr()), H, None), "s3enc_op_rnn_len")
            _lib.check(lib.s3enc_set_tuning(b"rnn_split", split), "s3enc_set_tuning")
            try:
                return statistics.median(timed(run, args.steps, args.warmup))
            finally:
                _lib.check(lib.s3enc_set_tuning(b"rnn_split", -1), "s3enc_set_tuning")

        per_step = lambda f, *a: round((f(T2, *a) - f(T1, *a)) * 1e3 / (T2 - T1), 3)  # noqa: E731
        ent["bidir_us_per_step"] = per_step(bidir)
        ent["bidir_us_per_step_and_direction"] = round(ent["bidir_us_per_step"] / 2, 3)
        if H <= 512:
            ent["rnn_len_one_launch_us_per_step"] = per_step(rnn_len, 0)
            ent["rnn_len_step_split8_us_per_step"] = per_step(rnn_len, 8)
            best = min(ent["rnn_len_one_launch_us_per_step"], ent["rnn_len_step_split8_us_per_step"])
            ent["bidir_per_direction_over_best_older"] = round(ent["bidir_us_per_step_and_direction"] / best, 3)
        Bp = -(-B // 32) * 32
        ent["derived_matrix_floor_us_per_step"] = round(2 * 2 * Bp * 4 * H * H / F32_MATRIX_FLOPS * 1e6, 3)
        ent["derived_l2_stream_floor_us_per_step"] = round(2 * (16 * H * H + Bp * H * H / 2) / L2_BYTES_PER_S * 1e6, 3)
        res.append(ent)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="decoar")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--secs", type=float, default=10.0)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-family", action="store_true")
    ap.add_argument("--no-ops", action="store_true")
    args = ap.parse_args()
    if args.steps < 5:
        ap.error("--steps must be at least 5 (the median of fewer runs is not a measurement)")

    import torch

    if not torch.cuda.is_available():
        raise SystemExit("decoar_bench needs the MI355X: there is no CPU fallback and no CPU timing")
    res = {}
    if not args.no_ops:
        res["ops"] = ops(args)
    if not args.no_family:
        res["family"] = family(args)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
