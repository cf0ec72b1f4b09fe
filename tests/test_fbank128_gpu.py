"""The ground the MAE-AST family stands on: s3enc_fbank_forward (csrc/fbank.hip) at 128 mel bins — torchaudio's kaldi defaults,
no deltas, no CMVN — against oracle/fbank_oracle.py::kaldi_fbank in float64, frame by frame.  Bounds: a frame's 128 log-mel values
are a few units each, so its relative error over the bins measures the fp32 spectrum GEMM and the log against the project's FP32_TOL;
the element bound is the one tests/test_fbank_gpu.py holds the 80-bin log-mel columns to."""

import ctypes as C

import numpy as np
import pytest

from oracle import encoder_oracle as O
from oracle import fbank_oracle as F

pytestmark = pytest.mark.gpu

FP32_TOL = 1e-4


@pytest.mark.parametrize("lengths, dc, scale", [([400, 559, 560], 0.0, 1.0), ([16000, 9999, 2960], 0.05, 0.3), ([40000], 0.0, 1.0)])
def test_fbank_at_128_bins_per_frame(lengths, dc, scale):
    import torch

    from s3prl_amd import _lib
    from s3prl_amd.synth import synth_wavs

    assert torch.cuda.is_available(), "these tests need the MI355X"
    lib = _lib.load()
    c = _lib.S3FbankConfig(16000, 128, 25.0, 10.0, 0.97, 0, 5, 0, 1e-10)
    wavs = synth_wavs(lengths, 31, dc=dc, scale=scale)
    held = [torch.from_numpy(w).cuda() for w in wavs]
    frames = [F.num_frames(n) for n in lengths]
    assert frames == [1 + (n - 400) // 160 for n in lengths]
    B, T = len(held), max(frames)
    out = torch.zeros((B, T, 128), dtype=torch.float32, device="cuda")
    ptrs = (C.c_void_p * B)(*[w.data_ptr() for w in held])
    rc = lib.s3enc_fbank_forward(C.byref(c), ptrs, (C.c_int64 * B)(*lengths), B, C.c_void_p(out.data_ptr()), T, torch.cuda.current_device(),
                                 C.c_void_p(torch.cuda.current_stream().cuda_stream))
    _lib.check(rc, "s3enc_fbank_forward")
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    worst = 0.0
    for b, w in enumerate(wavs):
        ref = F.kaldi_fbank(w.astype(np.float64), num_mel_bins=128)
        assert ref.shape == (frames[b], 128)
        rows = [O.rel_err(got[b, t], ref[t]) for t in range(frames[b])]
        worst = max(worst, max(rows))
        assert max(rows) < FP32_TOL and np.abs(got[b, :frames[b]] - ref).max() < 5e-4, (b, max(rows))
        assert np.all(got[b, frames[b]:] == 0)
    print(f"{lengths}: worst frame {worst:.2e}")
