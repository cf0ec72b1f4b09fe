// logmel.hip — the `OnlinePreprocessor` front end of the Mockingjay / TERA / AudioALBERT family (upstream/baseline/preprocessor.py:64-223,
// mockingjay/builder.py:129-134,394-400), exact fp32:
//   per utterance  x * 10^(target_level / 20) / (rms + 1e-10)   ->  zero-pad the batch to max_len
//   torch.stft(n_fft 400, hop 160, periodic hann, center = True, reflect) on the PADDED batch: T = 1 + max_len / 160 frames
//   |X|^2 -> 201 -> n_mels HTK triangles (MelScale: f_min 0, f_max 8000, no norm) -> log(x + 1e-10)
//   CMVN per mel bin over the utterance's feats_len[b] frames (unbiased std, eps added to the std); rows behind are zeros.
//
// The frame spectrum is the same overlapping-row GEMM as fbank.hip's (lda = 160 < K = 400) against hann x DFT folded in fp64 into a
// (2 x 201) x 400 matrix.  The edge frames read reflected or zero samples the caller's buffer does not hold, so spectral.h's
// reflect_pad_kernel first writes every utterance's scaled signal into a (B, max_len + 400) buffer: index j is position p = j - 200 of the padded batch
// row, reflected about 0 and about max_len - 1 (torch's reflect padding of the PADDED row: a shorter utterance's tail frames see the
// batch's zeros, the longest sees its own reflection, one ending within 200 samples of max_len a mixture), value
// p < len[b] ? x[p] * scale[b] : 0.  The scale comes from logmel_rms_kernel (sum of squares in double, one workgroup per utterance).
#include <cmath>
#include <map>
#include <mutex>
#include <vector>

#include "kernels.h"
#include "spectral.h"

namespace s3 {

namespace {

__global__ __launch_bounds__(1024) void logmel_rms_kernel(const float* const* wavs, const long* lens, double level, float* scale) {
    __shared__ double red[16];
    const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float* x = wavs[b];
    const long n = lens[b];
    double s = 0.0;
    for (long i = threadIdx.x; i < n; i += 1024) {
        const double v = x[i];
        s += v * v;
    }
    s = wave_sum_d(s);
    if (lane == 0) red[wave] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int w = 0; w < 16; ++w) t += red[w];
        // builder.py:129-134 in fp32: rms = mean(x^2)^0.5, scalar = 10^(level / 20) / (rms + 1e-10)
        const float rms = sqrtf((float)(t / (double)n));
        scale[b] = (float)level / (rms + 1e-10f);
    }
}

struct LogmelPlan {
    float* dft = nullptr;     // (2 * 201, 400): rows 0..200 hann * cos, 201..401 -hann * sin
    MelBank bank;             // the HTK bank over 201 bins, band by band
};
std::mutex g_mu;
std::map<std::pair<int, int>, LogmelPlan> g_plans;

hipError_t build_plan(LogmelPlan& pl, int nmel) {
    // torch.hann_window(400) x the 400-point DFT; torchaudio's MelScale(n_mels, f_min 0, f_max 8000, norm = None, "htk") over 201 bins
    hipError_t e = to_device(&pl.dft, fold_dft(hann_periodic(400).data(), 400, 400));
    return e != hipSuccess ? e : upload_bank(pl.bank, htk_bank(201, 0.0, 8000.0, nmel), 201, nmel);
}

}  // namespace

long logmel_num_frames(long max_len) { return 1 + max_len / 160; }

int logmel_frame_count(long length, long max_len) {
    const long T = logmel_num_frames(max_len);
    const double rate = (double)max_len / (double)T;           // preprocessor.py:204: wavs.size(-1) / feats.size(-1)
    long v = (long)std::nearbyint((double)length / rate);      // Python's round(): half to even, as the default rounding mode
    return (int)(v < 0 ? 0 : (v > T ? T : v));
}

size_t logmel_sig_elems(int B, long max_len) { return (size_t)B * (size_t)((max_len + 400 + 3) & ~3L); }
size_t logmel_spec_elems(int B, long max_len) { return (size_t)B * (size_t)logmel_num_frames(max_len) * 402; }

hipError_t launch_logmel(const LogmelParams& p, hipStream_t st) {
    const int F = p.linear ? 201 : p.n_mels;
    if (p.B <= 0 || p.max_len <= 200 || F < 1 || F > 256) return hipErrorInvalidValue;
    const long T = logmel_num_frames(p.max_len), Lp = (p.max_len + 400 + 3) & ~3L;
    if ((long)p.B * T > 0x7fffffffL / 402 || p.B > 65535 || p.o_bs < T * F) return hipErrorInvalidValue;
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    LogmelPlan* pl;
    {
        std::lock_guard<std::mutex> lock(g_mu);
        pl = &g_plans[std::make_pair(dev, p.linear ? 1 : p.n_mels)];  // linear reads the operand only
        if (!pl->dft) {
            e = build_plan(*pl, p.linear ? 1 : p.n_mels);
            if (e != hipSuccess) return e;
        }
    }
    if (!p.no_level)
        hipLaunchKernelGGL(logmel_rms_kernel, dim3(p.B), dim3(1024), 0, st, p.wavs, p.lens, std::pow(10.0, (double)p.target_level / 20.0),
                           p.scale);
    hipLaunchKernelGGL(reflect_pad_kernel<long>, dim3((unsigned)((Lp + 255) / 256), p.B), dim3(256), 0, st, p.wavs, p.lens,
                       p.no_level ? (const float*)nullptr : (const float*)p.scale, p.max_len, 200, Lp, p.sig);
    GemmParams g{};
    g.A = p.sig;
    g.lda = 160;  // overlapping rows: frame t starts at padded sample 160 t
    g.a_bs = Lp;
    g.W = pl->dft;
    g.M = (int)T;
    g.N = 402;
    g.K = 400;
    g.batches = p.B;
    g.out32 = p.spec;
    g.ldo = 402;
    g.o_bs = T * 402;
    e = launch_gemm(F32, g, st);
    if (e != hipSuccess) return e;
    if (p.linear)
        launch_spectrum_rows<POWER>(p.spec, 201, T, p.B, LogAdd{1e-10f}, nullptr, p.out, 201L, p.o_bs, st);
    else
        hipLaunchKernelGGL((mel_rows_kernel<POWER, LogAdd>), dim3((unsigned)(p.B * T)), dim3(128), 201 * sizeof(float), st, p.spec, 201,
                           (int)T, pl->bank.bands, pl->bank.wts, p.n_mels, LogAdd{1e-10f}, p.out, p.o_bs, (long)p.n_mels, nullptr);
    if (p.cmvn) launch_cmvn(p.out, p.counts, (int)T, F, p.B, F, p.o_bs, 1e-10f, st);
    return hipGetLastError();
}

}  // namespace s3
