// logmel.hip — the `OnlinePreprocessor` front end of the Mockingjay / TERA / AudioALBERT family (upstream/baseline/preprocessor.py:64-223,
// mockingjay/builder.py:129-134,394-400), exact fp32:
//   per utterance  x * 10^(target_level / 20) / (rms + 1e-10)   ->  zero-pad the batch to max_len
//   torch.stft(n_fft 400, hop 160, periodic hann, center = True, reflect) on the PADDED batch: T = 1 + max_len / 160 frames
//   |X|^2 -> 201 -> n_mels HTK triangles (MelScale: f_min 0, f_max 8000, no norm) -> log(x + 1e-10)
//   CMVN per mel bin over the utterance's feats_len[b] frames (unbiased std, eps added to the std); rows behind are zeros.
//
// The frame spectrum is the same overlapping-row GEMM as fbank.hip's (lda = 160 < K = 400) against hann x DFT folded in fp64 into a
// (2 x 201) x 400 matrix.  The edge frames read reflected or zero samples the caller's buffer does not hold, so logmel_pad_kernel
// first writes every utterance's scaled signal into a (B, max_len + 400) buffer: index j is position p = j - 200 of the padded batch
// row, reflected about 0 and about max_len - 1 (torch's reflect padding of the PADDED row: a shorter utterance's tail frames see the
// batch's zeros, the longest sees its own reflection, one ending within 200 samples of max_len a mixture), value
// p < len[b] ? x[p] * scale[b] : 0.  The scale comes from logmel_rms_kernel (sum of squares in double, one workgroup per utterance).
#include <cmath>
#include <map>
#include <mutex>
#include <vector>

#include "kernels.h"

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

__global__ __launch_bounds__(256) void logmel_pad_kernel(const float* const* wavs, const long* lens, const float* scale, long max_len,
                                                         long Lp, float* sig) {
    const int b = blockIdx.y;
    const long j = (long)blockIdx.x * 256 + threadIdx.x;
    if (j >= Lp) return;
    long p = j - 200;
    if (p < 0) p = -p;
    if (p >= max_len) p = 2 * (max_len - 1) - p;  // max_len > 200: p stays inside [0, max_len)
    float v = 0.f;
    if (j < max_len + 400 && p >= 0 && p < lens[b]) v = wavs[b][p] * scale[b];
    sig[(long)b * Lp + j] = v;
}

// one workgroup per frame: |X|^2 -> mel triangles -> log(x + eps)
__global__ __launch_bounds__(128) void logmel_mel_kernel(const float* spec, int nbin, int T, const float* banksT, int nmel, float eps,
                                                         float* out, long o_bs) {
    extern __shared__ float pw[];
    const long r = blockIdx.x;  // frame r = b * T + t
    const long b = r / T, t = r - b * T;
    const float* s = spec + r * (2L * nbin);
    for (int k = threadIdx.x; k < nbin; k += blockDim.x) {
        const float re = s[k], im = s[nbin + k];
        pw[k] = re * re + im * im;
    }
    __syncthreads();
    for (int m = threadIdx.x; m < nmel; m += blockDim.x) {
        float acc = 0.f;
        for (int k = 0; k < nbin; ++k) acc = fmaf(pw[k], banksT[k * nmel + m], acc);
        out[b * o_bs + t * nmel + m] = logf(acc + eps);
    }
}

// workgroup (f, b): mean / unbiased std of mel bin f over rows [0, cnt[b]), in place; rows [cnt[b], T) are written as zeros
__global__ __launch_bounds__(256) void logmel_cmvn_kernel(float* x, const int* cnt, int T, int nmel, long o_bs, float eps) {
    __shared__ double red[4];
    const int f = blockIdx.x, b = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float* xb = x + (long)b * o_bs + f;
    int L = cnt[b];
    L = L < 0 ? 0 : (L > T ? T : L);
    auto block_sum = [&](double v) {
        v = wave_sum_d(v);
        __syncthreads();
        if (lane == 0) red[wave] = v;
        __syncthreads();
        return red[0] + red[1] + red[2] + red[3];
    };
    double s = 0.0;
    for (int t = threadIdx.x; t < L; t += 256) s += xb[(long)t * nmel];
    const double mean = block_sum(s) / (double)L;
    double q = 0.0;
    for (int t = threadIdx.x; t < L; t += 256) {
        const double d = xb[(long)t * nmel] - mean;
        q += d * d;
    }
    const double var = block_sum(q) / (double)(L - 1);  // unbiased (torch.std); one frame -> nan like torch (the callers refuse it)
    const float inv = (float)(1.0 / ((double)eps + sqrt(var)));
    for (int t = threadIdx.x; t < T; t += 256) xb[(long)t * nmel] = t < L ? (float)(xb[(long)t * nmel] - mean) * inv : 0.f;
}

struct LogmelPlan {
    float* dft = nullptr;     // (2 * 201, 400): rows 0..200 hann * cos, 201..401 -hann * sin
    float* banksT = nullptr;  // (201, nmel)
};
std::mutex g_mu;
std::map<std::pair<int, int>, LogmelPlan> g_plans;

hipError_t build_plan(LogmelPlan& pl, int nmel) {
    const int N = 400, nb = 201;
    std::vector<float> M((size_t)2 * nb * N);
    for (int r = 0; r < nb; ++r)
        for (int i = 0; i < N; ++i) {
            const double w = 0.5 - 0.5 * std::cos(2.0 * M_PI * i / N);  // torch.hann_window(400): periodic
            const double a = 2.0 * M_PI * (double)((long)r * i % N) / N;
            M[(size_t)r * N + i] = (float)(w * std::cos(a));
            M[(size_t)(nb + r) * N + i] = (float)(-w * std::sin(a));
        }
    // torchaudio.functional.melscale_fbanks(201, 0, 8000, nmel, 16000, norm = None, "htk"): triangles in Hz between mel-spaced points
    std::vector<float> bT((size_t)nb * nmel, 0.f);
    auto hz2mel = [](double f) { return 2595.0 * std::log10(1.0 + f / 700.0); };
    auto mel2hz = [](double m) { return 700.0 * (std::pow(10.0, m / 2595.0) - 1.0); };
    const double m_lo = hz2mel(0.0), m_hi = hz2mel(8000.0);
    std::vector<double> fpt(nmel + 2);
    for (int i = 0; i < nmel + 2; ++i) fpt[i] = mel2hz(m_lo + (m_hi - m_lo) * i / (nmel + 1));
    for (int k = 0; k < nb; ++k) {
        const double f = 8000.0 * k / (nb - 1);
        for (int m = 0; m < nmel; ++m) {
            const double down = (f - fpt[m]) / (fpt[m + 1] - fpt[m]), up = (fpt[m + 2] - f) / (fpt[m + 2] - fpt[m + 1]);
            bT[(size_t)k * nmel + m] = (float)std::fmax(0.0, std::fmin(down, up));
        }
    }
    hipError_t e = hipMalloc((void**)&pl.dft, M.size() * 4);
    if (e != hipSuccess) return e;
    e = hipMemcpy(pl.dft, M.data(), M.size() * 4, hipMemcpyHostToDevice);
    if (e != hipSuccess) return e;
    e = hipMalloc((void**)&pl.banksT, bT.size() * 4);
    if (e != hipSuccess) return e;
    return hipMemcpy(pl.banksT, bT.data(), bT.size() * 4, hipMemcpyHostToDevice);
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
    if (p.B <= 0 || p.max_len <= 200 || p.n_mels < 1 || p.n_mels > 256) return hipErrorInvalidValue;
    const long T = logmel_num_frames(p.max_len), Lp = (p.max_len + 400 + 3) & ~3L;
    if ((long)p.B * T > 0x7fffffffL / 402 || p.B > 65535 || p.o_bs < T * p.n_mels) return hipErrorInvalidValue;
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    LogmelPlan* pl;
    {
        std::lock_guard<std::mutex> lock(g_mu);
        pl = &g_plans[std::make_pair(dev, p.n_mels)];
        if (!pl->dft) {
            e = build_plan(*pl, p.n_mels);
            if (e != hipSuccess) return e;
        }
    }
    hipLaunchKernelGGL(logmel_rms_kernel, dim3(p.B), dim3(1024), 0, st, p.wavs, p.lens, std::pow(10.0, (double)p.target_level / 20.0),
                       p.scale);
    hipLaunchKernelGGL(logmel_pad_kernel, dim3((unsigned)((Lp + 255) / 256), p.B), dim3(256), 0, st, p.wavs, p.lens, p.scale,
                       p.max_len, Lp, p.sig);
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
    hipLaunchKernelGGL(logmel_mel_kernel, dim3((unsigned)(p.B * T)), dim3(128), 201 * sizeof(float), st, p.spec, 201, (int)T,
                       pl->banksT, p.n_mels, 1e-10f, p.out, p.o_bs);
    if (p.cmvn)
        hipLaunchKernelGGL(logmel_cmvn_kernel, dim3(p.n_mels, p.B), dim3(256), 0, st, p.out, p.counts, (int)T, p.n_mels, p.o_bs, 1e-10f);
    return hipGetLastError();
}

}  // namespace s3
