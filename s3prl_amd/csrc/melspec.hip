// melspec.hip — BYOL-A's front end (upstream/byol_a/expert.py:45-60,83-107, torchaudio.transforms.MelSpectrogram's defaults), exact
// fp32, over a table of SEGMENTS of L samples each:
//   reflect-pad every segment by 512 about ITS OWN ends (center = True on the sub-wav; samples at or past the segment's `valid`
//   count are zeros: the utterance's zero padding)  ->  1 + L / 160 frames of 1024 samples every 160  ->  periodic hann(1024)
//   ->  |X|^2 over 513 one-sided bins, no normalisation  ->  64 HTK triangles in Hz between mel-spaced points (f_min 60, f_max 7800,
//   norm = None, over linspace(0, 8000, 513))  ->  (log(mel + FLT_EPSILON) - mean) / std, written as (segment, frame, mel).
// BYOL-S (upstream/byol_s/serab_byols/serab.py:136-144) runs the same front end with win_length = 400: torch.stft zero-pads the
// periodic hann(400) to 1024 with 312 zeros on either side — a second window table of the FFT kernel (win400), nothing else.
//
// Two forms of the spectrum (tuning key melspec_fft):
//   1  melspec_fft_kernel, one workgroup of 256 threads per frame: the windowed frame packed as 512 complex numbers z[n] = x[2n] +
//      i x[2n + 1], a 512-point radix-2 Stockham FFT in two LDS buffers (nine stages, one butterfly per thread and stage, a fixed
//      order: a frame's bits depend on its 1024 samples only), the split X[k] = (Z[k] + Z*[512 - k]) / 2 + e^(-2 pi i k / 1024)
//      (Z[k] - Z*[512 - k]) / 2i, the power, the sparse mel sum (band m walks its own bins in ascending order), log and the affine.
//      Twiddles come from one float64-built table e^(-2 pi i m / 1024), m = 0..512.  About 50 kFLOP per frame; 10 KiB LDS, no scratch.
//   0  fbank.hip's / logmel.hip's form at K = 1024: spectral.h's reflect_pad_kernel materialises every reflect-padded segment, the spectrum is an
//      overlapping-row GEMM (lda = 160) against hann x DFT folded in float64 into a (2 x 513) x 1024 matrix (2.1 MFLOP per frame), and
//      mel_rows_kernel is the same power -> mel -> log -> affine epilogue.  The yardstick and the fallback.
#include <cfloat>
#include <cmath>
#include <map>
#include <mutex>
#include <vector>

#include "kernels.h"
#include "spectral.h"

namespace s3 {

namespace {

constexpr int NFFT = 1024, NBIN = 513, HOP = 160, NMEL = 64, HALF = 512;

// sample i of frame t of a segment: padded position n = 160 t + i - 512 reflected about 0 and about L - 1 (L > 512: one reflection)
// (samples before `lo` are zeros too: a BYOL-S window that starts in front of its utterance)
__device__ __forceinline__ float seg_sample(const float* src, int nv, int L, int n, int lo = 0) {
    if (n < 0) n = -n;
    if (n >= L) n = 2 * (L - 1) - n;
    return n >= lo && n < nv ? src[n] : 0.f;
}

__global__ __launch_bounds__(256) void melspec_fft_kernel(const float* const* ptrs, const int* valid, int L, int T, const float2* tw,
                                                          const float* win, const int* bands, const float* wts, float mean, float std_,
                                                          float* out, long o_bs, long o_row, float* power, const int* lead) {
    __shared__ float2 za[HALF], zb[HALF];
    __shared__ float pw[NBIN + 3];
    const int tid = threadIdx.x;
    const long r = blockIdx.x;
    const int seg = (int)(r / T), t = (int)(r - (long)seg * T);
    const float* src = ptrs[seg];
    int nv = valid[seg];
    nv = nv < 0 ? 0 : (nv > L ? L : nv);
    const int lo = lead ? lead[seg] : 0;
    const int base = t * HOP - HALF;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int n = tid + 256 * h;
        za[n] = make_float2(seg_sample(src, nv, L, base + 2 * n, lo) * win[2 * n], seg_sample(src, nv, L, base + 2 * n + 1, lo) * win[2 * n + 1]);
    }
    __syncthreads();
    float2 *in = za, *ot = zb;
#pragma unroll 1
    for (int ns = 1; ns < HALF; ns <<= 1) {  // Stockham radix 2: natural order in, natural order out
        const int k = tid & (ns - 1);
        const float2 w = tw[k * (HALF / ns)];  // e^(-2 pi i k / (2 ns))
        const float2 a = in[tid], b = in[tid + 256];
        const float2 c = make_float2(b.x * w.x - b.y * w.y, b.x * w.y + b.y * w.x);
        const int j = ((tid - k) << 1) + k;
        ot[j] = make_float2(a.x + c.x, a.y + c.y);
        ot[j + ns] = make_float2(a.x - c.x, a.y - c.y);
        __syncthreads();
        float2* s = in;
        in = ot;
        ot = s;
    }
    // `in` holds Z; bins tid, tid + 256 and (thread 0) 512
    float* prow = power ? power + r * NBIN : nullptr;
    for (int k = tid; k < NBIN; k += 256) {
        const float2 zk = in[k & (HALF - 1)], zm = in[(HALF - k) & (HALF - 1)];
        const float er = 0.5f * (zk.x + zm.x), ei = 0.5f * (zk.y - zm.y);   // (Z[k] + conj Z[512 - k]) / 2
        const float orr = 0.5f * (zk.y + zm.y), oi = -0.5f * (zk.x - zm.x);  // (Z[k] - conj Z[512 - k]) / 2i
        const float2 w = tw[k];
        const float xr = er + (orr * w.x - oi * w.y), xi = ei + (orr * w.y + oi * w.x);
        const float v = xr * xr + xi * xi;
        pw[k] = v;
        if (prow) prow[k] = v;
    }
    __syncthreads();
    if (tid < NMEL) out[seg * o_bs + t * o_row + tid] = LogAffine{mean, std_}(mel_band_sum(pw, bands, wts, NMEL, tid));
}

struct MelspecPlan {
    float2* tw = nullptr;   // e^(-2 pi i m / 1024), m = 0..512
    float* win = nullptr;   // periodic hann(1024)
    float* win400 = nullptr;  // periodic hann(400) behind 312 zeros and in front of 312 (MelSpectrogram(win_length = 400) at n_fft = 1024)
    MelBank bank;           // the HTK bank, 64 bands over 513 bins, band by band
    float* dft = nullptr;   // the GEMM form's (2 * 513, 1024) matrix, built on first use
};
std::mutex g_mu;
std::map<int, MelspecPlan> g_plans;

hipError_t build_plan(MelspecPlan& pl) {
    std::vector<float2> tw(HALF + 1);
    for (int m = 0; m <= HALF; ++m) {
        const double a = 2.0 * M_PI * m / NFFT;
        tw[m] = make_float2((float)std::cos(a), (float)-std::sin(a));
    }
    const std::vector<double> h1024 = hann_periodic(NFFT), h400 = hann_periodic(400);
    std::vector<float> win(h1024.begin(), h1024.end()), win400(NFFT, 0.f);
    for (int i = 0; i < 400; ++i) win400[(NFFT - 400) / 2 + i] = (float)h400[i];
    hipError_t e = to_device(&pl.tw, tw);
    if (e == hipSuccess) e = to_device(&pl.win, win);
    if (e == hipSuccess) e = to_device(&pl.win400, win400);
    if (e == hipSuccess) e = upload_bank(pl.bank, htk_bank(NBIN, 60.0, 7800.0, NMEL), NBIN, NMEL);
    return e;
}

}  // namespace

// torchaudio.functional.melscale_fbanks(513, 60, 7800, 64, 16000, norm = None, "htk") in float64, stored band by band
void melspec_bank(std::vector<int>& bands, std::vector<float>& wts) { sparsify(htk_bank(NBIN, 60.0, 7800.0, NMEL), NBIN, NMEL, bands, wts); }

long melspec_num_frames(long L) { return 1 + L / HOP; }
size_t melspec_sig_elems(long nseg, long L) { return (size_t)nseg * (size_t)((L + NFFT + 3) & ~3L); }
size_t melspec_spec_elems(long nseg, long L) { return (size_t)nseg * (size_t)melspec_num_frames(L) * 2 * NBIN; }

const char* melspec_refusal(const MelspecParams& p) {
    if (!p.ptrs || !p.valid || !p.out) return "null operand";
    if (p.nseg < 1) return "no segments";
    if (p.L <= 512) return "a segment of at most 512 samples cannot be reflect-padded by 512 (n_fft / 2)";
    if (p.win400 < 0 || p.win400 > 1) return "win400 must be 0 or 1";
    if (!p.win400 && p.L < 1120) return "a segment below 1120 samples has fewer than 8 frames: nothing survives three 2 x 2 pools";
    if (p.win400 && !p.fft) return "the 400-sample window is built for the FFT form only";
    if (p.lead && !p.fft) return "leading zeros are built for the FFT form only";
    if (p.L > (1 << 24)) return "segment too long";
    const long T = melspec_num_frames(p.L);
    if ((long)p.nseg * T > 0x7fffffffL / (2 * NBIN) || p.nseg > 65535 * 16) return "too many frames";
    if (p.o_row < NMEL || p.o_bs < (T - 1) * p.o_row + NMEL) return "the output pitches are smaller than one segment";
    if (!p.fft && (!p.sig || !p.spec)) return "the GEMM form needs its scratch buffers";
    if (!p.fft && p.nseg > 65535) return "too many segments for the GEMM form";
    return nullptr;
}

hipError_t launch_melspec(const MelspecParams& p, hipStream_t st) {
    if (melspec_refusal(p)) return hipErrorInvalidValue;
    const long T = melspec_num_frames(p.L);
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    MelspecPlan* pl;
    {
        std::lock_guard<std::mutex> lock(g_mu);
        pl = &g_plans[dev];
        if (!pl->tw && (e = build_plan(*pl)) != hipSuccess) return e;
        if (!p.fft && !pl->dft && (e = to_device(&pl->dft, fold_dft(hann_periodic(NFFT).data(), NFFT, NFFT))) != hipSuccess) return e;
    }
    const unsigned frames = (unsigned)(p.nseg * T);
    if (p.fft) {
        hipLaunchKernelGGL(melspec_fft_kernel, dim3(frames), dim3(256), 0, st, p.ptrs, p.valid, p.L, (int)T, pl->tw,
                           p.win400 ? pl->win400 : pl->win, pl->bank.bands, pl->bank.wts, p.mean, p.std_, p.out, p.o_bs, p.o_row, p.power, p.lead);
        return hipGetLastError();
    }
    const long Lp = (p.L + NFFT + 3) & ~3L;
    hipLaunchKernelGGL(reflect_pad_kernel<int>, dim3((unsigned)((Lp + 255) / 256), p.nseg), dim3(256), 0, st, p.ptrs, p.valid,
                       (const float*)nullptr, (long)p.L, HALF, Lp, p.sig);
    GemmParams g{};
    g.A = p.sig;
    g.lda = HOP;  // overlapping rows: frame t starts at padded sample 160 t
    g.a_bs = Lp;
    g.W = pl->dft;
    g.M = (int)T;
    g.N = 2 * NBIN;
    g.K = NFFT;
    g.batches = p.nseg;
    g.out32 = p.spec;
    g.ldo = 2 * NBIN;
    g.o_bs = T * 2 * NBIN;
    e = launch_gemm(F32, g, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((mel_rows_kernel<POWER_FMA, LogAffine>), dim3(frames), dim3(128), NBIN * sizeof(float), st, p.spec, NBIN, (int)T,
                       pl->bank.bands, pl->bank.wts, NMEL, LogAffine{p.mean, p.std_}, p.out, p.o_bs, p.o_row, p.power);
    return hipGetLastError();
}

}  // namespace s3
