// fbank.hip — the `fbank` baseline upstream (BASELINE configs[0]) on the GPU:
//   torchaudio.compliance.kaldi.fbank(80 mel bins, 25 ms / 10 ms, log) -> 2 x ComputeDeltas(win 5) -> CMVN over time
//   (upstream/baseline/extracter.py:32-90, baseline/fbank.yaml).
//
// Framing, DC removal, pre-emphasis, the window (povey; hamming for APC's front end, FbankParams::window) and the zero-padded 512-point real DFT are all linear in the
// 400 samples of a frame, so they are folded (in fp64, once per configuration) into ONE (2*257) x 400 matrix; the
// spectrum of every frame is then a GEMM whose A rows OVERLAP in the raw waveform (row t starts at sample 160 t:
// lda = 160 < K = 400) — the same implicit-GEMM addressing as the strided convs, served by gemm.hip's exact-fp32 MFMA
// kernel straight from the caller's PCM.  Three small HBM-bound kernels finish the job:
//   mel_rows_kernel    |X|^2 -> 80 triangular mel filters -> log(max(., eps))          (spectral.h, one workgroup per frame)
//   fbank_delta_kernel delta and delta-delta with replicate padding                     (thread per (t, bin))
//   cmvn_kernel        per-dimension mean / unbiased std over time, two-pass, in place  (spectral.hip, workgroup per dimension)
#include <cmath>
#include <map>
#include <mutex>
#include <vector>

#include "kernels.h"
#include "spectral.h"

namespace s3 {

namespace {

// out[t][nmel*(o+1) + b] = delta of order o+1; d[t] = sum_k k * x[clamp(t+k)] / denom  (replicate padding)
__global__ void fbank_delta_kernel(float* out, long T, int nmel, int ldo, int order, int n, float inv_denom) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= T * nmel) return;
    const long t = idx / nmel;
    const int b = (int)(idx % nmel);
    auto x0 = [&](long tt) { return out[(tt < 0 ? 0 : (tt >= T ? T - 1 : tt)) * ldo + b]; };
    auto d1 = [&](long tt) {
        tt = tt < 0 ? 0 : (tt >= T ? T - 1 : tt);
        float a = 0.f;
        for (int k = -n; k <= n; ++k) a += (float)k * x0(tt + k);
        return a * inv_denom;
    };
    if (order >= 1) out[t * ldo + nmel + b] = d1(t);
    if (order >= 2) {
        float a = 0.f;
        for (int k = -n; k <= n; ++k) a += (float)k * d1(t + k);
        out[t * ldo + 2 * nmel + b] = a * inv_denom;
    }
}

struct FbankPlan {
    int size, shift, padded, nbin, nmel;
    float* dft = nullptr;     // (2*nbin, size) fp32: rows 0..nbin-1 cos, nbin.. -sin, pre-processing folded in
    MelBank bank;             // the kaldi bank, band by band
};
// Scratch is per (device, STREAM): the plan's constants are shared, but two experts / two streams running the same
// configuration concurrently must not share the spectrum workspace (re-use within one stream is stream-ordered).
struct FbankScratch {
    float* spec = nullptr;    // workspace (frames, 2*nbin)
    size_t spec_elems = 0;
    float* stage = nullptr;   // aligned copy of a misaligned waveform
    size_t stage_elems = 0;
};

std::mutex g_mu;
std::map<std::vector<long>, FbankPlan> g_plans;
std::map<std::pair<int, uintptr_t>, FbankScratch> g_scratch;

hipError_t build_plan(FbankPlan& pl, int nmel, int size, int shift, double preemph, int sample_rate, int window) {
    pl.size = size;
    pl.shift = shift;
    pl.padded = 1;
    while (pl.padded < size) pl.padded <<= 1;
    pl.nbin = pl.padded / 2 + 1;
    pl.nmel = nmel;
    const int N = size, nb = pl.nbin;
    // D = diag(window) * P(pre-emphasis, first sample replicated) * C(remove mean), as a dense N x N fp64 matrix
    std::vector<double> D((size_t)N * N, 0.0), tmp((size_t)N * N, 0.0);
    for (int i = 0; i < N; ++i)
        for (int j = 0; j < N; ++j) tmp[(size_t)i * N + j] = (i == j ? 1.0 : 0.0) - 1.0 / N;  // C
    for (int i = 0; i < N; ++i) {
        const double w = window == 1   ? 0.54 - 0.46 * std::cos(2.0 * M_PI * i / (N - 1))             // hamming
                         : window == 2 ? 0.5 - 0.5 * std::cos(2.0 * M_PI * i / (N - 1))               // hanning
                                       : std::pow(0.5 - 0.5 * std::cos(2.0 * M_PI * i / (N - 1)), 0.85);  // povey
        const int ip = i == 0 ? 0 : i - 1;
        for (int j = 0; j < N; ++j) D[(size_t)i * N + j] = w * (tmp[(size_t)i * N + j] - preemph * tmp[(size_t)ip * N + j]);
    }
    hipError_t e = to_device(&pl.dft, fold_dft_dense(D.data(), N, pl.padded));
    return e != hipSuccess ? e : upload_bank(pl.bank, kaldi_bank(nb, nmel, sample_rate, pl.padded), nb, nmel);
}

// under g_mu
hipError_t plan_for(const FbankParams& c, int dev, int size, int shift, FbankPlan** out) {
    const std::vector<long> key{dev, c.num_mel_bins, size, shift, (long)std::lround(c.preemph * 1e6), c.sample_rate, c.window};
    FbankPlan& pl = g_plans[key];
    *out = &pl;
    return pl.dft ? hipSuccess : build_plan(pl, c.num_mel_bins, size, shift, c.preemph, c.sample_rate, c.window);
}

}  // namespace

hipError_t fbank_operand(const FbankParams& c, FbankOperand* op) {
    const int size = (int)(c.sample_rate * c.frame_length_ms * 0.001), shift = (int)(c.sample_rate * c.frame_shift_ms * 0.001);
    if (size <= 0 || shift <= 0 || (size & 3) || (shift & 3) || c.num_mel_bins <= 0 || c.window < 0 || c.window > 2)
        return hipErrorInvalidValue;
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    std::lock_guard<std::mutex> lock(g_mu);
    FbankPlan* pl = nullptr;
    e = plan_for(c, dev, size, shift, &pl);
    if (e != hipSuccess) return e;
    *op = FbankOperand{pl->dft, pl->bank, pl->size, pl->shift, pl->nbin};
    return hipSuccess;
}

void launch_fbank_delta(float* out, long T, int nmel, int ldo, int order, int delta_win, hipStream_t st) {
    const int nw = (delta_win - 1) / 2;
    const float inv = 3.0f / (float)(nw * (nw + 1) * (2 * nw + 1));
    const long tot = T * nmel;
    hipLaunchKernelGGL(fbank_delta_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, out, T, nmel, ldo, order, nw, inv);
}

long fbank_num_frames(long n, const FbankParams& c) {
    const int size = (int)(c.sample_rate * c.frame_length_ms * 0.001), shift = (int)(c.sample_rate * c.frame_shift_ms * 0.001);
    return n < size ? 0 : 1 + (n - size) / shift;  // snip_edges
}

// One utterance: wav (device, n samples) -> out (device, frames x ldo), columns [0, nmel*(order+1)).
hipError_t launch_fbank(const FbankParams& c, const float* wav, long n, float* out, int ldo, hipStream_t st) {
    const int size = (int)(c.sample_rate * c.frame_length_ms * 0.001), shift = (int)(c.sample_rate * c.frame_shift_ms * 0.001);
    const long T = fbank_num_frames(n, c);
    if (T <= 0) return hipSuccess;
    if (size <= 0 || shift <= 0 || (size & 3) || (shift & 3) || c.num_mel_bins <= 0 || c.delta_order < 0 || c.delta_order > 2 ||
        c.window < 0 || c.window > 2)
        return hipErrorInvalidValue;
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    std::lock_guard<std::mutex> lock(g_mu);
    FbankPlan* plan = nullptr;
    e = plan_for(c, dev, size, shift, &plan);
    if (e != hipSuccess) return e;
    FbankPlan& pl = *plan;
    const int N2 = 2 * pl.nbin;
    FbankScratch& sc = g_scratch[std::make_pair(dev, (uintptr_t)st)];
    if ((size_t)T * N2 > sc.spec_elems) {
        if (sc.spec) (void)hipFree(sc.spec);  // device-synchronising: nothing in flight still uses it
        sc.spec = nullptr;
        sc.spec_elems = (size_t)T * N2 + (size_t)T * N2 / 4;
        e = hipMalloc((void**)&sc.spec, sc.spec_elems * 4);
        if (e != hipSuccess) return e;
    }
    const float* a = wav;
    if (((uintptr_t)wav) & 15) {  // the GEMM loads 16-byte vectors: stage a misaligned waveform once
        if ((size_t)n > sc.stage_elems) {
            if (sc.stage) (void)hipFree(sc.stage);
            sc.stage = nullptr;
            sc.stage_elems = (size_t)n + (size_t)n / 4;
            e = hipMalloc((void**)&sc.stage, sc.stage_elems * 4);
            if (e != hipSuccess) return e;
        }
        e = hipMemcpyAsync(sc.stage, wav, (size_t)n * 4, hipMemcpyDeviceToDevice, st);
        if (e != hipSuccess) return e;
        a = sc.stage;
    }
    GemmParams g{};
    g.A = a;
    g.lda = shift;  // overlapping rows: frame t starts at sample t * shift
    g.a_bs = 0;
    g.W = pl.dft;
    g.M = (int)T;
    g.N = N2;
    g.K = size;
    g.batches = 1;
    g.out32 = sc.spec;
    g.ldo = N2;
    g.o_bs = 0;
    e = launch_gemm(F32, g, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((mel_rows_kernel<POWER, LogFloor>), dim3((unsigned)T), dim3(128), pl.nbin * sizeof(float), st, sc.spec, pl.nbin,
                       (int)T, pl.bank.bands, pl.bank.wts, pl.nmel, LogFloor{FLT_EPSILON}, out, 0L, (long)ldo, nullptr);
    if (c.delta_order > 0) launch_fbank_delta(out, T, pl.nmel, ldo, c.delta_order, c.delta_win, st);
    if (c.use_cmvn)
        launch_cmvn(out, nullptr, (int)T, pl.nmel * (c.delta_order + 1), 1, ldo, 0, c.cmvn_eps, st);
    return hipGetLastError();
}

// ---- the batch-wide pass ------------------------------------------------------------------------------------------------------------
// The spectrum of a frame is 2 * nbin floats (2 * 257 at the kaldi geometry: 66 MB at 32 x 10 s).  A batch whose spectra outgrow the cap
// is walked in chunks of whole utterances; one utterance above the cap is a chunk of its own.
size_t fbank_batch_spec_cap() { return (size_t)128 << 20; }

int fbank_batch_chunk(int B, long Fmax, int nbin, size_t cap_bytes) {
    const size_t per = (size_t)(Fmax > 0 ? Fmax : 1) * 2 * (size_t)nbin * sizeof(float);
    const size_t fit = (cap_bytes ? cap_bytes : fbank_batch_spec_cap()) / per;
    return fit < 1 ? 1 : (fit > (size_t)B ? B : (int)fit);
}

size_t fbank_batch_workspace(const FbankParams& c, int B, long Fmax, size_t cap_bytes) {
    const int size = (int)(c.sample_rate * c.frame_length_ms * 0.001);
    int padded = 1;
    while (padded < size) padded <<= 1;
    const int nbin = padded / 2 + 1;
    return (size_t)fbank_batch_chunk(B, Fmax, nbin, cap_bytes) * (size_t)Fmax * 2 * nbin * sizeof(float);
}

// pcm: (B, row_stride) with row b's samples from pcm + b * row_stride (16-byte aligned, row_stride a multiple of 4, at least
// size + (Fmax - 1) * shift); frames: device [B], the utterance's own frame count F_b <= Fmax.  out: (B, Fmax, ldo), columns [0, nmel):
// rows [0, F_b) the log-mels with the CMVN over those F_b rows, rows [F_b, Fmax) zeros — written by the CMVN kernel, the last one to
// touch them, whatever the samples behind the utterance held.  A frame's arithmetic is launch_fbank's: the same operand, the same K
// order in the GEMM, the same band sums, the same reduction order over an utterance's own rows.
hipError_t launch_fbank_batch(const FbankParams& c, const float* pcm, long row_stride, const int* frames, int B, long Fmax, float* out,
                              int ldo, float* spec, size_t spec_bytes, size_t cap_bytes, hipStream_t st) {
    const int size = (int)(c.sample_rate * c.frame_length_ms * 0.001), shift = (int)(c.sample_rate * c.frame_shift_ms * 0.001);
    if (B <= 0 || Fmax <= 0) return hipSuccess;
    if (size <= 0 || shift <= 0 || (size & 3) || (shift & 3) || c.num_mel_bins <= 0 || c.delta_order != 0 || !c.use_cmvn || c.window < 0 ||
        c.window > 1 || (((uintptr_t)pcm) & 15) || (row_stride & 3) || row_stride < size + (Fmax - 1) * shift || Fmax > 0x7fffffffL ||
        ldo < c.num_mel_bins)
        return hipErrorInvalidValue;
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    FbankPlan* plan = nullptr;
    {
        std::lock_guard<std::mutex> lock(g_mu);
        e = plan_for(c, dev, size, shift, &plan);
        if (e != hipSuccess) return e;
    }
    const FbankPlan& pl = *plan;  // (a plan is never rebuilt or freed: the pointer outlives the lock)
    const int N2 = 2 * pl.nbin;
    const int chunk = fbank_batch_chunk(B, Fmax, pl.nbin, cap_bytes);
    if (!spec || spec_bytes < (size_t)chunk * Fmax * N2 * sizeof(float)) return hipErrorInvalidValue;
    for (int b0 = 0; b0 < B; b0 += chunk) {
        const int nb = B - b0 < chunk ? B - b0 : chunk;
        GemmParams g{};
        g.A = pcm + (long)b0 * row_stride;
        g.lda = shift;  // overlapping rows: frame t of utterance b starts at sample b * row_stride + t * shift
        g.a_bs = row_stride;
        g.W = pl.dft;
        g.M = (int)Fmax;
        g.N = N2;
        g.K = size;
        g.batches = nb;
        g.out32 = spec;
        g.ldo = N2;
        g.o_bs = Fmax * N2;
        e = launch_gemm(F32, g, st);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL((mel_rows_kernel<POWER, LogFloor>), dim3((unsigned)((long)nb * Fmax)), dim3(128), pl.nbin * sizeof(float), st, spec,
                           pl.nbin, (int)Fmax, pl.bank.bands, pl.bank.wts, pl.nmel, LogFloor{FLT_EPSILON}, out + (long)b0 * Fmax * ldo,
                           Fmax * (long)ldo, (long)ldo, nullptr);
    }
    launch_cmvn(out, frames, (int)Fmax, pl.nmel, B, ldo, Fmax * (long)ldo, c.cmvn_eps, st);
    return hipGetLastError();
}

// ---- the window-wise pass -----------------------------------------------------------------------------------------------------------
namespace {
struct LogFloorAffine {  // SSAST: (log(max(e, eps)) + add) / div, an fp32 add followed by an fp32 divide
    float eps, add, div;
    __device__ float operator()(float acc) const {
#pragma clang fp contract(off)
        return (logf(fmaxf(acc, eps)) + add) / div;
    }
};
}  // namespace

hipError_t launch_fbank_windows(const FbankParams& c, const float* pcm, long row_stride, int nwin, long F, float add, float div, float* out,
                                long out_bs, int ldo, float* spec, size_t spec_bytes, size_t cap_bytes, hipStream_t st) {
    const int size = (int)(c.sample_rate * c.frame_length_ms * 0.001), shift = (int)(c.sample_rate * c.frame_shift_ms * 0.001);
    if (nwin <= 0 || F <= 0) return hipSuccess;
    if (size <= 0 || shift <= 0 || (size & 3) || (shift & 3) || c.num_mel_bins <= 0 || c.delta_order != 0 || c.use_cmvn || c.window < 0 ||
        c.window > 2 || (((uintptr_t)pcm) & 15) || (row_stride & 3) || row_stride < size + (F - 1) * shift || F > 0x7fffffffL ||
        ldo < c.num_mel_bins || out_bs < F * (long)ldo || !(div != 0.f))
        return hipErrorInvalidValue;
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    FbankPlan* plan = nullptr;
    {
        std::lock_guard<std::mutex> lock(g_mu);
        e = plan_for(c, dev, size, shift, &plan);
        if (e != hipSuccess) return e;
    }
    const FbankPlan& pl = *plan;  // (a plan is never rebuilt or freed: the pointer outlives the lock)
    const int N2 = 2 * pl.nbin;
    const int chunk = fbank_batch_chunk(nwin, F, pl.nbin, cap_bytes);
    if (!spec || spec_bytes < (size_t)chunk * F * N2 * sizeof(float)) return hipErrorInvalidValue;
    for (int w0 = 0; w0 < nwin; w0 += chunk) {
        const int nb = nwin - w0 < chunk ? nwin - w0 : chunk;
        GemmParams g{};
        g.A = pcm + (long)w0 * row_stride;
        g.lda = shift;  // overlapping rows: frame t of window w starts at sample w * row_stride + t * shift
        g.a_bs = row_stride;
        g.W = pl.dft;
        g.M = (int)F;
        g.N = N2;
        g.K = size;
        g.batches = nb;
        g.out32 = spec;
        g.ldo = N2;
        g.o_bs = F * N2;
        e = launch_gemm(F32, g, st);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL((mel_rows_kernel<POWER, LogFloorAffine>), dim3((unsigned)((long)nb * F)), dim3(128), pl.nbin * sizeof(float), st,
                           spec, pl.nbin, (int)F, pl.bank.bands, pl.bank.wts, pl.nmel, LogFloorAffine{FLT_EPSILON, add, div},
                           out + (long)w0 * out_bs, out_bs, (long)ldo, nullptr);
    }
    return hipGetLastError();
}

}  // namespace s3
