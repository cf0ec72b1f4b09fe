// spectral.h — the steps the fbank, log-mel, melspec and VGGish front ends share (spectral.hip): on the host, in float64 and rounded
// once, the window x zero-padded real DFT folded into a GEMM operand and the three mel banks, stored band by band; on the device the
// one-workgroup-per-frame power -> mel -> log kernel, the CMVN over time and the reflect padding in front of the overlapping-row GEMM.
#pragma once
#include <cfloat>
#include <vector>

#include "common.h"

namespace s3 {

// ---- host ----------------------------------------------------------------------------------------------------------------------
// (2 nbin) x N, nbin = nfft / 2 + 1: rows 0..nbin-1 win[i] cos a, the rest -win[i] sin a, a = 2 pi ((r i) mod nfft) / nfft
std::vector<float> fold_dft(const double* win, int N, int nfft);
// the same with a dense N x N pre-processing matrix D in front of the DFT (fbank: window . pre-emphasis . mean removal):
// row r, column j = sum_i cos a(r, i) D[i][j] (and -sin), accumulated over ascending i
std::vector<float> fold_dft_dense(const double* D, int N, int nfft);
std::vector<double> hann_periodic(int N);  // torch.hann_window(N)

// dense (nbin, nmel) banks over bins 0 .. Nyquist:
//   htk     torchaudio.functional.melscale_fbanks(nbin, f_min, f_max, nmel, 16000, norm = None, "htk"): triangles in Hz
//   kaldi   torchaudio.compliance.kaldi's (no VTLN): low 20 Hz, high = Nyquist, triangles in mel space; the Nyquist row is zero
//   vggish  mel_features.spectrogram_to_mel_matrix: triangles in mel space between np.linspace edges; the DC row is zero
std::vector<float> htk_bank(int nbin, double f_min, double f_max, int nmel);
std::vector<float> kaldi_bank(int nbin, int nmel, int sample_rate, int nfft);
std::vector<float> vggish_bank(int nbin, int nmel, double min_hz, double max_hz);
// dense -> bands[3][nmel] (first bin, bins, offset into wts) and every band's weights from its first to its last non-zero one
void sparsify(const std::vector<float>& dense, int nbin, int nmel, std::vector<int>& bands, std::vector<float>& wts);

template <class T>
hipError_t to_device(T** dst, const std::vector<T>& v) {
    hipError_t e = hipMalloc((void**)dst, v.size() * sizeof(T) + 16);
    if (e != hipSuccess) return e;
    return hipMemcpy(*dst, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice);
}
struct MelBank {  // sparsify's tables on the device
    int* bands = nullptr;
    float* wts = nullptr;
};
hipError_t upload_bank(MelBank& b, const std::vector<float>& dense, int nbin, int nmel);

// workgroup (f, b): mean / unbiased std (eps added to the std) of column f over rows [0, L) of x + b * x_bs, row pitch `pitch`, in
// place, in double; L = cnt ? cnt[b] clamped to [0, T] : T, and rows [L, T) are written as zeros
void launch_cmvn(float* x, const int* cnt, int T, int cols, int B, long pitch, long x_bs, float eps, hipStream_t st);

// ---- device --------------------------------------------------------------------------------------------------------------------
// band m's sum over its own bins, ascending, one fmaf per bin.  A bin outside the band has weight 0 and fmaf(pw, 0, acc) == acc
// for finite pw, so this is the dense sum's bits (a non-finite bin reaches only the bands that hold it)
__device__ __forceinline__ float mel_band_sum(const float* pw, const int* bands, const float* wts, int nmel, int m) {
    const int lo = bands[m], n = bands[nmel + m];
    const float* w = wts + bands[2 * nmel + m];
    float acc = 0.f;
    for (int i = 0; i < n; ++i) acc = fmaf(pw[lo + i], w[i], acc);
    return acc;
}

struct LogFloor {  // fbank
    float eps;
    __device__ float operator()(float acc) const { return logf(fmaxf(acc, eps)); }
};
struct LogAdd {  // log-mel, VGGish
    float eps;
    __device__ float operator()(float acc) const { return logf(acc + eps); }
};
struct LogAffine {  // melspec
    float mean, std_;
    __device__ float operator()(float acc) const { return (logf(acc + FLT_EPSILON) - mean) / std_; }
};

// What the mel bands sum.  The front ends' recorded bits hold two roundings of re^2 + im^2: both squares rounded, then added (fbank,
// log-mel, VGGish), and fmaf(re, re, fl(im^2)) (melspec).  Both are spelled out, so that the compiler's contraction chooses neither
enum Spectrum { POWER, POWER_FMA, MAGNITUDE };
__device__ __forceinline__ float sum_of_squares(float re, float im) {
#pragma clang fp contract(off)
    return re * re + im * im;
}

// one workgroup per row r of `spec` (re[nbin] | im[nbin]): the power (MAGNITUDE: its root) into LDS (nbin floats, dynamic), every
// band's sum, the epilogue; value (r / T, r % T, m) goes to out + (r / T) o_bs + (r % T) o_row + m.  power: null, or (rows, nbin)
template <Spectrum S, class Ep>
__global__ __launch_bounds__(128) void mel_rows_kernel(const float* spec, int nbin, int T, const int* bands, const float* wts, int nmel,
                                                       Ep ep, float* out, long o_bs, long o_row, float* power) {
    extern __shared__ float pw[];
    const long r = blockIdx.x, seg = r / T, t = r - seg * T;
    const float* s = spec + r * (2L * nbin);
    for (int k = threadIdx.x; k < nbin; k += 128) {
        const float re = s[k], im = s[nbin + k];
        const float v = S == POWER_FMA ? fmaf(re, re, im * im) : sum_of_squares(re, im);
        pw[k] = S == MAGNITUDE ? sqrtf(v) : v;
        if (power) power[r * nbin + k] = v;
    }
    __syncthreads();
    float* o = out + seg * o_bs + t * o_row;
    for (int m = threadIdx.x; m < nmel; m += 128) o[m] = ep(mel_band_sum(pw, bands, wts, nmel, m));
}

// sig[b][j], j < Lp: position p = j - half of row b's L samples reflect-padded by `half` about 0 and about L - 1 (L > half: one
// reflection), times scale[b] if given; samples at or past valid[b], and j at or past L + 2 half, are zeros.  Grid (Lp / 256, rows)
template <class Cnt>
__global__ __launch_bounds__(256) void reflect_pad_kernel(const float* const* ptrs, const Cnt* valid, const float* scale, long L,
                                                          int half, long Lp, float* sig) {
    const int b = blockIdx.y;
    const long j = (long)blockIdx.x * 256 + threadIdx.x;
    if (j >= Lp) return;
    long p = j - half;
    if (p < 0) p = -p;
    if (p >= L) p = 2 * (L - 1) - p;
    float v = 0.f;
    if (j < L + 2 * half && p >= 0 && p < valid[b]) v = scale ? ptrs[b][p] * scale[b] : ptrs[b][p];
    sig[(long)b * Lp + j] = v;
}

}  // namespace s3
