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

// kaldi's MFCC behind nmel log-mels: (nceps, nmel) row c = lifter_c M[:, c], M = create_dct(nmel, nmel, "ortho") with column 0
// sqrt(1 / nmel): M[n][c] = cos(pi / nmel (n + 0.5) c) sqrt(2 / nmel); lifter_c = 1 + 0.5 Q sin(pi c / Q) (Q = 0: 1)
std::vector<float> dct_lifter(int nceps, int nmel, double Q);
// the expert's rule behind the OnlinePreprocessor (baseline/expert.py:62-64): min(round(length * (T / first)), T), Python's round
long preproc_rows_kept(long length, long first, long T);

// fbank.hip's plan for these parameters on the current device, built on first use: the folded operand launch_fbank multiplies by,
// (2 nbin, size), and the kaldi bank of c.num_mel_bins bands
struct FbankParams;
struct FbankOperand {
    const float* dft;
    MelBank bank;
    int size, shift, nbin;
};
hipError_t fbank_operand(const FbankParams& c, FbankOperand* op);
// launch_fbank's deltas: columns [nmel, nmel (order + 1)) of out (T rows of pitch ldo) from columns [0, nmel)
void launch_fbank_delta(float* out, long T, int nmel, int ldo, int order, int delta_win, hipStream_t st);

// kaldi's raw log energy of T frames straight from the PCM (frame t = x[t shift .. t shift + size), size <= 1024, any 4-byte
// alignment), one wave per frame: energy[t] = max(log(max(sum (x - mean)^2, eps)), log_floor)
void launch_frame_energy(const float* x, long T, int size, int shift, float eps, float log_floor, float* energy, hipStream_t st);
// one workgroup per utterance: last[b] = 1 + the index of the last non-zero sample of x[b][0 .. n[b]), or `none` if all are zero
void launch_last_nonzero(const float* const* x, const long* n, int B, long none, long* last, hipStream_t st);
// one utterance: sig[j], j < Lp = x reflect-padded by `half` about 0 and about L - 1 (L > half), zeros behind L + 2 half
void launch_reflect_pad_one(const float* x, long L, int half, long Lp, float* sig, hipStream_t st);

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

struct ClampLog {  // stft_mag with log: log(clamp(|X|, lo))
    float lo;
    __device__ float operator()(float v) const { return logf(fmaxf(v, lo)); }
};
struct Identity {  // stft_mag without
    __device__ float operator()(float v) const { return v; }
};

// value (r, k) of the spectrum itself, no mel bank behind it: the epilogue of row r's power (MAGNITUDE: its root) at bin k, or
// bin0[r] at k = 0 when bin0 is given (kaldi's spectrogram puts the frame's log energy there)
template <Spectrum S, class Ep>
__device__ __forceinline__ float spectrum_value(const float* spec, int nbin, long r, int k, const Ep& ep, const float* bin0) {
    if (k == 0 && bin0) return bin0[r];
    const float* s = spec + r * (2L * nbin);
    const float v = sum_of_squares(s[k], s[nbin + k]);
    return ep(S == MAGNITUDE ? sqrtf(v) : v);
}

// `rows` rows of `spec` (re[nbin] | im[nbin]) -> out, rows x nbin CONTIGUOUS floats, per segment blockIdx.y (spec + y rows 2 nbin,
// bin0 + y rows, out + y o_bs).  HBM-bound: one read, one write.  nbin is odd (257, 201), so neither a row nor the segment starts
// on a 16-byte line: the segment is walked as one flat array — up to 3 single floats to the first 16-byte line of `out`, float4
// stores behind it (thread g owns the 4 values at head + 4 g, which may straddle two rows), up to 3 single floats at the end
template <Spectrum S, class Ep>
__global__ __launch_bounds__(256) void spectrum_rows_kernel(const float* spec, int nbin, long rows, Ep ep, const float* bin0, float* out,
                                                            long o_bs) {
    spec += (long)blockIdx.y * rows * 2 * nbin;
    if (bin0) bin0 += (long)blockIdx.y * rows;
    float* o = out + (long)blockIdx.y * o_bs;
    const long total = rows * nbin, g = (long)blockIdx.x * 256 + threadIdx.x;
    long head = (long)(((16 - ((uintptr_t)o & 15)) & 15) >> 2);
    if (head > total) head = total;
    const long nvec = (total - head) >> 2, tail = head + 4 * nvec;
    if (g < nvec) {
        const long i = head + 4 * g;
        long r = i / nbin;
        int k = (int)(i - r * nbin);
        float v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            v[j] = spectrum_value<S>(spec, nbin, r, k, ep, bin0);
            if (++k == nbin) k = 0, ++r;
        }
        *reinterpret_cast<float4*>(o + i) = make_float4(v[0], v[1], v[2], v[3]);
    }
    if (g < 3) {  // the unaligned ends, at most 3 floats each
        if (g < head) o[g] = spectrum_value<S>(spec, nbin, g / nbin, (int)(g % nbin), ep, bin0);
        const long i = tail + g;
        if (i < total) o[i] = spectrum_value<S>(spec, nbin, i / nbin, (int)(i % nbin), ep, bin0);
    }
}
// the same into rows of pitch o_row != nbin (deltas behind the bins): one workgroup per row, single floats
template <Spectrum S, class Ep>
__global__ __launch_bounds__(256) void spectrum_rows_pitched_kernel(const float* spec, int nbin, Ep ep, const float* bin0, float* out,
                                                                    long o_row) {
    const long r = blockIdx.x;
    for (int k = threadIdx.x; k < nbin; k += 256) out[r * o_row + k] = spectrum_value<S>(spec, nbin, r, k, ep, bin0);
}
template <Spectrum S, class Ep>
void launch_spectrum_rows(const float* spec, int nbin, long rows, int segs, Ep ep, const float* bin0, float* out, long o_row, long o_bs,
                          hipStream_t st) {
    if (o_row == nbin) {
        const long nvec = rows * nbin / 4 + 1;
        hipLaunchKernelGGL((spectrum_rows_kernel<S, Ep>), dim3((unsigned)((nvec + 255) / 256), segs), dim3(256), 0, st, spec, nbin, rows, ep,
                           bin0, out, o_bs);
    } else {
        for (int s = 0; s < segs; ++s)
            hipLaunchKernelGGL((spectrum_rows_pitched_kernel<S, Ep>), dim3((unsigned)rows), dim3(256), 0, st, spec + s * rows * 2L * nbin,
                               nbin, ep, bin0 ? bin0 + s * rows : nullptr, out + s * o_bs, o_row);
    }
}

// mel_rows_kernel with a DCT behind the log: the nmel log-mels of the frame stay in LDS (behind the nbin powers) and thread c sums
// dct[c][n] lm[n] over ascending n, one fmaf each — the same order for every frame.  dct: (nceps, nmel), the lifter folded in
template <class Ep>
__global__ __launch_bounds__(128) void mel_dct_rows_kernel(const float* spec, int nbin, const int* bands, const float* wts, int nmel,
                                                           Ep ep, const float* dct, int nceps, float* out, long o_row) {
    extern __shared__ float pw[];
    float* lm = pw + nbin;
    const long r = blockIdx.x;
    const float* s = spec + r * (2L * nbin);
    for (int k = threadIdx.x; k < nbin; k += 128) pw[k] = sum_of_squares(s[k], s[nbin + k]);
    __syncthreads();
    for (int m = threadIdx.x; m < nmel; m += 128) lm[m] = ep(mel_band_sum(pw, bands, wts, nmel, m));
    __syncthreads();
    for (int c = threadIdx.x; c < nceps; c += 128) {
        float acc = 0.f;
        for (int n = 0; n < nmel; ++n) acc = fmaf(lm[n], dct[c * nmel + n], acc);
        out[r * o_row + c] = acc;
    }
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
