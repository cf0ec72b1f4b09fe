// spectral.hip — the host builders and the CMVN kernel of spectral.h.  Everything here is float64 on the host and rounded to fp32
// once; the expressions and their order are the ones the front ends' recorded bits were computed with (tests/golden/frontends).
#include <cmath>

#include "spectral.h"

namespace s3 {

namespace {

// c[i] = cos a, s[i] = -sin a of row r: a = 2 pi ((r i) mod nfft) / nfft
void dft_row(int r, int N, int nfft, double* c, double* s) {
    for (int i = 0; i < N; ++i) {
        const double a = 2.0 * M_PI * (double)((long)r * i % nfft) / nfft;
        c[i] = std::cos(a);
        s[i] = -std::sin(a);
    }
}

__global__ __launch_bounds__(256) void cmvn_kernel(float* x, const int* cnt, int T, long pitch, long x_bs, float eps) {
    __shared__ double red[4];
    const int f = blockIdx.x, b = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float* xb = x + (long)b * x_bs + f;
    int L = cnt ? cnt[b] : T;
    L = L < 0 ? 0 : (L > T ? T : L);
    auto block_sum = [&](double v) {
        v = wave_sum_d(v);
        __syncthreads();
        if (lane == 0) red[wave] = v;
        __syncthreads();
        return red[0] + red[1] + red[2] + red[3];
    };
    double s = 0.0;
    for (int t = threadIdx.x; t < L; t += 256) s += xb[t * pitch];
    const double mean = block_sum(s) / (double)L;
    double q = 0.0;
    for (int t = threadIdx.x; t < L; t += 256) {
        const double d = xb[t * pitch] - mean;
        q += d * d;
    }
    const double var = block_sum(q) / (double)(L - 1);  // unbiased (torch.std); one row -> nan like torch (the callers refuse it)
    const float inv = (float)(1.0 / ((double)eps + sqrt(var)));
    for (int t = threadIdx.x; t < T; t += 256) xb[t * pitch] = t < L ? (float)(xb[t * pitch] - mean) * inv : 0.f;
}

// one wave per frame: the mean, then the squared deviations of the samples held in registers (never sum x^2 - (sum x)^2 / N),
// max(log(max(e, eps)), log_floor)
__global__ __launch_bounds__(256) void frame_energy_kernel(const float* x, long T, int size, int shift, float eps, float log_floor,
                                                           float* energy) {
    const long t = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (t >= T) return;
    const float* f = x + t * shift;
    float v[16], s = 0.f;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const int i = lane + 64 * j;
        v[j] = i < size ? f[i] : 0.f;
        s += v[j];
    }
    const float mean = wave_sum(s) / (float)size;
    float q = 0.f;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const float d = lane + 64 * j < size ? v[j] - mean : 0.f;
        q = fmaf(d, d, q);
    }
    q = wave_sum(q);
    if (lane == 0) energy[t] = fmaxf(logf(fmaxf(q, eps)), log_floor);
}

// one workgroup per utterance: last[b] = 1 + the index of the last non-zero sample of x[b][0 .. n[b]), or `none` if all are zero
__global__ __launch_bounds__(1024) void last_nonzero_kernel(const float* const* x, const long* n, long none, long* last) {
    __shared__ long red[16];
    const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    long hi = 0;
    for (long i = threadIdx.x; i < n[b]; i += 1024)
        if (x[b][i] != 0.f) hi = i + 1;  // ascending i: the thread's last hit is its largest
    for (int o = 32; o; o >>= 1) {
        const long other = __shfl_xor(hi, o);
        hi = other > hi ? other : hi;
    }
    if (lane == 0) red[wave] = hi;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 16; ++w) hi = red[w] > hi ? red[w] : hi;
        last[b] = hi ? hi : none;
    }
}

// one utterance: sig[j], j < Lp = x reflect-padded by `half` about 0 and about L - 1 (L > half), zeros behind L + 2 half
__global__ __launch_bounds__(256) void reflect_pad_one_kernel(const float* x, long L, int half, long Lp, float* sig) {
    const long j = (long)blockIdx.x * 256 + threadIdx.x;
    if (j >= Lp) return;
    long p = j - half;
    if (p < 0) p = -p;
    if (p >= L) p = 2 * (L - 1) - p;
    sig[j] = j < L + 2 * half && p >= 0 && p < L ? x[p] : 0.f;
}

}  // namespace

std::vector<float> fold_dft(const double* win, int N, int nfft) {
    const int nb = nfft / 2 + 1;
    std::vector<float> M((size_t)2 * nb * N);
    std::vector<double> c(N), s(N);
    for (int r = 0; r < nb; ++r) {
        dft_row(r, N, nfft, c.data(), s.data());
        for (int i = 0; i < N; ++i) {
            M[(size_t)r * N + i] = (float)(win[i] * c[i]);
            M[(size_t)(nb + r) * N + i] = (float)(win[i] * s[i]);
        }
    }
    return M;
}

std::vector<float> fold_dft_dense(const double* D, int N, int nfft) {
    const int nb = nfft / 2 + 1;
    std::vector<float> M((size_t)2 * nb * N);
    std::vector<double> c(N), s(N);
    for (int r = 0; r < nb; ++r) {
        dft_row(r, N, nfft, c.data(), s.data());
        for (int j = 0; j < N; ++j) {
            double re = 0.0, im = 0.0;
            for (int i = 0; i < N; ++i) {
                re += c[i] * D[(size_t)i * N + j];
                im += s[i] * D[(size_t)i * N + j];
            }
            M[(size_t)r * N + j] = (float)re;
            M[(size_t)(nb + r) * N + j] = (float)im;
        }
    }
    return M;
}

std::vector<double> hann_periodic(int N) {
    std::vector<double> w(N);
    for (int i = 0; i < N; ++i) w[i] = 0.5 - 0.5 * std::cos(2.0 * M_PI * i / N);
    return w;
}

std::vector<float> htk_bank(int nbin, double f_min, double f_max, int nmel) {
    auto hz2mel = [](double f) { return 2595.0 * std::log10(1.0 + f / 700.0); };
    auto mel2hz = [](double m) { return 700.0 * (std::pow(10.0, m / 2595.0) - 1.0); };
    const double m_lo = hz2mel(f_min), m_hi = hz2mel(f_max);
    std::vector<double> fpt(nmel + 2);
    for (int i = 0; i < nmel + 2; ++i) fpt[i] = mel2hz(m_lo + (m_hi - m_lo) * i / (nmel + 1));
    std::vector<float> bT((size_t)nbin * nmel);
    for (int k = 0; k < nbin; ++k) {
        const double f = 8000.0 * k / (nbin - 1);
        for (int m = 0; m < nmel; ++m) {
            const double down = (f - fpt[m]) / (fpt[m + 1] - fpt[m]), up = (fpt[m + 2] - f) / (fpt[m + 2] - fpt[m + 1]);
            bT[(size_t)k * nmel + m] = (float)std::fmax(0.0, std::fmin(down, up));
        }
    }
    return bT;
}

std::vector<float> kaldi_bank(int nbin, int nmel, int sample_rate, int nfft) {
    std::vector<float> bT((size_t)nbin * nmel, 0.f);
    auto mel = [](double f) { return 1127.0 * std::log(1.0 + f / 700.0); };
    const double lo = mel(20.0), hi = mel(0.5 * sample_rate), delta = (hi - lo) / (nmel + 1);
    const double width = (double)sample_rate / nfft;
    for (int b = 0; b < nmel; ++b) {
        const double left = lo + b * delta, center = left + delta, right = center + delta;
        for (int k = 0; k < nbin - 1; ++k) {
            const double m = mel(width * k);
            const double up = (m - left) / (center - left), down = (right - m) / (right - center);
            bT[(size_t)k * nmel + b] = (float)std::fmax(0.0, std::fmin(up, down));
        }
    }
    return bT;
}

std::vector<float> vggish_bank(int nbin, int nmel, double min_hz, double max_hz) {
    std::vector<float> mT((size_t)nbin * nmel, 0.f);
    auto mel = [](double f) { return 1127.0 * std::log(1.0 + f / 700.0); };
    const double lo = mel(min_hz), hi = mel(max_hz);
    for (int b = 0; b < nmel; ++b) {
        // np.linspace(lo, hi, nmel + 2)[b : b + 3]
        const double step = (hi - lo) / (nmel + 1);
        const double left = lo + b * step, center = lo + (b + 1) * step, right = b + 2 == nmel + 1 ? hi : lo + (b + 2) * step;
        for (int k = 1; k < nbin; ++k) {
            const double m = mel(8000.0 * k / (nbin - 1));
            const double up = (m - left) / (center - left), down = (right - m) / (right - center);
            mT[(size_t)k * nmel + b] = (float)std::fmax(0.0, std::fmin(up, down));
        }
    }
    return mT;
}

void sparsify(const std::vector<float>& dense, int nbin, int nmel, std::vector<int>& bands, std::vector<float>& wts) {
    bands.assign(3 * (size_t)nmel, 0);
    wts.clear();
    for (int m = 0; m < nmel; ++m) {
        int lo = -1, hi = -1;
        for (int k = 0; k < nbin; ++k)
            if (dense[(size_t)k * nmel + m] != 0.f) {
                if (lo < 0) lo = k;
                hi = k;
            }
        bands[m] = lo < 0 ? 0 : lo;
        bands[nmel + m] = lo < 0 ? 0 : hi - lo + 1;
        bands[2 * nmel + m] = (int)wts.size();
        for (int k = bands[m]; k < bands[m] + bands[nmel + m]; ++k) wts.push_back(dense[(size_t)k * nmel + m]);
    }
}

hipError_t upload_bank(MelBank& b, const std::vector<float>& dense, int nbin, int nmel) {
    std::vector<int> bands;
    std::vector<float> wts;
    sparsify(dense, nbin, nmel, bands, wts);
    const hipError_t e = to_device(&b.bands, bands);
    return e != hipSuccess ? e : to_device(&b.wts, wts);
}

std::vector<float> dct_lifter(int nceps, int nmel, double Q) {
    std::vector<float> D((size_t)nceps * nmel);
    for (int c = 0; c < nceps; ++c) {
        const double lift = Q > 0.0 ? 1.0 + 0.5 * Q * std::sin(M_PI * c / Q) : 1.0;
        for (int n = 0; n < nmel; ++n) {
            const double m = c == 0 ? std::sqrt(1.0 / nmel) : std::cos(M_PI / nmel * (n + 0.5) * c) * std::sqrt(2.0 / nmel);
            D[(size_t)c * nmel + n] = (float)(lift * m);
        }
    }
    return D;
}

long preproc_rows_kept(long length, long first, long T) {
    const double ratio = (double)T / (double)first;
    const long v = (long)std::nearbyint((double)length * ratio);  // Python's round(): half to even, the default rounding mode
    return v < 0 ? 0 : (v > T ? T : v);
}

void launch_frame_energy(const float* x, long T, int size, int shift, float eps, float log_floor, float* energy, hipStream_t st) {
    hipLaunchKernelGGL(frame_energy_kernel, dim3((unsigned)((T + 3) / 4)), dim3(256), 0, st, x, T, size, shift, eps, log_floor, energy);
}

void launch_last_nonzero(const float* const* x, const long* n, int B, long none, long* last, hipStream_t st) {
    hipLaunchKernelGGL(last_nonzero_kernel, dim3(B), dim3(1024), 0, st, x, n, none, last);
}

void launch_reflect_pad_one(const float* x, long L, int half, long Lp, float* sig, hipStream_t st) {
    hipLaunchKernelGGL(reflect_pad_one_kernel, dim3((unsigned)((Lp + 255) / 256)), dim3(256), 0, st, x, L, half, Lp, sig);
}

void launch_cmvn(float* x, const int* cnt, int T, int cols, int B, long pitch, long x_bs, float eps, hipStream_t st) {
    hipLaunchKernelGGL(cmvn_kernel, dim3(cols, B), dim3(256), 0, st, x, cnt, T, pitch, x_bs, eps);
}

}  // namespace s3
