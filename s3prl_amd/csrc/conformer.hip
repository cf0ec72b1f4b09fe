// conformer.hip — the row passes of the wav2vec 2.0 Conformer block (wav2vec2_model.py:313-393,25-71, 523-578) that are not
// GEMMs, attention or LayerNorm:
//   conformer_conv_kernel  GLU -> depthwise Conv1d over time (zero padding (k-1)/2 per utterance) -> BatchNorm (eval, folded
//                          into the taps and a per-channel shift at s3enc_create) -> swish, on pointwise_conv1's (M, 2D) output;
//                          writes pointwise_conv2's (M, D) operand
//   rope_kernel            rot(x) = x * cos + rotate_half(x) * sin per 64-wide head chunk (RotaryPositionalEmbedding,
//                          apply_rotary_pos_emb), the operand of the q | k projections
#include "kernels.h"

namespace s3 {
namespace {

constexpr int CV_C = 64;    // channels per workgroup (16 lanes x float4)
constexpr int CV_T = 128;   // output frames per workgroup (16 frame groups x 8)
constexpr int CV_F = 8;     // output frames per thread

__device__ __forceinline__ float swishf(float x) { return x / (1.f + __expf(-x)); }

// One workgroup: CV_C channels x CV_T frames of one utterance.  The GLU'd input window (CV_T + K - 1 frames, zero outside
// [0, T)) is staged once in LDS; a thread owns 4 channels x 8 consecutive frames and runs the K taps over them (one tap float4
// and 8 window float4 reads per 32 FMAs; every ds_read_b128 lane group reads 16 different channel quads: conflict-free).
__global__ __launch_bounds__(256) void conformer_conv_kernel(ConformerConvParams p) {
    extern __shared__ __attribute__((aligned(16))) float cv_lds[];
    const int K = p.K, pad = (K - 1) / 2, D = p.D;
    const int WIN = CV_T + K - 1;
    float* xs = cv_lds;                  // [WIN][CV_C]
    float* ws = cv_lds + WIN * CV_C;     // [K][CV_C]
    const int c0 = blockIdx.x * CV_C, t0 = blockIdx.y * CV_T, b = blockIdx.z;
    const int tid = threadIdx.x;
    const long row0 = (long)b * p.T;
    for (int i = tid; i < WIN * (CV_C / 4); i += 256) {
        const int r = i / (CV_C / 4), q = i % (CV_C / 4);
        const int t = t0 - pad + r;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (t >= 0 && t < p.T) {
            const float* src = p.x + (row0 + t) * (2L * D) + c0 + 4 * q;
            const float4 a = *(const float4*)src;
            const float4 g = *(const float4*)(src + D);
            v = make_float4(a.x / (1.f + __expf(-g.x)), a.y / (1.f + __expf(-g.y)), a.z / (1.f + __expf(-g.z)),
                            a.w / (1.f + __expf(-g.w)));
        }
        *(float4*)(xs + r * CV_C + 4 * q) = v;
    }
    for (int i = tid; i < K * (CV_C / 4); i += 256) {
        const int k = i / (CV_C / 4), q = i % (CV_C / 4);
        float4 w;
        w.x = p.taps[(long)(c0 + 4 * q) * K + k];
        w.y = p.taps[(long)(c0 + 4 * q + 1) * K + k];
        w.z = p.taps[(long)(c0 + 4 * q + 2) * K + k];
        w.w = p.taps[(long)(c0 + 4 * q + 3) * K + k];
        *(float4*)(ws + k * CV_C + 4 * q) = w;
    }
    __syncthreads();
    const int cq = tid & 15, fg = tid >> 4;
    float4 acc[CV_F];
#pragma unroll
    for (int f = 0; f < CV_F; ++f) acc[f] = make_float4(0.f, 0.f, 0.f, 0.f);
    const float* xb = xs + fg * CV_F * CV_C + 4 * cq;
    for (int k = 0; k < K; ++k) {
        const float4 w = *(const float4*)(ws + k * CV_C + 4 * cq);
#pragma unroll
        for (int f = 0; f < CV_F; ++f) {
            const float4 x = *(const float4*)(xb + (f + k) * CV_C);
            acc[f].x = fmaf(w.x, x.x, acc[f].x);
            acc[f].y = fmaf(w.y, x.y, acc[f].y);
            acc[f].z = fmaf(w.z, x.z, acc[f].z);
            acc[f].w = fmaf(w.w, x.w, acc[f].w);
        }
    }
    const float4 sh = *(const float4*)(p.shift + c0 + 4 * cq);
#pragma unroll
    for (int f = 0; f < CV_F; ++f) {
        const int t = t0 + fg * CV_F + f;
        if (t >= p.T) break;
        float4 v = acc[f];
        v.x = swishf(v.x + sh.x);
        v.y = swishf(v.y + sh.y);
        v.z = swishf(v.z + sh.z);
        v.w = swishf(v.w + sh.w);
        *(float4*)(p.out + (row0 + t) * D + c0 + 4 * cq) = v;
    }
}

// rot(x) for the rows of (B, T, D): position t = row % T; table[t] = {cos[0..31], sin[0..31]} (emb = cat(freqs, freqs), so the
// second half of each head chunk uses the same 32 angles).  The reference's operation order: x * cos + rotate_half(x) * sin,
// rotate_half = cat(-x2, x1), each product rounded before the sum.
__global__ __launch_bounds__(256) void rope_kernel(const float* __restrict__ x, const float* __restrict__ table, long rows, int T,
                                                    int D, float* __restrict__ out) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;  // one float4 of the output
    const long n4 = rows * (D / 4);
    if (i >= n4) return;
    const long row = i / (D / 4);
    const int d = (int)(i % (D / 4)) * 4;
    const int hd = d & 63, hb = d - hd;
    const int t = (int)(row % T);
    const float* tc = table + (long)t * 64;
    const float* xr = x + row * D + hb;
    const float4 v = *(const float4*)(xr + hd);
    const int j = hd & 31;
    const float4 c = *(const float4*)(tc + j);
    const float4 s = *(const float4*)(tc + 32 + j);
    float4 o;
    if (hd < 32) {  // x1 * cos - x2 * sin
        const float4 u = *(const float4*)(xr + hd + 32);
        o = make_float4(__fadd_rn(__fmul_rn(v.x, c.x), __fmul_rn(-u.x, s.x)), __fadd_rn(__fmul_rn(v.y, c.y), __fmul_rn(-u.y, s.y)),
                        __fadd_rn(__fmul_rn(v.z, c.z), __fmul_rn(-u.z, s.z)), __fadd_rn(__fmul_rn(v.w, c.w), __fmul_rn(-u.w, s.w)));
    } else {        // x2 * cos + x1 * sin
        const float4 u = *(const float4*)(xr + hd - 32);
        o = make_float4(__fadd_rn(__fmul_rn(v.x, c.x), __fmul_rn(u.x, s.x)), __fadd_rn(__fmul_rn(v.y, c.y), __fmul_rn(u.y, s.y)),
                        __fadd_rn(__fmul_rn(v.z, c.z), __fmul_rn(u.z, s.z)), __fadd_rn(__fmul_rn(v.w, c.w), __fmul_rn(u.w, s.w)));
    }
    *(float4*)(out + row * D + d) = o;
}

}  // namespace

hipError_t launch_conformer_conv(const ConformerConvParams& p, hipStream_t s) {
    if (p.B <= 0 || p.T <= 0) return hipSuccess;
    if (p.D % CV_C || p.K < 1 || p.K > 63 || !(p.K & 1)) return hipErrorInvalidValue;
    if (((uintptr_t)p.x | (uintptr_t)p.out | (uintptr_t)p.shift) & 15) return hipErrorInvalidValue;
    const int lds = ((CV_T + p.K - 1) * CV_C + p.K * CV_C) * (int)sizeof(float);  // <= 63.5 KiB at K = 63
    hipError_t e = ensure_dynamic_lds<conformer_conv_kernel>(lds);
    if (e != hipSuccess) return e;
    dim3 grid((unsigned)(p.D / CV_C), (unsigned)((p.T + CV_T - 1) / CV_T), (unsigned)p.B);
    hipLaunchKernelGGL(conformer_conv_kernel, grid, dim3(256), lds, s, p);
    return hipGetLastError();
}

hipError_t launch_rope(const float* x, const float* table, long rows, int T, int D, float* out, hipStream_t s) {
    if (rows <= 0) return hipSuccess;
    if (D % 64 || T <= 0 || (((uintptr_t)x | (uintptr_t)out | (uintptr_t)table) & 15)) return hipErrorInvalidValue;
    const long n4 = rows * (D / 4);
    hipLaunchKernelGGL(rope_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, s, x, table, rows, T, D, out);
    return hipGetLastError();
}

}  // namespace s3
