// stem.hip — the stem of BYOL-S's ResNet (upstream/byol_s/byol_a/models/resnetish.py:196-203,279-282), exact fp32: Conv2d(1, 64, 7,
// stride 1, padding 3, no bias) -> BatchNorm2d (eval: a per-channel affine) -> ReLU -> MaxPool2d(3, 2, 1) on single-channel (H, 64)
// images (in this family H = time and W = mel: byol_s.hip transposes the taps before it packs them).
//
//   u[b][y][x][n] = relu( (sum_{ky} sum_{kx} img[b][y + ky - 3][x + kx - 3] * w[n][ky][kx]) * scale[n] + shift[n] )
//   out[b][yo][xo][n] = max over dy, dx in 0..2 of u[b][2 yo - 1 + dy][2 xo - 1 + dx][n], pixels outside the map left out
//
// K = 49 is not matrix work: VALU kernels in the manner of conv2d3x3_first_kernel, one thread per (output position, 4 channels), the
// 49 x 64 weights in LDS.  A thread walks the kernel rows in ascending order; per row it loads the run of input pixels its outputs
// share once and walks the 7 taps in ascending order, so every u is ONE fmaf chain in the order (ky, kx) whichever kernel computes it.
//   stem_fused_kernel:  thread = pooled pixel.  It walks the 9 operand rows under its window once; a row (9 input pixels) feeds kernel
//                       row r - dy of each of the three pool rows dy: 9 x 49 multiply-adds per pooled pixel where the map has 4 x 49,
//                       2.25 x, and the un-pooled map (64 x the input) is never written.  The operand's border is 4 wide: the
//                       un-pooled row / column -1 of a window at the edge is computed from zeros and left out of the max.
//   stem_map_kernel + stem_pool_kernel: the split form.  Thread = 4 neighbouring un-pooled pixels of a row (10 input pixels per kernel
//                       row), written behind the ReLU into a map with a zero border; the pool kernel reads its 3 x 3 window there.
// Every u is at least +0 behind the ReLU (negative zero is written as +0) or a NaN, so the map's zero border stands for the -inf padding
// of nn.MaxPool2d, every window holds at least one real pixel, and max is order-free: the two forms agree bit for bit.
#include "kernels.h"

namespace s3 {

namespace {

constexpr int SW = 64, SN = 64, SK = 7, SB = 4;  // mel columns, channels, taps per side, border of the operand
constexpr int PITCH = SW + 2 * SB;

__device__ __forceinline__ float relu0(float v) { return (v > 0.f || v != v) ? v : 0.f; }  // -0 -> +0; a NaN stays a NaN
__device__ __forceinline__ float pmax(float a, float b) { return (a > b || a != a) ? a : b; }  // a NaN stays a NaN
__device__ __forceinline__ float4 epi(const float4& a, const float4& s, const float4& t) {
    return make_float4(relu0(fmaf(a.x, s.x, t.x)), relu0(fmaf(a.y, s.y, t.y)), relu0(fmaf(a.z, s.z, t.z)), relu0(fmaf(a.w, s.w, t.w)));
}
__device__ __forceinline__ float4 pmax4(const float4& a, const float4& b) {
    return make_float4(pmax(a.x, b.x), pmax(a.y, b.y), pmax(a.z, b.z), pmax(a.w, b.w));
}

__device__ __forceinline__ void load_weights(float* wl, const float* Wt) {
    for (int i = threadIdx.x; i < SK * SK * SN / 4; i += 256) ((float4*)wl)[i] = ((const float4*)Wt)[i];
    __syncthreads();
}

// NX neighbouring un-pooled pixels of one row: `row0` points at the operand pixel under tap (0, 0) of the first one
template <int NX>
__device__ __forceinline__ void conv_row(const float* row0, const float* wl, int g, float4 (&a)[NX]) {
#pragma unroll
    for (int i = 0; i < NX; ++i) a[i] = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int ky = 0; ky < SK; ++ky) {
        float in[NX + SK - 1];
#pragma unroll
        for (int c = 0; c < NX + SK - 1; ++c) in[c] = row0[ky * PITCH + c];
#pragma unroll
        for (int kx = 0; kx < SK; ++kx) {
            const float4 w = *(const float4*)(wl + (ky * SK + kx) * SN + g * 4);
#pragma unroll
            for (int i = 0; i < NX; ++i) {
                const float v = in[i + kx];
                a[i].x = fmaf(v, w.x, a[i].x); a[i].y = fmaf(v, w.y, a[i].y); a[i].z = fmaf(v, w.z, a[i].z); a[i].w = fmaf(v, w.w, a[i].w);
            }
        }
    }
}

__global__ __launch_bounds__(256) void stem_fused_kernel(StemParams p) {
    __shared__ __attribute__((aligned(16))) float wl[SK * SK * SN];
    load_weights(wl, p.Wt);
    const int Hp = (p.H - 1) / 2 + 1;
    const long items = (long)p.B * Hp * (SW / 2) * (SN / 4);
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= items) return;
    const int g = (int)(idx & 15);
    const long pix = idx >> 4;
    const int xo = (int)(pix & 31);
    const int yo = (int)((pix >> 5) % Hp);
    const int b = (int)((pix >> 5) / Hp);
    const float4 s4 = *(const float4*)(p.scale + g * 4), t4 = *(const float4*)(p.shift + g * 4);
    // un-pooled pixel (y, x) reads operand rows y + 1 .. y + 7 and columns x + 1 .. x + 7 (border 4); the window starts at (2 yo - 1, 2 xo - 1)
    const float* img = p.src + (long)b * p.src_bs + (long)(2 * yo) * PITCH + 2 * xo;
    // the 9 operand rows under the window, one at a time: row r is kernel row r - dy of pool row dy, so every un-pooled pixel still
    // meets its kernel rows in ascending order (and the 49 weights are read as they are used, never held in registers)
    float4 a[3][3];
#pragma unroll
    for (int dy = 0; dy < 3; ++dy)
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) a[dy][dx] = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 1
    for (int r = 0; r < SK + 2; ++r) {
        float in[SK + 2];
#pragma unroll
        for (int c = 0; c < SK + 2; ++c) in[c] = img[r * PITCH + c];
#pragma unroll
        for (int dy = 0; dy < 3; ++dy) {
            const int ky = r - dy;
            if (ky < 0 || ky >= SK) continue;
#pragma unroll
            for (int kx = 0; kx < SK; ++kx) {
                const float4 w = *(const float4*)(wl + (ky * SK + kx) * SN + g * 4);
#pragma unroll
                for (int dx = 0; dx < 3; ++dx) {
                    const float v = in[dx + kx];
                    a[dy][dx].x = fmaf(v, w.x, a[dy][dx].x); a[dy][dx].y = fmaf(v, w.y, a[dy][dx].y);
                    a[dy][dx].z = fmaf(v, w.z, a[dy][dx].z); a[dy][dx].w = fmaf(v, w.w, a[dy][dx].w);
                }
            }
        }
    }
    float4 out = make_float4(0.f, 0.f, 0.f, 0.f);
    bool have = false;
#pragma unroll
    for (int dy = 0; dy < 3; ++dy)
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) {
            const int y = 2 * yo - 1 + dy, x = 2 * xo - 1 + dx;
            if (y < 0 || y >= p.H || x < 0 || x >= SW) continue;
            const float4 v = epi(a[dy][dx], s4, t4);
            out = have ? pmax4(out, v) : v;
            have = true;
        }
    *(float4*)(p.dst + (long)b * p.dst_bs + ((long)(yo + 1) * (SW / 2 + 2) + xo + 1) * SN + g * 4) = out;
}

__global__ __launch_bounds__(256) void stem_map_kernel(StemParams p) {
    __shared__ __attribute__((aligned(16))) float wl[SK * SK * SN];
    load_weights(wl, p.Wt);
    const long items = (long)p.B * p.H * (SW / 4) * (SN / 4);
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= items) return;
    const int g = (int)(idx & 15);
    const long q = idx >> 4;
    const int x = (int)(q & 15) * 4;
    const int y = (int)((q >> 4) % p.H);
    const int b = (int)((q >> 4) / p.H);
    const float4 s4 = *(const float4*)(p.scale + g * 4), t4 = *(const float4*)(p.shift + g * 4);
    float4 a[4];
    conv_row<4>(p.src + (long)b * p.src_bs + (long)(y + 1) * PITCH + x + 1, wl, g, a);
    float* o = p.map + (long)b * p.map_bs + ((long)(y + 1) * (SW + 2) + x + 1) * SN + g * 4;
#pragma unroll
    for (int i = 0; i < 4; ++i) *(float4*)(o + i * SN) = epi(a[i], s4, t4);
}

__global__ __launch_bounds__(256) void stem_pool_kernel(StemParams p) {
    const int Hp = (p.H - 1) / 2 + 1;
    const long items = (long)p.B * Hp * (SW / 2) * (SN / 4);
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= items) return;
    const int g = (int)(idx & 15);
    const long pix = idx >> 4;
    const int xo = (int)(pix & 31);
    const int yo = (int)((pix >> 5) % Hp);
    const int b = (int)((pix >> 5) / Hp);
    // un-pooled pixel (y, x) is bordered pixel (y + 1, x + 1) of the map: the window starts at bordered (2 yo, 2 xo)
    const float* m = p.map + (long)b * p.map_bs + ((long)(2 * yo) * (SW + 2) + 2 * xo) * SN + g * 4;
    float4 out = *(const float4*)m;
#pragma unroll
    for (int t = 1; t < 9; ++t) out = pmax4(out, *(const float4*)(m + ((long)(t / 3) * (SW + 2) + t % 3) * SN));
    *(float4*)(p.dst + (long)b * p.dst_bs + ((long)(yo + 1) * (SW / 2 + 2) + xo + 1) * SN + g * 4) = out;
}

}  // namespace

void pack_stem7x7(const float* w, std::vector<float>& out) {
    out.assign((size_t)SK * SK * SN, 0.f);
    for (int n = 0; n < SN; ++n)
        for (int t = 0; t < SK * SK; ++t) out[(size_t)t * SN + n] = w[(size_t)n * SK * SK + t];
}

const char* stem_refusal(const StemParams& p) {
    if (!p.src || !p.Wt || !p.scale || !p.shift || !p.dst) return "null operand";
    if (p.B < 1 || p.H < 1) return "bad shape";
    if (p.fused < 0 || p.fused > 1) return "fused must be 0 or 1";
    if (!p.fused && !p.map) return "the split form needs its map";
    const long Hp = (p.H - 1) / 2 + 1;
    if (p.src_bs < (long)(p.H + 2 * SB) * PITCH) return "src example stride is smaller than one bordered image";
    if (p.B > 1 && p.dst_bs < (Hp + 2) * (SW / 2 + 2) * SN) return "dst example stride is smaller than one bordered image";
    if (!p.fused && p.B > 1 && p.map_bs < (long)(p.H + 2) * (SW + 2) * SN) return "map example stride is smaller than one bordered image";
    if ((p.dst_bs | p.map_bs) & 3) return "dst and map example strides must be multiples of 4 floats (vector stores)";
    if (((uintptr_t)p.Wt | (uintptr_t)p.scale | (uintptr_t)p.shift | (uintptr_t)p.dst | (uintptr_t)p.map) & 15) return "operands must be 16-byte aligned";
    if ((uintptr_t)p.src & 3) return "operands must be 4-byte aligned";
    if ((long)p.B * p.H * 256 > 0x7fffffffL * 64L) return "too many pixels";
    return nullptr;
}

hipError_t launch_stem(const StemParams& p, hipStream_t stream) {
    if (stem_refusal(p)) return hipErrorInvalidValue;
    const long Hp = (p.H - 1) / 2 + 1;
    const long pooled = (long)p.B * Hp * (SW / 2) * (SN / 4);
    if (p.fused) {
        hipLaunchKernelGGL(stem_fused_kernel, dim3((unsigned)((pooled + 255) / 256)), dim3(256), 0, stream, p);
        return hipGetLastError();
    }
    const long items = (long)p.B * p.H * (SW / 4) * (SN / 4);
    hipLaunchKernelGGL(stem_map_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, stream, p);
    hipLaunchKernelGGL(stem_pool_kernel, dim3((unsigned)((pooled + 255) / 256)), dim3(256), 0, stream, p);
    return hipGetLastError();
}

}  // namespace s3
