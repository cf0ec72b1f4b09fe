// conv2d.hip — exact-fp32 stride-1 3 x 3 Conv2d(C, N, padding = 1) over channel-last images with bias -> ReLU -> optional 2 x 2 /
// stride-2 max-pool in the epilogue: VGGish's `features` stack (upstream/vggish/vggish.py:18-41,123-133).
//
//   v[b][y][x][n] = act( sum_{ky} sum_{kx} sum_c img[b][y + ky][x + kx][c] * w[n][c][ky][kx] + bias[n] )
//   pool: out[b][y'][x'][n] = max over the 2 x 2 window of v;  else out = v
//
// Operand geometry, the 2-D form of cpc.hip's / convtaps.hip's bordered rows: every example is an (H + 2) x (W + 2) x C image whose
// outermost pixels are zeros, so a tap that hangs over an edge reads zeros and never a neighbouring example.  For a fixed kernel
// row ky the three taps of an output pixel are ONE contiguous run of 3 C floats of A; the K walk is three such runs, and between
// two runs the A offset jumps by (W + 2 - 3) C floats while the W offset does not: the weights are packed (N, 9 C) with k = (ky * 3
// + kx) * C + c.  C is a multiple of 16: a tap is a whole number of 64-byte K steps.
//
// The GEMM's M axis is the pixels of ALL examples, m = b * H * W + p: a tile spans examples, so the late layers (96 or 24 pixels per
// example) fill their tiles like the early ones and only the launch's last tile is ragged.  Under `pool` an example's pixels are
// enumerated pool-window-major, p = 4 * (wy * W / 2 + wx) + 2 * dy + dx: the four partners of a window are four consecutive rows,
// aligned to 4, which the 32 x 32 MFMA's C/D map (row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)) keeps in one lane's registers 4 g ..
// 4 g + 3, and in the epilogue's LDS transpose in four consecutive rows.  The un-pooled activation is never written to memory.
//
// Schedule: convtaps.hip's (v_mfma_f32_32x32x2_f32 on 64-byte K steps, LDS-DMA staging of lane-linear planes with the XOR swizzle
// applied to the source slot, two register sets of fragments around the step's one barrier) on a (128 | 64) x 128 tile.  Per output
// element the order is fixed — kernel rows ascending, taps ascending, the tile GEMM's order inside a step — so an example's bits
// depend neither on B, nor on its place in the batch, nor on the tile height or the n-tile; max is order-free.
//
// Epilogue, one pass, plain vector stores into the INTERIOR of the next layer's bordered buffer (border width dst_pad, pixel pitch
// ld_dst; dst_pad = 0 gives a plain contiguous (B, H', W', N) tensor — VGGish's flatten order, the first Linear's A operand).
//
// BYOL-A's additions (upstream/byol_a/byol_a.py:95-107), as template parameters of separate instantiations — the ones above are
// VGGish's as they were.  EXT: the epilogue is act(acc * scale[n] + shift[n]), an eval-mode BatchNorm2d behind the conv (the host
// folds the conv bias into the shift; (1, bias) is bit for bit acc + bias), and under pool_floor an example's M extent is 4 (H / 2)
// (W / 2): odd maps pool as nn.MaxPool2d(2, 2) does and the dropped last row / column is never enumerated, while the operand's row
// pitch and the kernel-row jump keep the true W.  WN = 1: a 64-wide n-tile for Cout <= 64 with all four waves along M.
//
// BYOL-S's additions (upstream/byol_s/byol_a/models/resnetish.py:23-102), the GEN instantiations: k x k taps, k = 3 or 1, at
// padding (k - 1) / 2 and stride 1 or 2 over the same (H + 2) x (W + 2) operand, and a residual added behind the affine and before
// the activation.  The K walk is k runs of k C floats (k = 1: one run of C floats of the pixel's own interior position), the jump
// between two runs is (W + 2 - k) C floats, and only a row's first A offset knows the stride: output pixel (y, x) starts at bordered
// pixel (y s + 1 - p, x s + 1 - p).  The M axis is the Ho x Wo OUTPUT pixels of all examples.  k = 3, s = 1 without a residual is bit
// for bit the EXT instantiation; no pooling.
//
// conv2d3x3_first_kernel is the C = 1 layer (K = 9 is not matrix work): a VALU kernel, one thread per (pixel or window, 4 output
// channels), an fmaf chain over the nine taps in the same order, the same epilogue.
#include "kernels.h"

namespace s3 {

namespace {

constexpr int ROWB = 64;
typedef int i32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ void mma4(const uint4& a, const uint4& b, f32x16& c) {  // k order x, y, z, w (gemm_kernel<float>'s)
    c = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.x), __uint_as_float(b.x), c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.y), __uint_as_float(b.y), c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.z), __uint_as_float(b.z), c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.w), __uint_as_float(b.w), c, 0, 0, 0);
}

__device__ __forceinline__ float act1(float v, int act) {
    if (act == 1) return v < 0.f ? 0.f : v;  // ReLU; a NaN stays a NaN
    return v;
}
__device__ __forceinline__ float pmax(float a, float b) { return (a > b || a != a) ? a : b; }  // a NaN stays a NaN
__device__ __forceinline__ float4 act4(float4 v, const float4& b, int act) {
    v.x = act1(v.x + b.x, act); v.y = act1(v.y + b.y, act); v.z = act1(v.z + b.z, act); v.w = act1(v.w + b.w, act);
    return v;
}
// the affine epilogue: act(acc * s + t), one fma per element; s = 1, t = bias is bit for bit act4's acc + bias
__device__ __forceinline__ float4 aff4(float4 v, const float4& s, const float4& t, int act) {
    v.x = act1(fmaf(v.x, s.x, t.x), act); v.y = act1(fmaf(v.y, s.y, t.y), act); v.z = act1(fmaf(v.z, s.z, t.z), act);
    v.w = act1(fmaf(v.w, s.w, t.w), act);
    return v;
}
// the residual epilogue: act(acc * s + t + r), the fma first (a BasicBlock's bn2, then `out += identity`, then ReLU)
__device__ __forceinline__ float4 res4(float4 v, const float4& s, const float4& t, const float4& r, int act) {
    v.x = act1(fmaf(v.x, s.x, t.x) + r.x, act); v.y = act1(fmaf(v.y, s.y, t.y) + r.y, act); v.z = act1(fmaf(v.z, s.z, t.z) + r.z, act);
    v.w = act1(fmaf(v.w, s.w, t.w) + r.w, act);
    return v;
}
template <bool EXT>
__device__ __forceinline__ float4 ep4(const float4& v, const float4& s, const float4& t, int act) {
    if constexpr (EXT) return aff4(v, s, t, act);
    else return act4(v, t, act);
}
// the per-channel pair of the epilogue: (scale, shift), or (1, bias) / (1, 0) without an affine
template <bool EXT>
__device__ __forceinline__ void load_ep(const Conv2dParams& p, int n, bool ok, float4& s4, float4& t4) {
    s4 = make_float4(1.f, 1.f, 1.f, 1.f);
    t4 = make_float4(0.f, 0.f, 0.f, 0.f);
    if (!ok) return;
    if (EXT && p.scale) {
        s4 = *(const float4*)(p.scale + n);
        t4 = *(const float4*)(p.shift + n);
    } else if (p.bias) {
        t4 = *(const float4*)(p.bias + n);
    }
}
__device__ __forceinline__ float4 pmax4(const float4& a, const float4& b) {
    return make_float4(pmax(a.x, b.x), pmax(a.y, b.y), pmax(a.z, b.z), pmax(a.w, b.w));
}

// row m of the GEMM -> (example, y, x) of the un-pooled output pixel
__device__ __forceinline__ void pixel_of(int m, int HW, int W, int pool, int& b, int& y, int& x) {
    b = m / HW;
    const int p = m - b * HW;
    if (pool) {
        const int q = p >> 2, s = p & 3, Wh = W >> 1;
        const int wy = q / Wh, wx = q - wy * Wh;
        y = 2 * wy + (s >> 1);
        x = 2 * wx + (s & 1);
    } else {
        y = p / W;
        x = p - y * W;
    }
}

// WN = waves along N: 2 is the (64 TM) x 128 tile, 1 the (128 TM) x 64 tile for Cout <= 64 (all four waves along M; a wave's block,
// fragments and K order are the same, so the bits are too).  EXT = the affine epilogue and floor pooling (an example's M extent is
// 4 (H / 2) (W / 2): the dropped last row / column is never enumerated); EXT = false is VGGish's kernel as it was.  GEN (with EXT):
// k x k taps at stride 1 or 2 and the residual, no pooling.
template <int TM, int WN, bool EXT, bool GEN = false>
__global__ __launch_bounds__(256, 2) void conv2d3x3_kernel(Conv2dParams p) {
    constexpr int BM = (4 / WN) * 32 * TM, BN = 64 * WN;
    constexpr int PLANE = (BM + BN) * ROWB;
    constexpr int NPASS = (BM + BN) / 64;
    constexpr int APASS = BM / 64;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = WN == 2 ? wave >> 1 : wave, wc = WN == 2 ? wave & 1 : 0;
    const int half = lane >> 5;
    const int l31 = lane & 31;

    const int KS = GEN ? p.k : 3;                                     // taps per kernel row
    const int Wq = GEN ? conv2d_out(p.W, p.k, p.stride) : p.W;        // the width the M axis enumerates
    const int HW = GEN ? conv2d_out(p.H, p.k, p.stride) * Wq : (EXT && p.pool ? 4 * (p.H >> 1) * (p.W >> 1) : p.H * p.W);
    const int M = p.B * HW;
    const int n_tiles = (p.N + BN - 1) / BN;
    int tile;
    {  // XCD-aware tile order (gemm.hip): every XCD gets a contiguous range of the (m-tile, n-tile) sequence
        const int nwg = gridDim.x, wg = blockIdx.x;
        const int q8 = nwg >> 3, r8 = nwg & 7, xcd = wg & 7, loc = wg >> 3;
        tile = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + loc;
    }
    const int tn = tile % n_tiles, tm = tile / n_tiles;
    const int m0 = tm * BM, n0 = tn * BN;
    const int Kw = KS * KS * p.C;            // floats per weight row
    const int nkr = (KS * p.C) >> 4;         // 64-byte steps of one kernel row
    const int nk = Kw >> 4;
    const unsigned jump = (unsigned)(p.W + 2 - KS) * (unsigned)p.C * 4u;  // A bytes skipped between two kernel rows

    i32x4 rsrc_a, rsrc_w;
    {
        const unsigned long ua = (unsigned long)p.src, uw = (unsigned long)p.Wt;
        rsrc_a = (i32x4){(int)__builtin_amdgcn_readfirstlane((unsigned)ua), (int)__builtin_amdgcn_readfirstlane((unsigned)(ua >> 32)),
                         -1, 0x00020000};
        rsrc_w = (i32x4){(int)__builtin_amdgcn_readfirstlane((unsigned)uw), (int)__builtin_amdgcn_readfirstlane((unsigned)(uw >> 32)),
                         -1, 0x00020000};
    }
    // rows past M / N are clamped to the last one (never stored): every fetch stays inside the bordered images / the weights
    const int src_slot = (lane & 3) ^ ((lane >> 4) & 3);
    unsigned voff[NPASS];
#pragma unroll
    for (int i = 0; i < NPASS; ++i) {
        if (i < APASS) {
            int r = m0 + 16 * wave + 64 * i + (lane >> 2);
            r = r < M ? r : M - 1;
            int b, y, x;
            pixel_of(r, HW, Wq, GEN ? 0 : p.pool, b, y, x);
            if constexpr (GEN) {  // the first tap of output pixel (y, x): bordered pixel (y s + 1 - p, x s + 1 - p)
                y = y * p.stride + (KS == 1);
                x = x * p.stride + (KS == 1);
            }
            voff[i] = ((unsigned)b * (unsigned)p.src_bs + (unsigned)(y * (p.W + 2) + x) * (unsigned)p.C) * 4u + src_slot * 16;
        } else {
            int r = n0 + 16 * wave + 64 * (i - APASS) + (lane >> 2);
            r = r < p.N ? r : p.N - 1;
            voff[i] = (unsigned)r * (unsigned)(Kw * 4) + src_slot * 16;
        }
    }
    const unsigned lds0 = __builtin_amdgcn_readfirstlane((unsigned)(uintptr_t)(__attribute__((address_space(3))) char*)smem) + wave * 1024;
    auto dma = [&](unsigned vo, const i32x4& rs, unsigned dst, unsigned soff) {
        asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, %3 offen lds"
                     :
                     : "s"(dst), "v"(vo), "s"(rs), "s"(soff)
                     : "memory");
    };
    auto issue = [&](int kt, int slot) {
        const unsigned kw = (unsigned)kt * ROWB;
        const unsigned ka = kw + (kt >= nkr ? jump : 0u) + (kt >= 2 * nkr ? jump : 0u);
        const unsigned d0 = lds0 + slot * PLANE;
#pragma unroll
        for (int i = 0; i < NPASS; ++i) dma(voff[i], i < APASS ? rsrc_a : rsrc_w, d0 + i * 4096, i < APASS ? ka : kw);
    };

    const int swz = (l31 >> 2) & 3;
    const char* fa_base = smem + (wr * (TM * 32) + l31) * ROWB;
    const char* fb_base = smem + (BM + wc * 64 + l31) * ROWB;
    const int so0 = ((half * 2) ^ swz) << 4, so1 = ((half * 2 + 1) ^ swz) << 4;

    f32x16 acc[TM][2];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    struct Frag {
        uint4 a[TM], b[2];
    };
    auto read = [&](Frag& f, int slot, int so) {
#pragma unroll
        for (int i = 0; i < TM; ++i) f.a[i] = *(const uint4*)(fa_base + slot * PLANE + i * 32 * ROWB + so);
#pragma unroll
        for (int j = 0; j < 2; ++j) f.b[j] = *(const uint4*)(fb_base + slot * PLANE + j * 32 * ROWB + so);
    };
    issue(0, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    if (nk > 1) issue(1, 1);
    {
        auto mma = [&](const Frag& f, int i, int j) { mma4(f.a[i], f.b[j], acc[i][j]); };
        Frag f0, f1;
        read(f0, 0, so0);
        // step kt multiplies plane kt (LDS slot kt & 1) — gemmt.hip's K loop: one wait + barrier per step between the two halves
        auto step = [&](int kt, int slot) {
            read(f1, slot, so1);
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) mma(f0, i, j);
            __builtin_amdgcn_sched_barrier(0);
            asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
            __builtin_amdgcn_sched_barrier(0);
            mma(f1, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
            if (kt + 2 < nk) issue(kt + 2, slot);
            if (kt + 1 < nk) read(f0, slot ^ 1, so0);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    if (i | j) mma(f1, i, j);
        };
        int kt = 0;
        for (; kt + 1 < nk; kt += 2) {
            step(kt, 0);
            step(kt + 1, 1);
        }
        if (kt < nk) step(kt, 0);
    }
    // the last step's barrier ordered every wave's fragment reads before this point: the planes are free for the epilogue

    // ---- epilogue: each 32 x 64 block through a wave-private LDS transpose, then 16 lanes x 4 columns per row (or per window) ----
    float* stg = (float*)(smem + wave * 8192);
    const int c4 = (lane & 15) * 4;
    const int n = n0 + wc * 64 + c4;
    const bool n_ok = n < p.N;
    float4 scale4, bias4;
    load_ep<EXT>(p, n, n_ok, scale4, bias4);
    const int pad = p.dst_pad;
#pragma unroll
    for (int i = 0; i < TM; ++i) {
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) stg[((r & 3) + 8 * (r >> 2) + 4 * half) * 64 + j * 32 + l31] = acc[i][j][r];
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        const int mb = m0 + wr * (TM * 32) + i * 32;
        if (!GEN && p.pool) {
            const int Wo = p.W >> 1;
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const int row = (t * 4 + (lane >> 4)) * 4;  // the window's first row; its partners are the next three
                const int m = mb + row;
                if (m < M && n_ok) {
                    float4 v = ep4<EXT>(*(const float4*)(stg + row * 64 + c4), scale4, bias4, p.act);
#pragma unroll
                    for (int s = 1; s < 4; ++s) v = pmax4(v, ep4<EXT>(*(const float4*)(stg + (row + s) * 64 + c4), scale4, bias4, p.act));
                    int b, y, x;
                    pixel_of(m, HW, p.W, 1, b, y, x);
                    *(float4*)(p.dst + (long)b * p.dst_bs + ((long)((y >> 1) + pad) * (Wo + 2 * pad) + (x >> 1) + pad) * p.ld_dst + n) = v;
                }
            }
        } else {
#pragma unroll
            for (int t = 0; t < 8; ++t) {
                const int row = t * 4 + (lane >> 4);
                const int m = mb + row;
                if (m < M && n_ok) {
                    int b, y, x;
                    pixel_of(m, HW, Wq, 0, b, y, x);
                    float4 v = *(const float4*)(stg + row * 64 + c4);
                    if (GEN && p.res) {
                        const int rp = p.res_pad;
                        v = res4(v, scale4, bias4, *(const float4*)(p.res + (long)b * p.res_bs + ((long)(y + rp) * (Wq + 2 * rp) + x + rp) * p.ld_res + n),
                                 p.act);
                    } else {
                        v = ep4<EXT>(v, scale4, bias4, p.act);
                    }
                    *(float4*)(p.dst + (long)b * p.dst_bs + ((long)(y + pad) * (Wq + 2 * pad) + x + pad) * p.ld_dst + n) = v;
                }
            }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    }
}

// GEMM rows of the launch: every un-pooled pixel, or under pool the four pixels of every whole window
long m_rows(const Conv2dParams& p) {
    if (p.gen) return (long)p.B * conv2d_out(p.H, p.k, p.stride) * conv2d_out(p.W, p.k, p.stride);
    return (long)p.B * (p.pool ? 4L * (p.H / 2) * (p.W / 2) : (long)p.H * p.W);
}

template <int TM, int WN, bool EXT, bool GEN = false>
hipError_t go(const Conv2dParams& p, hipStream_t stream) {
    constexpr int BM = (4 / WN) * 32 * TM, BN = 64 * WN;
    constexpr int plane2 = 2 * (BM + BN) * ROWB;
    constexpr int lds = plane2 > 4 * 8192 ? plane2 : 4 * 8192;
    hipError_t e = ensure_dynamic_lds<conv2d3x3_kernel<TM, WN, EXT, GEN>>(lds);
    if (e != hipSuccess) return e;
    const long M = m_rows(p);
    dim3 grid((unsigned)(((M + BM - 1) / BM) * ((p.N + BN - 1) / BN)));
    hipLaunchKernelGGL((conv2d3x3_kernel<TM, WN, EXT, GEN>), grid, dim3(256), lds, stream, p);
    return hipGetLastError();
}

// ---- the C = 1 layer: thread = (pixel or window, 4 output channels) ----
template <int POOL, bool EXT>
__global__ __launch_bounds__(256) void conv2d3x3_first_kernel(Conv2dParams p) {
    const int n4 = p.N >> 2;
    const int Ho = POOL ? p.H >> 1 : p.H, Wo = POOL ? p.W >> 1 : p.W;
    const long items = (long)p.B * Ho * Wo * n4;
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= items) return;
    const int g = (int)(idx % n4);
    const long pix = idx / n4;
    const int xo = (int)(pix % Wo);
    const int yo = (int)((pix / Wo) % Ho);
    const int b = (int)(pix / ((long)Wo * Ho));
    const int n = g * 4;
    constexpr int S = POOL ? 2 : 1;  // un-pooled pixels per side of this thread's output
    // the (S + 2) x (S + 2) patch of the bordered single-channel image
    const float* img = p.src + (long)b * p.src_bs + (long)(yo * S) * (p.W + 2) + xo * S;
    float in[S + 2][S + 2];
#pragma unroll
    for (int r = 0; r < S + 2; ++r)
#pragma unroll
        for (int c = 0; c < S + 2; ++c) in[r][c] = img[r * (p.W + 2) + c];
    float4 w[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) w[t] = *(const float4*)(p.Wt + t * p.N + n);
    float4 scale4, bias4;
    load_ep<EXT>(p, n, true, scale4, bias4);
    float4 out = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int dy = 0; dy < S; ++dy)
#pragma unroll
        for (int dx = 0; dx < S; ++dx) {
            float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
            for (int t = 0; t < 9; ++t) {  // kernel rows ascending, taps ascending
                const float v = in[dy + t / 3][dx + t % 3];
                a.x = fmaf(v, w[t].x, a.x); a.y = fmaf(v, w[t].y, a.y); a.z = fmaf(v, w[t].z, a.z); a.w = fmaf(v, w[t].w, a.w);
            }
            a = ep4<EXT>(a, scale4, bias4, p.act);
            out = (dy | dx) ? pmax4(out, a) : a;
        }
    const int pad = p.dst_pad;
    *(float4*)(p.dst + (long)b * p.dst_bs + ((long)(yo + pad) * (Wo + 2 * pad) + xo + pad) * p.ld_dst + n) = out;
}

}  // namespace

void pack_conv2d3x3(const float* w, int N, int C, std::vector<float>& out) {
    out.assign((size_t)N * 9 * C, 0.f);
    if (C == 1) {  // the first layer's image: (9, N) tap-major
        for (int n = 0; n < N; ++n)
            for (int t = 0; t < 9; ++t) out[(size_t)t * N + n] = w[(size_t)n * 9 + t];
        return;
    }
    for (int n = 0; n < N; ++n)
        for (int c = 0; c < C; ++c)
            for (int t = 0; t < 9; ++t) out[((size_t)n * 9 + t) * C + c] = w[((size_t)n * C + c) * 9 + t];
}

const char* conv2d3x3_refusal(const Conv2dParams& p) {
    if (!p.src || !p.Wt || !p.dst) return "null operand";
    if (p.B < 1 || p.H < 1 || p.W < 1 || p.N < 4 || p.C < 1) return "bad shape";
    if (p.C != 1 && (p.C & 15)) return "Cin must be 1 (the first-layer kernel) or a multiple of 16 (a tap is a whole number of 64-byte K steps)";
    if (p.N & 3) return "Cout must be a multiple of 4 (vector stores)";
    if (p.act < 0 || p.act > 1) return "act must be 0 (none) or 1 (ReLU)";
    if (p.pool < 0 || p.pool > 1) return "pool must be 0 or 1";
    if (p.pool_floor < 0 || p.pool_floor > 1) return "pool_floor must be 0 or 1";
    if (p.pool_floor && !p.pool) return "pool_floor needs pool";
    if (p.pool && !p.pool_floor && ((p.H | p.W) & 1)) return "H and W must be even under pool (2 x 2 windows, stride 2)";
    if (p.pool_floor && (p.H < 2 || p.W < 2)) return "the map is smaller than one 2 x 2 pool window";
    if ((p.scale != nullptr) != (p.shift != nullptr)) return "the affine needs both scale and shift";
    if (p.scale && p.bias) return "bias and an affine together: the shift carries the bias";
    if (p.gen < 0 || p.gen > 1) return "gen must be 0 or 1";
    if (!p.gen && (p.k || p.stride || p.res)) return "kernel size, stride and residual belong to the general form (gen = 1)";
    if (p.gen) {
        if (p.k != 1 && p.k != 3) return "the kernel size must be 3 or 1";
        if (p.stride != 1 && p.stride != 2) return "the stride must be 1 or 2";
        if (p.pool) return "the general form does not pool";
        if (p.C == 1) return "the general form needs Cin to be a multiple of 16";
        if (p.res) {
            if (p.res_pad < 0) return "res border width must not be negative";
            if (p.ld_res < p.N) return "the res pixel pitch is smaller than Cout";
            if ((p.ld_res | p.res_bs) & 3) return "res pixel pitch and example stride must be multiples of 4 floats (vector loads)";
            if ((uintptr_t)p.res & 15) return "operands must be 16-byte aligned";
            const long Ho = conv2d_out(p.H, p.k, p.stride), Wo = conv2d_out(p.W, p.k, p.stride);
            if (p.B > 1 && p.res_bs < (Ho + 2 * p.res_pad) * (Wo + 2 * p.res_pad) * p.ld_res) return "res example stride is smaller than one bordered image";
        }
    }
    if (p.dst_pad < 0) return "dst border width must not be negative";
    if (p.ld_dst < p.N) return "the dst pixel pitch is smaller than Cout";
    if ((p.ld_dst | p.dst_bs) & 3) return "dst pixel pitch and example stride must be multiples of 4 floats (vector stores)";
    if (p.C != 1 && (p.src_bs & 3)) return "src example stride must be a multiple of 4 floats";
    if (p.src_bs < (long)(p.H + 2) * (p.W + 2) * p.C) return "src example stride is smaller than one bordered image";
    {
        const long Ho = p.gen ? conv2d_out(p.H, p.k, p.stride) : (p.pool ? p.H / 2 : p.H);
        const long Wo = p.gen ? conv2d_out(p.W, p.k, p.stride) : (p.pool ? p.W / 2 : p.W);
        if (p.B > 1 && p.dst_bs < (Ho + 2 * p.dst_pad) * (Wo + 2 * p.dst_pad) * p.ld_dst)
            return "dst example stride is smaller than one bordered image";
    }
    if (((uintptr_t)p.Wt | (uintptr_t)p.bias | (uintptr_t)p.scale | (uintptr_t)p.shift | (uintptr_t)p.dst | (p.C == 1 ? 0 : (uintptr_t)p.src)) & 15)
        return "operands must be 16-byte aligned";
    if ((uintptr_t)p.src & 3) return "operands must be 4-byte aligned";
    const unsigned long a_span = (unsigned long)p.B * (unsigned long)p.src_bs * 4ul;
    const unsigned long w_span = (unsigned long)p.N * (p.gen ? (unsigned long)(p.k * p.k) : 9ul) * (unsigned long)p.C * 4ul;
    if (a_span >= (1ul << 32) - 64 || w_span >= (1ul << 32) - 64) return "an operand is not addressable with 32-bit offsets";
    const long M = m_rows(p);
    if (M > 0x7fffffffL - 256) return "too many pixels";
    if (((M + 63) / 64) * ((p.N + 63) / 64) > 0x7fffffffL || M * (p.N / 4) / 256 > 0x7fffffffL) return "too many tiles";
    return nullptr;
}

hipError_t launch_conv2d3x3(const Conv2dParams& p, hipStream_t stream) {
    if (conv2d3x3_refusal(p)) return hipErrorInvalidValue;
    // the instantiations with the affine epilogue / floor pooling / the 64-wide tile serve only the launches that ask for them
    const bool ext = p.scale || p.pool_floor || p.n64;
    if (p.gen) {  // the tile rules of the instantiations below
        const long M = m_rows(p);
        if (p.n64 && p.N <= 64 && tuning().conv2d_n64)
            return (M > 128 && (M + 255) / 256 >= device_cus()) ? go<2, 1, true, true>(p, stream) : go<1, 1, true, true>(p, stream);
        const bool big = M > 64 && ((M + 127) / 128) * ((p.N + 127) / 128) >= device_cus();
        return big ? go<2, 2, true, true>(p, stream) : go<1, 2, true, true>(p, stream);
    }
    if (p.C == 1) {
        const long items = (long)p.B * (p.pool ? (p.H / 2) * (p.W / 2) : p.H * p.W) * (p.N / 4);
        dim3 grid((unsigned)((items + 255) / 256));
        if (ext) {
            if (p.pool)
                hipLaunchKernelGGL((conv2d3x3_first_kernel<1, true>), grid, dim3(256), 0, stream, p);
            else
                hipLaunchKernelGGL((conv2d3x3_first_kernel<0, true>), grid, dim3(256), 0, stream, p);
        } else if (p.pool)
            hipLaunchKernelGGL((conv2d3x3_first_kernel<1, false>), grid, dim3(256), 0, stream, p);
        else
            hipLaunchKernelGGL((conv2d3x3_first_kernel<0, false>), grid, dim3(256), 0, stream, p);
        return hipGetLastError();
    }
    const long M = m_rows(p);
    if (ext && p.n64 && p.N <= 64 && tuning().conv2d_n64) {
        // Cout <= 64: a 128-wide tile would multiply 64 columns of padding; 256-row tiles once they fill the chip (the bits are the same)
        return (M > 128 && (M + 255) / 256 >= device_cus()) ? go<2, 1, true>(p, stream) : go<1, 1, true>(p, stream);
    }
    // 128-row tiles once they fill the chip, 64-row tiles for few pixels (the bits are the same)
    const long t128 = ((M + 127) / 128) * ((p.N + 127) / 128);
    const bool big = M > 64 && t128 >= device_cus();
    if (ext) return big ? go<2, 2, true>(p, stream) : go<1, 2, true>(p, stream);
    return big ? go<2, 2, false>(p, stream) : go<1, 2, false>(p, stream);
}

}  // namespace s3
