// patchstrided.hip — exact-fp32 patch embedding with OVERLAPPING patches of a (rows, 128) image, as an implicit GEMM over the tokens of
// all windows: SSAST's Conv2d(1, N, (fshape, tshape), stride (fstride, tstride)) on the (128, rows) transpose of the image, its bias,
// the token's position row and the sequence layout with two prefix tokens (upstream/ssast/ast_models.py:367-378).
//
//   out[w][2 + ti*f_dim + fi][n] = sum_{t<tshape} sum_{f<fshape} img[w][ti*tstride + t][fi*fstride + f] * W[n][t*fshape + f]
//                                  + bias[n] + pos[ti*f_dim + fi][n],      out[w][0 | 1][n] = prefix[0 | 1][n]
//
// with f_dim = (128 - fshape) / fstride + 1, t_dim = (rows - tshape) / tstride + 1 and the tokens of a window TIME-major: the f_dim
// tokens of one time step are neighbours, so rows 2 + ti*f_dim .. of a sequence are one state row of f_dim * N floats.  (The reference
// orders them f-major; attention has neither a mask nor a relative position, so the model is equivariant under the permutation and the
// caller hands `pos` over in this order.)  W is the conv weight permuted to [n][t][f]: K = tshape * fshape is walked as tshape runs of
// fshape contiguous floats, run t at image row ti*tstride + t, column fi*fstride.
//
// Schedule: patchembed.hip's (v_mfma_f32_32x32x2_f32 on 64-byte K steps, XOR-swizzled lane-linear planes, two register sets of fragments
// around the step's one barrier, the XCD-aware tile order, a (128 | 64) x 128 tile per (window, m-tile, n-tile)) with one difference.  A
// patch row starts at a multiple of 4 * fstride bytes — 40 for the 16 x 16 / stride 10 geometry: 8-byte aligned, not 16 — so the A
// operand does not go through the LDS-DMA: a lane fetches its 16-byte piece as two 8-byte global loads into registers one step ahead
// and writes the swizzled LDS slot itself before the step's barrier.  W keeps the DMA path.  Per output element the order is fixed
// (runs ascending, then the step's order): a token's bits depend neither on the number of windows, nor on the window it sits in, nor on
// the tile height.  Rows past the window's last token are clamped to it (never stored): no load reaches past the window's `rows`
// image rows.
//
// The two-step form (tuning key patch_strided_fused = 0) is the yardstick and a second implementation: a gather into (tokens, K) rows,
// the tile GEMM storing at the sequence pitch, then the position add.
#include "kernels.h"

namespace s3 {

namespace {

constexpr int BN = 128, ROWB = 64, IMG_W = 128;
typedef int i32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ void mma4(const uint4& a, const uint4& b, f32x16& c) {  // k order x, y, z, w (gemm_kernel<float>'s)
    c = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.x), __uint_as_float(b.x), c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.y), __uint_as_float(b.y), c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.z), __uint_as_float(b.z), c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.w), __uint_as_float(b.w), c, 0, 0, 0);
}

template <int TM>
__global__ __launch_bounds__(256, 2) void patch_strided_kernel(PatchStridedParams p) {
    constexpr int BM = 64 * TM;
    constexpr int PLANE = (BM + BN) * ROWB;
    constexpr int APASS = BM / 64;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave >> 1, wc = wave & 1;
    const int half = lane >> 5;
    const int l31 = lane & 31;

    const int T = p.f_dim * p.t_dim;            // patch tokens per window
    const int n_tiles = (p.N + BN - 1) / BN;
    const int m_tiles = (T + BM - 1) / BM;
    int tile;
    {  // XCD-aware tile order (gemm.hip): every XCD gets a contiguous range of the (window, m-tile, n-tile) sequence
        const int nwg = gridDim.x, wg = blockIdx.x;
        const int q8 = nwg >> 3, r8 = nwg & 7, xcd = wg & 7, loc = wg >> 3;
        tile = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + loc;
    }
    const int tn = tile % n_tiles;
    const int tmb = tile / n_tiles;
    const int tm = tmb % m_tiles, win = tmb / m_tiles;
    const int m0 = tm * BM, n0 = tn * BN;
    const int Kw = p.tshape * p.fshape;         // floats per weight row
    const int ssh = p.sshift;                   // fshape / 16 = 1 << ssh 64-byte steps per run
    const int nk = Kw >> 4;

    i32x4 rsrc_w;
    {
        const unsigned long uw = (unsigned long)p.W;
        rsrc_w = (i32x4){(int)__builtin_amdgcn_readfirstlane((unsigned)uw), (int)__builtin_amdgcn_readfirstlane((unsigned)(uw >> 32)),
                         -1, 0x00020000};
    }
    const float* img = p.img + (long)win * p.img_bs;
    // rows past T / N are clamped to the last one (never stored): every fetch stays inside the window's `rows` image rows
    const int src_slot = (lane & 3) ^ ((lane >> 4) & 3);  // the W DMA: LDS slot lane & 3 of row lane >> 2 holds this source slot
    unsigned aoff[APASS];                                 // floats: the token's first image element + this lane's 4-float piece
    unsigned woff[2];
#pragma unroll
    for (int i = 0; i < APASS; ++i) {
        int r = m0 + 16 * wave + 64 * i + (lane >> 2);
        r = r < T ? r : T - 1;
        const int ti = r / p.f_dim, fi = r - ti * p.f_dim;
        aoff[i] = (unsigned)(ti * p.tstride) * (unsigned)IMG_W + (unsigned)(fi * p.fstride) + (unsigned)(lane & 3) * 4u;
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        int r = n0 + 16 * wave + 64 * i + (lane >> 2);
        r = r < p.N ? r : p.N - 1;
        woff[i] = (unsigned)r * (unsigned)(Kw * 4) + src_slot * 16;
    }
    const unsigned lds0 = __builtin_amdgcn_readfirstlane((unsigned)(uintptr_t)(__attribute__((address_space(3))) char*)smem) + wave * 1024;
    auto dma = [&](unsigned vo, const i32x4& rs, unsigned dst, unsigned soff) {
        asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, %3 offen lds"
                     :
                     : "s"(dst), "v"(vo), "s"(rs), "s"(soff)
                     : "memory");
    };
    // the A piece of this lane in LDS: row 16 * wave + 64 * i + (lane >> 2) of the plane, source slot lane & 3 at slot ^ ((row >> 2) & 3)
    char* a_dst = smem + (16 * wave + (lane >> 2)) * ROWB + (((lane & 3) ^ ((lane >> 4) & 3)) << 4);
    float2 areg[APASS][2];
    // step ks is step (ks mod steps-per-run) of run ks / steps-per-run: the next image row is IMG_W floats further
    auto fetch_a = [&](int ks) {
        const unsigned ka = (unsigned)(ks >> ssh) * (unsigned)IMG_W + (unsigned)(ks & ((1 << ssh) - 1)) * 16u;
#pragma unroll
        for (int i = 0; i < APASS; ++i) {
            const float* s = img + (aoff[i] + ka);  // 8-byte aligned: fstride is even, every other term a multiple of 4 floats
            areg[i][0] = *(const float2*)s;
            areg[i][1] = *(const float2*)(s + 2);
        }
    };
    auto store_a = [&](int slot) {
#pragma unroll
        for (int i = 0; i < APASS; ++i)
            *(float4*)(a_dst + slot * PLANE + i * 4096) = make_float4(areg[i][0].x, areg[i][0].y, areg[i][1].x, areg[i][1].y);
    };
    auto issue_w = [&](int ks, int slot) {
        const unsigned d0 = lds0 + slot * PLANE + BM * ROWB;
#pragma unroll
        for (int i = 0; i < 2; ++i) dma(woff[i], rsrc_w, d0 + i * 4096, (unsigned)ks * ROWB);
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
    // plane 0 whole, plane 1's W in flight and its A pieces in registers
    issue_w(0, 0);
    fetch_a(0);
    store_a(0);
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    if (nk > 1) {
        issue_w(1, 1);
        fetch_a(1);
    }
    {
        auto mma = [&](const Frag& f, int i, int j) { mma4(f.a[i], f.b[j], acc[i][j]); };
        Frag f0, f1;
        read(f0, 0, so0);
        // step ks multiplies plane ks (LDS slot ks & 1).  Before its barrier the wave writes the A pieces of plane ks + 1 (fetched one
        // step ago) into the other slot, whose last readers passed the barrier of step ks - 1; the barrier publishes them together
        // with that plane's W DMA.  Behind it slot ks & 1 is free: the W DMA and the A fetch of plane ks + 2 start
        auto step = [&](int ks, int slot) {
            read(f1, slot, so1);
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) mma(f0, i, j);
            __builtin_amdgcn_sched_barrier(0);
            if (ks + 1 < nk) store_a(slot ^ 1);
            asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
            __builtin_amdgcn_sched_barrier(0);
            mma(f1, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
            if (ks + 2 < nk) {
                issue_w(ks + 2, slot);
                fetch_a(ks + 2);
            }
            if (ks + 1 < nk) read(f0, slot ^ 1, so0);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    if (i | j) mma(f1, i, j);
        };
        int ks = 0;
        for (; ks + 1 < nk; ks += 2) {
            step(ks, 0);
            step(ks + 1, 1);
        }
        if (ks < nk) step(ks, 0);
    }
    // the last step's barrier ordered every wave's fragment reads before this point: the planes are free for the epilogue

    // ---- epilogue: each 32 x 64 block through a wave-private LDS transpose, then 16 lanes x 4 columns per row ----
    float* stg = (float*)(smem + wave * 8192);
    const int c4 = (lane & 15) * 4;
    const int n = n0 + wc * 64 + c4;
    const bool n_ok = n < p.N;
    float4 bias4 = make_float4(0.f, 0.f, 0.f, 0.f);
    if (p.bias && n_ok) bias4 = *(const float4*)(p.bias + n);
    float* ob = p.out + ((long)win * (T + 2) + 2) * p.N;  // the window's sequence behind its two prefix rows
#pragma unroll
    for (int i = 0; i < TM; ++i) {
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) stg[((r & 3) + 8 * (r >> 2) + 4 * half) * 64 + j * 32 + l31] = acc[i][j][r];
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            const int row = t * 4 + (lane >> 4);
            float4 v = *(const float4*)(stg + row * 64 + c4);
            const int m = m0 + wr * (TM * 32) + i * 32 + row;
            if (m < T && n_ok) {
                v.x += bias4.x; v.y += bias4.y; v.z += bias4.z; v.w += bias4.w;
                if (p.pos) {
                    const float4 q = *(const float4*)(p.pos + (long)m * p.N + n);
                    v.x += q.x; v.y += q.y; v.z += q.z; v.w += q.w;
                }
                *(float4*)(ob + (long)m * p.N + n) = v;
            }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    }
}

template <int TM>
hipError_t go(const PatchStridedParams& p, hipStream_t stream) {
    constexpr int BM = 64 * TM;
    constexpr int plane2 = 2 * (BM + BN) * ROWB;
    constexpr int lds = plane2 > 4 * 8192 ? plane2 : 4 * 8192;
    hipError_t e = ensure_dynamic_lds<patch_strided_kernel<TM>>(lds);
    if (e != hipSuccess) return e;
    const int T = p.f_dim * p.t_dim;
    dim3 grid(((T + BM - 1) / BM) * ((p.N + BN - 1) / BN) * p.nwin);
    hipLaunchKernelGGL((patch_strided_kernel<TM>), grid, dim3(256), lds, stream, p);
    return hipGetLastError();
}

// out[w][0 | 1][:] = prefix[0 | 1][:]: one thread per 16-byte piece
__global__ __launch_bounds__(256) void patch_prefix_kernel(PatchStridedParams p) {
    const int n4 = p.N >> 2;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)p.nwin * 2 * n4) return;
    const long wrow = i / n4;  // window * 2 + prefix row
    const int n = (int)(i - wrow * n4) * 4;
    const long w = wrow >> 1;
    const int r = (int)(wrow & 1);
    const long T = (long)p.f_dim * p.t_dim;
    *(float4*)(p.out + (w * (T + 2) + r) * p.N + n) = *(const float4*)(p.prefix + (long)r * p.N + n);
}

// ---- the two-step form's row passes ----
// rows[(w * T + m)][t * fshape + f] = img[w][ti * tstride + t][fi * fstride + f]: one thread per 8-byte piece
__global__ __launch_bounds__(256) void patch_strided_gather_kernel(PatchStridedParams p, float* rows) {
    const int K = p.tshape * p.fshape, k2 = K >> 1;
    const long T = (long)p.f_dim * p.t_dim;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)p.nwin * T * k2) return;
    const long row = i / k2;
    const int k = (int)(i - row * k2) * 2;
    const long w = row / T;
    const int m = (int)(row - w * T);
    const int ti = m / p.f_dim, fi = m - ti * p.f_dim;
    const int t = k / p.fshape, f = k - t * p.fshape;
    *(float2*)(rows + row * K + k) = *(const float2*)(p.img + w * p.img_bs + ((long)ti * p.tstride + t) * IMG_W + fi * p.fstride + f);
}

// out[w][2 + m] += pos[m]
__global__ __launch_bounds__(256) void patch_strided_pos_kernel(PatchStridedParams p) {
    const int n4 = p.N >> 2;
    const long T = (long)p.f_dim * p.t_dim;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)p.nwin * T * n4) return;
    const long row = i / n4;
    const int n = (int)(i - row * n4) * 4;
    const long w = row / T;
    const long m = row - w * T;
    float* o = p.out + (w * (T + 2) + 2 + m) * p.N + n;
    float4 v = *(const float4*)o;
    const float4 q = *(const float4*)(p.pos + m * p.N + n);
    v.x += q.x; v.y += q.y; v.z += q.z; v.w += q.w;
    *(float4*)o = v;
}

hipError_t launch_prefix(const PatchStridedParams& p, hipStream_t stream) {
    if (!p.prefix) return hipSuccess;
    const long g = ((long)p.nwin * 2 * (p.N >> 2) + 255) / 256;
    hipLaunchKernelGGL(patch_prefix_kernel, dim3((unsigned)g), dim3(256), 0, stream, p);
    return hipGetLastError();
}

}  // namespace

void patch_strided_geometry(PatchStridedParams& p) {
    p.f_dim = p.t_dim = p.sshift = 0;
    if (p.fshape == 16 || p.fshape == 32 || p.fshape == 64 || p.fshape == 128) p.sshift = __builtin_ctz(p.fshape / 16);
    if (p.fshape >= 1 && p.fshape <= IMG_W && p.fstride >= 1) p.f_dim = (IMG_W - p.fshape) / p.fstride + 1;
    if (p.tshape >= 1 && p.tstride >= 1 && p.rows >= p.tshape) p.t_dim = (p.rows - p.tshape) / p.tstride + 1;
}

const char* patch_strided_refusal(const PatchStridedParams& p) {
    if (!p.img || !p.W || !p.out) return "null operand";
    if (p.fshape != 16 && p.fshape != 32 && p.fshape != 64 && p.fshape != 128)
        return "fshape must be 16, 32, 64 or 128 (a patch row is a whole number of 64-byte K steps of a 128-wide image)";
    if (p.tshape < 1 || p.tshape > 32) return "tshape must be 1..32";
    if (p.fstride < 2 || p.fstride > 128 || (p.fstride & 1)) return "fstride must be even, 2..128 (a patch row starts 8-byte aligned)";
    if (p.tstride < 1 || p.tstride > 1024) return "tstride must be 1..1024";
    if (p.nwin < 1 || p.N < 4) return "bad shape";
    if (p.rows < p.tshape) return "the image has fewer rows than one patch (rows < tshape)";
    if (p.rows > (1 << 20)) return "too many image rows";
    if (p.N & 3) return "N must be a multiple of 4 (vector stores)";
    if (p.sshift != __builtin_ctz(p.fshape / 16) || p.f_dim != (IMG_W - p.fshape) / p.fstride + 1 ||
        p.t_dim != (p.rows - p.tshape) / p.tstride + 1)
        return "f_dim / t_dim / sshift do not belong to the geometry (internal)";
    if (p.img_bs & 3) return "img window stride must be a multiple of 4 floats";
    if (p.img_bs < (long)p.rows * IMG_W) return "img window stride is smaller than the window's image rows";
    if (((uintptr_t)p.img | (uintptr_t)p.W | (uintptr_t)p.bias | (uintptr_t)p.pos | (uintptr_t)p.prefix | (uintptr_t)p.out) & 15)
        return "operands must be 16-byte aligned";
    const unsigned long w_span = (unsigned long)p.N * (unsigned long)(p.tshape * p.fshape) * 4ul;
    if (w_span >= (1ul << 32) - 64) return "an operand is not addressable with 32-bit offsets";
    const long T = (long)p.f_dim * p.t_dim;
    if (T > 0x7fffffffL / 4) return "too many tokens per window";
    const long tiles = (long)p.nwin * ((T + 63) / 64) * ((p.N + BN - 1) / BN);
    if (tiles > 0x7fffffffL) return "too many tiles";
    if ((long)p.nwin * (T + 2) > 0x7fffffffL / 4) return "too many rows";
    return nullptr;
}

hipError_t launch_patch_strided(const PatchStridedParams& p, hipStream_t stream) {
    if (patch_strided_refusal(p)) return hipErrorInvalidValue;
    // 128-row tiles once they fill the chip, 64-row tiles for short or few windows (the bits are the same)
    const long T = (long)p.f_dim * p.t_dim;
    const long t128 = (long)p.nwin * ((T + 127) / 128) * ((p.N + BN - 1) / BN);
    hipError_t e = (T > 64 && t128 >= device_cus()) ? go<2>(p, stream) : go<1>(p, stream);
    return e != hipSuccess ? e : launch_prefix(p, stream);
}

hipError_t launch_patch_strided_tile(const PatchStridedParams& p, int tile_rows, hipStream_t stream) {
    if (patch_strided_refusal(p) || (tile_rows != 64 && tile_rows != 128)) return hipErrorInvalidValue;
    hipError_t e = tile_rows == 128 ? go<2>(p, stream) : go<1>(p, stream);
    return e != hipSuccess ? e : launch_prefix(p, stream);
}

size_t patch_strided_rows_elems(const PatchStridedParams& p) {
    return (size_t)p.nwin * (size_t)p.f_dim * (size_t)p.t_dim * (size_t)(p.tshape * p.fshape);
}

hipError_t launch_patch_strided_two_step(const PatchStridedParams& p, float* rows, hipStream_t stream) {
    if (patch_strided_refusal(p) || !rows || ((uintptr_t)rows & 15)) return hipErrorInvalidValue;
    const long T = (long)p.f_dim * p.t_dim, M = (long)p.nwin * T;
    const int K = p.tshape * p.fshape;
    const long g1 = (M * (K >> 1) + 255) / 256, g2 = (M * (p.N >> 2) + 255) / 256;
    if (g1 > 0x7fffffffL || g2 > 0x7fffffffL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(patch_strided_gather_kernel, dim3((unsigned)g1), dim3(256), 0, stream, p, rows);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    GemmParams g{};  // one batch per window: the products land behind the window's two prefix rows
    g.A = rows;
    g.lda = K;
    g.a_bs = T * K;
    g.W = p.W;
    g.bias = p.bias;
    g.M = (int)T;
    g.N = p.N;
    g.K = K;
    g.batches = p.nwin;
    g.out32 = p.out + 2L * p.N;
    g.ldo = p.N;
    g.o_bs = (T + 2) * p.N;
    e = launch_gemm(0 /* fp32 */, g, stream);
    if (e != hipSuccess) return e;
    if (p.pos) hipLaunchKernelGGL(patch_strided_pos_kernel, dim3((unsigned)g2), dim3(256), 0, stream, p);
    e = hipGetLastError();
    return e != hipSuccess ? e : launch_prefix(p, stream);
}

}  // namespace s3
