// patchembed.hip — exact-fp32 patch embedding of a (frames, 128) log-mel image as an implicit GEMM over the tokens of all utterances:
// MAE-AST's nn.Unfold((kt, kc), stride = kernel) + Linear(kt * kc, N) + sinusoidal position row (upstream/mae_ast/mae_ast.py:219-222,
// 415-449).
//
//   out[b][t*V+v][n] = sum_{r<kt} sum_{c<kc} img[b][t*kt + r][v*kc + c] * W[n][r*kc + c] + bias[n] + (t*V+v < kv[b] ? pos[t*V+v][n] : 0)
//
// with V = 128 / kc tokens per time step, time the slow axis of the token order and a patch's content in (time, channel) row-major
// order — exactly the Linear's own K order, so W is the (N, kt * kc) matrix as stored.  The image has a row stride of 128 floats:
// a token is kt pieces of kc floats that are 512 bytes apart, which no lda / batch stride of the tile GEMM expresses.  kc is a
// multiple of 16, so a patch row is a whole number of 64-byte K steps and every 16-byte piece is contiguous in the image.  The K
// walk is kt runs of kc floats: between two runs the A offset jumps to the next image row (512 bytes), the W offset does not jump.
// A token row's base address is computed per row (t and v share no stride unless kt = 1).  Frames at or past Tt * kt are never read.
//
// Schedule: convtaps.hip's, for the same arithmetic (v_mfma_f32_32x32x2_f32 on 64-byte K steps, LDS-DMA staging of lane-linear planes
// with the XOR swizzle applied to the source slot and a per-lane source address, two register sets of fragments around the step's
// one barrier, the XCD-aware tile order) on a (128 | 64) x 128 tile per (utterance, m-tile, n-tile).  Per output element the order
// is fixed — runs ascending, then the step's order — so a token row's bits depend neither on B, nor on its place in the batch, nor on
// Tt, nor on the tile height.
//
// The two-step form (tuning key patch_embed_fused = 0) is the yardstick and a second implementation: patch_gather_kernel writes the
// (B * Tt * V, kt * kc) rows, the tile GEMM multiplies them, patch_pos_kernel adds the position rows.
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
__global__ __launch_bounds__(256, 2) void patch_embed_kernel(PatchEmbedParams p) {
    constexpr int BM = 64 * TM;
    constexpr int PLANE = (BM + BN) * ROWB;
    constexpr int NPASS = (BM + BN) / 64;
    constexpr int APASS = BM / 64;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave >> 1, wc = wave & 1;
    const int half = lane >> 5;
    const int l31 = lane & 31;

    const int vsh = p.vshift;                   // V = 1 << vsh tokens per time step
    const int T = p.Tt << vsh;                  // tokens per utterance
    const int n_tiles = (p.N + BN - 1) / BN;
    const int m_tiles = (T + BM - 1) / BM;
    int tile;
    {  // XCD-aware tile order (gemm.hip): every XCD gets a contiguous range of the (utterance, m-tile, n-tile) sequence
        const int nwg = gridDim.x, wg = blockIdx.x;
        const int q8 = nwg >> 3, r8 = nwg & 7, xcd = wg & 7, loc = wg >> 3;
        tile = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + loc;
    }
    const int tn = tile % n_tiles;
    const int tmb = tile / n_tiles;
    const int tm = tmb % m_tiles, b = tmb / m_tiles;
    const int m0 = tm * BM, n0 = tn * BN;
    const int Kw = p.kt * p.kc;                 // floats per weight row
    const int ssh = p.sshift;                   // kc / 16 = 1 << ssh 64-byte steps per run
    const int nk = Kw >> 4;

    i32x4 rsrc_a, rsrc_w;
    {
        const unsigned long ua = (unsigned long)(p.img + (long)b * p.img_bs), uw = (unsigned long)p.W;
        rsrc_a = (i32x4){(int)__builtin_amdgcn_readfirstlane((unsigned)ua), (int)__builtin_amdgcn_readfirstlane((unsigned)(ua >> 32)),
                         -1, 0x00020000};
        rsrc_w = (i32x4){(int)__builtin_amdgcn_readfirstlane((unsigned)uw), (int)__builtin_amdgcn_readfirstlane((unsigned)(uw >> 32)),
                         -1, 0x00020000};
    }
    // rows past T / N are clamped to the last one (never stored): every fetch stays inside the utterance's Tt * kt image rows
    const int src_slot = (lane & 3) ^ ((lane >> 4) & 3);
    unsigned voff[NPASS];
#pragma unroll
    for (int i = 0; i < NPASS; ++i) {
        if (i < APASS) {
            int r = m0 + 16 * wave + 64 * i + (lane >> 2);
            r = r < T ? r : T - 1;
            const int t = r >> vsh, v = r - (t << vsh);  // token r = (time step t, channel patch v): its first image row and column
            voff[i] = ((unsigned)(t * p.kt) * (unsigned)IMG_W + (unsigned)(v * p.kc)) * 4u + src_slot * 16;
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
    auto issue = [&](int ks, int slot) {
        const unsigned kw = (unsigned)ks * ROWB;
        // step ks is step (ks mod steps-per-run) of run ks / steps-per-run: the next image row is IMG_W floats further
        const unsigned ka = (unsigned)(ks >> ssh) * (unsigned)(IMG_W * 4) + (unsigned)(ks & ((1 << ssh) - 1)) * ROWB;
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
        // step ks multiplies plane ks (LDS slot ks & 1) — gemmt.hip's K loop: one wait + barrier per step between the two halves
        auto step = [&](int ks, int slot) {
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
            if (ks + 2 < nk) issue(ks + 2, slot);
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
    const int kvb = p.pos ? p.kv[b] : 0;  // tokens of this utterance that carry a position row
    float4 bias4 = make_float4(0.f, 0.f, 0.f, 0.f);
    if (p.bias && n_ok) bias4 = *(const float4*)(p.bias + n);
    float* ob = p.out + (long)b * T * p.N;
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
                if (m < kvb) {
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
hipError_t go(const PatchEmbedParams& p, hipStream_t stream) {
    constexpr int BM = 64 * TM;
    constexpr int plane2 = 2 * (BM + BN) * ROWB;
    constexpr int lds = plane2 > 4 * 8192 ? plane2 : 4 * 8192;
    hipError_t e = ensure_dynamic_lds<patch_embed_kernel<TM>>(lds);
    if (e != hipSuccess) return e;
    const int T = p.Tt << p.vshift;
    dim3 grid(((T + BM - 1) / BM) * ((p.N + BN - 1) / BN) * p.B);
    hipLaunchKernelGGL((patch_embed_kernel<TM>), grid, dim3(256), lds, stream, p);
    return hipGetLastError();
}

// ---- the two-step form's row passes ----
// rows[(b * T + m)][r * kc + c] = img[b][t * kt + r][v * kc + c]: one thread per 16-byte piece
__global__ __launch_bounds__(256) void patch_gather_kernel(PatchEmbedParams p, float* rows) {
    const int K = p.kt * p.kc, k4 = K >> 2;
    const long T = (long)p.Tt << p.vshift;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)p.B * T * k4) return;
    const long row = i / k4;
    const int k = (int)(i - row * k4) * 4;
    const long b = row / T;
    const int m = (int)(row - b * T);
    const int t = m >> p.vshift, v = m - (t << p.vshift);
    const int r = k / p.kc, c = k - r * p.kc;
    *(float4*)(rows + row * K + k) = *(const float4*)(p.img + b * p.img_bs + ((long)t * p.kt + r) * IMG_W + v * p.kc + c);
}

// out[b][m] += pos[m] for m < kv[b]
__global__ __launch_bounds__(256) void patch_pos_kernel(PatchEmbedParams p) {
    const int n4 = p.N >> 2;
    const long T = (long)p.Tt << p.vshift;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)p.B * T * n4) return;
    const long row = i / n4;
    const int n = (int)(i - row * n4) * 4;
    const long b = row / T;
    const long m = row - b * T;
    if (m >= p.kv[b]) return;
    float4 v = *(const float4*)(p.out + row * p.N + n);
    const float4 q = *(const float4*)(p.pos + m * p.N + n);
    v.x += q.x; v.y += q.y; v.z += q.z; v.w += q.w;
    *(float4*)(p.out + row * p.N + n) = v;
}

}  // namespace

const char* patch_embed_refusal(const PatchEmbedParams& p) {
    if (!p.img || !p.W || !p.out) return "null operand";
    if ((p.pos == nullptr) != (p.kv == nullptr)) return "pos and kv come together (both or neither)";
    if (p.kc != 16 && p.kc != 32 && p.kc != 64 && p.kc != 128) return "kc must be 16, 32, 64 or 128 (a patch row is a whole number of 64-byte K steps of a 128-wide image)";
    if (p.kt < 1 || p.kt > 32) return "kt must be 1..32";
    if (p.B < 1 || p.Tt < 1 || p.N < 4) return "bad shape";
    if (p.B > 65535) return "B above 65535";
    if (p.N & 3) return "N must be a multiple of 4 (vector stores)";
    if (p.vshift != __builtin_ctz(IMG_W / p.kc) || p.sshift != __builtin_ctz(p.kc / 16)) return "vshift / sshift do not belong to kc (internal)";
    if (p.img_bs & 3) return "img batch stride must be a multiple of 4 floats";
    if (p.img_bs < (long)p.Tt * p.kt * IMG_W) return "img batch stride is smaller than Tt * kt image rows";
    if (((uintptr_t)p.img | (uintptr_t)p.W | (uintptr_t)p.bias | (uintptr_t)p.pos | (uintptr_t)p.out) & 15) return "operands must be 16-byte aligned";
    if ((uintptr_t)p.kv & 3) return "kv must be 4-byte aligned";
    const unsigned long a_span = (unsigned long)p.Tt * p.kt * IMG_W * 4ul;
    const unsigned long w_span = (unsigned long)p.N * (unsigned long)(p.kt * p.kc) * 4ul;
    if (a_span >= (1ul << 32) - 64 || w_span >= (1ul << 32) - 64) return "an operand is not addressable with 32-bit offsets";
    const long T = (long)p.Tt << p.vshift;
    if (T > 0x7fffffffL / 2) return "too many tokens per utterance";
    const long tiles = (long)p.B * ((T + 63) / 64) * ((p.N + BN - 1) / BN);
    if (tiles > 0x7fffffffL) return "too many tiles";
    return nullptr;
}

void patch_embed_geometry(PatchEmbedParams& p) {
    p.vshift = p.sshift = 0;
    if (p.kc == 16 || p.kc == 32 || p.kc == 64 || p.kc == 128) {
        p.vshift = __builtin_ctz(IMG_W / p.kc);
        p.sshift = __builtin_ctz(p.kc / 16);
    }
}

hipError_t launch_patch_embed(const PatchEmbedParams& p, hipStream_t stream) {
    if (patch_embed_refusal(p)) return hipErrorInvalidValue;
    // 128-row tiles once they fill the chip, 64-row tiles for short or few utterances (the bits are the same)
    const long T = (long)p.Tt << p.vshift;
    const long t128 = (long)p.B * ((T + 127) / 128) * ((p.N + BN - 1) / BN);
    return (T > 64 && t128 >= device_cus()) ? go<2>(p, stream) : go<1>(p, stream);
}

size_t patch_embed_rows_elems(const PatchEmbedParams& p) { return (size_t)p.B * ((size_t)p.Tt << p.vshift) * (size_t)(p.kt * p.kc); }

hipError_t launch_patch_embed_two_step(const PatchEmbedParams& p, float* rows, hipStream_t stream) {
    if (patch_embed_refusal(p) || !rows || ((uintptr_t)rows & 15)) return hipErrorInvalidValue;
    const long T = (long)p.Tt << p.vshift, M = (long)p.B * T;
    const int K = p.kt * p.kc;
    if (M > 0x7fffffffL / 4) return hipErrorInvalidValue;
    const long g1 = (M * (K >> 2) + 255) / 256, g2 = (M * (p.N >> 2) + 255) / 256;
    if (g1 > 0x7fffffffL || g2 > 0x7fffffffL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(patch_gather_kernel, dim3((unsigned)g1), dim3(256), 0, stream, p, rows);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    GemmParams g{};
    g.A = rows;
    g.lda = K;
    g.W = p.W;
    g.bias = p.bias;
    g.M = (int)M;
    g.N = p.N;
    g.K = K;
    g.batches = 1;
    g.out32 = p.out;
    g.ldo = p.N;
    e = launch_gemm(0 /* fp32 */, g, stream);
    if (e != hipSuccess) return e;
    if (p.pos) hipLaunchKernelGGL(patch_pos_kernel, dim3((unsigned)g2), dim3(256), 0, stream, p);
    return hipGetLastError();
}

}  // namespace s3
