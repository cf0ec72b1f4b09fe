// convf22.hip — exact-fp32 Conv1d(C, C, k = 3, stride = 2) on channel-last activations in the two-output (Winograd-class)
// form: 5 C x C block products per PAIR of outputs where the implicit GEMM (gemmt.hip) needs 6.  Same fp32 operands, fp32
// products and fp32 accumulation; only the association differs.  Per pair u of outputs (W0 | W1 | W2 the tap slices of
// the packed weight W[n][j*C + c], WP = fl(W0 + W2) packed at s3enc_create):
//
//   P[u]      = WP . x[4u+2]
//   y[2u]     = W1 . x[4u+1] + W0 . (x[4u]   - x[4u+2]) + P[u]
//   y[2u+1]   = W1 . x[4u+3] + W2 . (x[4u+4] - x[4u+2]) + P[u]
//
// Tile: 128 outputs (64 pairs, starting at an even output m0 of one utterance: a pair never straddles a tile or an
// utterance) x 128 columns, 4 waves.  Wave (pb, wc) owns pairs pb*32 .. +32 and columns wc*64 .. +64: both parities of its
// pairs (acc_e / acc_o) and their shared P (acc_p) — 6 x 16 accumulator VGPRs, no exchange of P between waves.
// Two K phases of C/16 64-byte steps each, on gemmt.hip's machinery (LDS-DMA through a buffer descriptor, XOR-swizzled
// planes, the half-step fragment schedule with one wait + barrier per step, XCD-aware tile order, transposed vector
// epilogue):
//   A (odd tap):    rows x[2t+1] parity-sorted (LDS row r < 64: t = m0 + 2r, else t = m0 + 2(r-64) + 1) and W1.
//                   16 MFMAs per half-step: acc_e += x[4u+1] W1, acc_o += x[4u+3] W1.
//   B (difference + shared product): E_odd[j] = x[2m0 + 4j + 2], E_even[j] = x[2m0 + 4j] (j <= 64: the 65th row sits in
//                   its own 16-row piece at the plane's end), W0, W2, WP.  24 MFMAs per half-step:
//                   acc_e += (E_even[j] - E_odd[j]) W0, acc_o += (E_even[j+1] - E_odd[j]) W2, acc_p += E_odd[j] WP.
// MFMAs per 64-byte step and wave: 32 + 48 = 80 per C where the direct 128 x 128 tile issues 96.
// Frames past the last one an output < M reads (2M) are clamped to it; their results are never stored.
#include <type_traits>

#include "kernels.h"

namespace s3 {

namespace {

constexpr int BM = 128, BN = 128, ROWB = 64;
// phase B plane rows: E_odd [0, 64), E_even[0..63] [64, 128), W0 [128, 256), W2 [256, 384), WP [384, 512), E_even[64..79] [512, 528)
constexpr int R_EO = 0, R_EE = 64, R_W0 = 128, R_W2 = 256, R_WP = 384, R_EE64 = 512, ROWS = 528;
// phase A plane rows: x[2t+1] [0, 128), W1 [128, 256)
constexpr int R_XA = 0, R_W1 = 128;
constexpr int PLANE = ROWS * ROWB;  // 33 KiB; two planes: 66 KiB, two workgroups per CU
typedef int i32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ uint4 sub4(const uint4& a, const uint4& b) {
    return make_uint4(__float_as_uint(__uint_as_float(a.x) - __uint_as_float(b.x)), __float_as_uint(__uint_as_float(a.y) - __uint_as_float(b.y)),
                      __float_as_uint(__uint_as_float(a.z) - __uint_as_float(b.z)), __float_as_uint(__uint_as_float(a.w) - __uint_as_float(b.w)));
}
__device__ __forceinline__ void mma4(const uint4& a, const uint4& b, f32x16& c) {  // k order x, y, z, w (as gemmt.hip)
    c = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.x), __uint_as_float(b.x), c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.y), __uint_as_float(b.y), c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.z), __uint_as_float(b.z), c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.w), __uint_as_float(b.w), c, 0, 0, 0);
}

__global__ __launch_bounds__(256, 2) void conv_f22_kernel(ConvF22Params p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int pb = wave >> 1, wc = wave & 1;
    const int half = lane >> 5;
    const int l31 = lane & 31;
    const int C = p.C, N = p.C;

    int tile;
    {
        const int nwg = gridDim.x, wg = blockIdx.x;
        const int q8 = nwg >> 3, r8 = nwg & 7, xcd = wg & 7, loc = wg >> 3;
        tile = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + loc;
    }
    const int n_tiles = (N + BN - 1) / BN;
    const int m_tiles = (p.M + BM - 1) / BM;
    const int tn = tile % n_tiles;
    const int tmb = tile / n_tiles;
    const int tm = tmb % m_tiles, b = tmb / m_tiles;
    const int m0 = tm * BM, n0 = tn * BN;
    const int nc = C >> 4;  // 64-byte steps per phase (launcher: C is a multiple of 32, so phase B starts in slot 0)

    // ---- LDS-DMA sources: pass i of wave w lands rows 16 w + 64 i + lane / 4 (pass 8: wave 0 only, rows 512..527) ----
    i32x4 rsrc_x, rsrc_w, rsrc_p;
    {
        const unsigned long ux = (unsigned long)(p.x + (long)b * p.x_bs), uw = (unsigned long)p.W, up = (unsigned long)p.WP;
        rsrc_x = (i32x4){(int)__builtin_amdgcn_readfirstlane((unsigned)ux), (int)__builtin_amdgcn_readfirstlane((unsigned)(ux >> 32)), -1, 0x00020000};
        rsrc_w = (i32x4){(int)__builtin_amdgcn_readfirstlane((unsigned)uw), (int)__builtin_amdgcn_readfirstlane((unsigned)(uw >> 32)), -1, 0x00020000};
        rsrc_p = (i32x4){(int)__builtin_amdgcn_readfirstlane((unsigned)up), (int)__builtin_amdgcn_readfirstlane((unsigned)(up >> 32)), -1, 0x00020000};
    }
    const int src_slot = (lane & 3) ^ ((lane >> 4) & 3);
    const int fmax = 2 * p.M;  // the last frame an output < M reads
    auto xoff = [&](int f) { return (unsigned)(f < fmax ? f : fmax) * (unsigned)(C * 4) + src_slot * 16; };
    auto woff = [&](int n, int tap) {
        n = n < N ? n : N - 1;
        return (unsigned)n * (unsigned)(3 * C * 4) + (unsigned)(tap * C * 4) + src_slot * 16;
    };
    const int rl = 16 * wave + (lane >> 2);  // row of pass 0
    unsigned va[4], vb[9];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int r = rl + 64 * i;
        va[i] = xoff(2 * (m0 + 2 * (r & 63) + (r >> 6)) + 1);
    }
#pragma unroll
    for (int i = 2; i < 4; ++i) va[i] = woff(n0 + rl + 64 * i - R_W1, 1);
    vb[0] = xoff(2 * m0 + 4 * rl + 2);
    vb[1] = xoff(2 * m0 + 4 * (rl + 64 - R_EE));
    vb[2] = woff(n0 + rl + 128 - R_W0, 0);
    vb[3] = woff(n0 + rl + 192 - R_W0, 0);
    vb[4] = woff(n0 + rl + 256 - R_W2, 2);
    vb[5] = woff(n0 + rl + 320 - R_W2, 2);
    {
        int n6 = n0 + rl + 384 - R_WP, n7 = n0 + rl + 448 - R_WP;
        n6 = n6 < N ? n6 : N - 1;
        n7 = n7 < N ? n7 : N - 1;
        vb[6] = (unsigned)n6 * (unsigned)(C * 4) + src_slot * 16;
        vb[7] = (unsigned)n7 * (unsigned)(C * 4) + src_slot * 16;
    }
    vb[8] = xoff(2 * m0 + 4 * (64 + (lane >> 2)));  // wave 0: E_even[64..79]
    const unsigned lds0 = __builtin_amdgcn_readfirstlane((unsigned)(uintptr_t)(__attribute__((address_space(3))) char*)smem) + wave * 1024;
    auto dma = [&](unsigned vo, const i32x4& rs, unsigned dst, unsigned soff) {
        asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, %3 offen lds"
                     :
                     : "s"(dst), "v"(vo), "s"(rs), "s"(soff)
                     : "memory");
    };
    // plane of global step s (s < nc: phase A, channel chunk s; else phase B, chunk s - nc) into LDS slot `slot`
    auto issue = [&](int s, int slot) {
        const unsigned d0 = lds0 + slot * PLANE;
        if (s < nc) {
            const unsigned kb = (unsigned)s * ROWB;
#pragma unroll
            for (int i = 0; i < 4; ++i) dma(va[i], i < 2 ? rsrc_x : rsrc_w, d0 + i * 4096, kb);
        } else {
            const unsigned kb = (unsigned)(s - nc) * ROWB;
#pragma unroll
            for (int i = 0; i < 8; ++i) dma(vb[i], i < 2 ? rsrc_x : (i < 6 ? rsrc_w : rsrc_p), d0 + i * 4096, kb);
            if (wave == 0) dma(vb[8], rsrc_x, d0 + 8 * 4096, kb);
        }
    };

    // ---- fragment addresses: row `row` of the plane, 16-byte slot (half * 2 + q) ^ swizzle(row) ----
    auto rowoff = [&](int row, int q) { return row * ROWB + (((half * 2 + q) ^ ((row >> 2) & 3)) << 4); };
    const int ee1 = pb * 32 + l31 + 1 < 64 ? R_EE + pb * 32 + l31 + 1 : R_EE64;  // E_even[j + 1]
    int offA[2][4], offB[2][9];  // [q][a0, a1, b0, b1] / [q][a0, a1, a2, b0..b5]
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        offA[q][0] = rowoff(R_XA + pb * 32 + l31, q);
        offA[q][1] = rowoff(R_XA + 64 + pb * 32 + l31, q);
        offB[q][0] = rowoff(R_EO + pb * 32 + l31, q);
        offB[q][1] = rowoff(R_EE + pb * 32 + l31, q);
        offB[q][2] = rowoff(ee1, q);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            offA[q][2 + j] = rowoff(R_W1 + wc * 64 + j * 32 + l31, q);
            offB[q][3 + j] = rowoff(R_W0 + wc * 64 + j * 32 + l31, q);
            offB[q][5 + j] = rowoff(R_W2 + wc * 64 + j * 32 + l31, q);
            offB[q][7 + j] = rowoff(R_WP + wc * 64 + j * 32 + l31, q);
        }
    }

    f32x16 acc_e[2], acc_o[2], acc_p[2];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc_e[j][r] = acc_o[j][r] = acc_p[j][r] = 0.f;

    struct Frag {
        uint4 v[9];  // phase A: a0, a1, b0, b1; phase B: a0 (E_odd), a1 (E_even), a2 (E_even + 1), W0 x 2, W2 x 2, WP x 2
    };
    auto read = [&](Frag& f, bool phb, int slot, int q) {
        const char* base = smem + slot * PLANE;
        if (!phb) {
#pragma unroll
            for (int i = 0; i < 4; ++i) f.v[i] = *(const uint4*)(base + offA[q][i]);
        } else {
#pragma unroll
            for (int i = 0; i < 9; ++i) f.v[i] = *(const uint4*)(base + offB[q][i]);
        }
    };
    // MFMA group g of a half-step (phase A: 4 groups, phase B: 6 groups of 4 MFMAs)
    auto mma = [&](const Frag& f, bool phb, int g) {
        if (!phb) {
            if (g < 2) mma4(f.v[0], f.v[2 + g], acc_e[g]);
            else mma4(f.v[1], f.v[g], acc_o[g - 2]);
        } else {
            if (g < 2) mma4(sub4(f.v[1], f.v[0]), f.v[3 + g], acc_e[g]);
            else if (g < 4) mma4(sub4(f.v[2], f.v[0]), f.v[3 + g], acc_o[g - 2]);
            else mma4(f.v[0], f.v[3 + g], acc_p[g - 4]);
        }
    };

    issue(0, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    issue(1, 1);
    Frag f0, f1;
    read(f0, false, 0, 0);
    // ---- K loop (gemmt.hip's schedule).  Step s multiplies plane s (LDS slot s & 1):
    //        read F1 = (s, second half) | MFMAs on F0 = (s, first half) | wait + barrier | first group of F1 | DMA plane s+2
    //        into plane s's slot | read F0 = (s+1, first half) | rest of F1.                                        ----
    const int ns = 2 * nc;
    auto step = [&](int s, int slot, auto phb_c, auto next_phb_c) {  // (compile-time phases: a Frag must never be indexed at run time)
        constexpr bool phb = decltype(phb_c)::value, next_phb = decltype(next_phb_c)::value;
        constexpr int ng = phb ? 6 : 4;
        read(f1, phb, slot, 1);
#pragma unroll
        for (int g = 0; g < ng; ++g) mma(f0, phb, g);
        __builtin_amdgcn_sched_barrier(0);
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
        mma(f1, phb, 0);
        __builtin_amdgcn_sched_barrier(0);
        if (s + 2 < ns) issue(s + 2, slot);
        if (s + 1 < ns) read(f0, next_phb, slot ^ 1, 0);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int g = 1; g < ng; ++g) mma(f1, phb, g);
    };
    const std::false_type PA{};
    const std::true_type PB{};
    int s = 0;
    for (; s + 2 < nc; s += 2) {
        step(s, 0, PA, PA);
        step(s + 1, 1, PA, PA);
    }
    step(s, 0, PA, PA);
    step(s + 1, 1, PA, PB);  // the last phase-A step reads phase B's first fragments
    for (s = nc; s < ns; s += 2) {
        step(s, 0, PB, PB);
        step(s + 1, 1, PB, PB);
    }
    // the last step's barrier ordered every wave's fragment reads before this point: the planes are free for the epilogue

    // ---- epilogue: acc[j][r] is (pair row = pb*32 + (r&3) + 8*(r>>2) + 4*half, col = wc*64 + j*32 + l31); output row of pair
    //      row i and parity q: t = m0 + 2 (pb*32 + i) + q.  y = acc_(e|o) + acc_p, then gemmt.hip's transposed vector store ----
    const int limit = p.row_limit ? p.row_limit[b] : p.M;
    const long ob = (long)b * p.o_bs;
    float* stg = (float*)(smem + wave * 8192);
    const int c4 = (lane & 15) * 4;
    const int n = n0 + wc * 64 + c4;
    const bool n_ok = n < N;
    float4 bias4 = make_float4(0.f, 0.f, 0.f, 0.f);
    if (p.bias && n_ok) bias4 = *(const float4*)(p.bias + n);
#pragma unroll
    for (int q = 0; q < 2; ++q) {
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r)
                stg[((r & 3) + 8 * (r >> 2) + 4 * half) * 64 + j * 32 + l31] = (q ? acc_o[j][r] : acc_e[j][r]) + acc_p[j][r];
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            const int row = t * 4 + (lane >> 4);
            float4 v = *(const float4*)(stg + row * 64 + c4);
            const int m = m0 + 2 * (pb * 32 + row) + q;
            if (m < p.M && n_ok) {
                v.x += bias4.x; v.y += bias4.y; v.z += bias4.z; v.w += bias4.w;
                if (p.act == 2) {
                    gelu_fast4(v);
                } else if (p.act) {
                    v.x = gelu_erf(v.x); v.y = gelu_erf(v.y); v.z = gelu_erf(v.z); v.w = gelu_erf(v.w);
                }
                if (m >= limit) v = make_float4(0.f, 0.f, 0.f, 0.f);
                *(float4*)(p.out + ob + (long)m * C + n) = v;
            }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    }
}

// the part of the refusal that depends on C and the buffers only, never on B, M or a tile picker
const char* ineligible(const ConvF22Params& p) {
    if (!tuning().conv_f22) return "the tuning key conv_f22 is 0 (the two-output kernel is switched off)";
    if (!p.x || !p.W || !p.WP || !p.out) return "null operand";
    if (p.C < 32 || (p.C & 31)) return "C must be a multiple of 32 (each K phase is an even number of 64-byte steps)";
    if ((p.x_bs & 3) || (p.o_bs & 3)) return "batch strides must be multiples of 4 floats (vector accesses)";
    const uintptr_t al = (uintptr_t)p.x | (uintptr_t)p.W | (uintptr_t)p.WP | (uintptr_t)p.out | (uintptr_t)p.bias;
    if (al & 15) return "operands must be 16-byte aligned";
    // 32-bit buffer offsets: frames up to 2M of an utterance, the whole (C, 3C) weight
    const unsigned long x_span = ((unsigned long)p.x_bs + (unsigned long)p.C) * 4ul;
    const unsigned long w_span = (unsigned long)p.C * 3ul * (unsigned long)p.C * 4ul;
    if (x_span >= (1ul << 32) - 64 || w_span >= (1ul << 32) - 64) return "an operand is not addressable with 32-bit offsets";
    return nullptr;
}

}  // namespace

// Batch-independent by construction: it depends on C and the buffers only, never on B, M or a tile picker.
bool conv_f22_eligible(const ConvF22Params& p) { return !ineligible(p); }

const char* conv_f22_refusal(const ConvF22Params& p) {
    if (const char* why = ineligible(p)) return why;
    if (p.M < 1 || p.batches < 1) return "bad shape";
    if (p.act < 0 || p.act > 2) return "act must be 0 (none) or 1 (GELU)";
    if ((2L * p.M + 1) * p.C > p.x_bs) return "x_bs is smaller than (2M + 1) C: frame 2M must exist";
    if ((long)p.M * p.C > p.o_bs) return "o_bs is smaller than M C";
    const long tiles = (long)p.batches * ((p.M + BM - 1) / BM) * ((p.C + BN - 1) / BN);
    if (tiles > 0x7fffffffL) return "too many tiles";
    return nullptr;
}

hipError_t launch_conv_f22(const ConvF22Params& p0, hipStream_t stream) {
    ConvF22Params p = p0;
    if (p.M <= 0 || p.batches <= 0) return hipSuccess;
    if (conv_f22_refusal(p)) return hipErrorInvalidValue;
    if (p.act == 1 && tuning().gelu32 == 1) p.act = 2;  // as launch_gemm: the one-transcendental GELU of the fp32 mode
    constexpr int lds = 2 * PLANE;
    hipError_t e = ensure_dynamic_lds<conv_f22_kernel>(lds);
    if (e != hipSuccess) return e;
    dim3 grid(((p.M + BM - 1) / BM) * ((p.C + BN - 1) / BN) * p.batches);
    hipLaunchKernelGGL(conv_f22_kernel, grid, dim3(256), lds, stream, p);
    return hipGetLastError();
}

}  // namespace s3
