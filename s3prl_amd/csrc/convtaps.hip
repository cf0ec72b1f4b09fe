// convtaps.hip — exact-fp32 stride-1 Conv1d over channel-last rows as an implicit GEMM whose K walk may skip a run of taps in the
// middle of the kernel: NPC's masked convolutions (upstream/npc/npc.py:21-52; k = 15 with 8 / 6 / 4 / 2 live taps at the released
// shape) and, as single runs, its k = 3 and 1 x 1 convolutions (npc.py:55-93).
//
//   out[b][t][n] = act( sum_{j live} sum_c x[b][t + j - pad][c] * w[n][c][j] + bias[n] [+ res[b][t][n]] )
//
// Operand geometry (cpc.hip's): every utterance is P zero rows, its T data rows, P zero rows, so a window that hangs over either
// end reads zeros and never a neighbour; `src` points at the row tap 0 of output row 0 reads.  A tap run is then ONE contiguous K
// segment of ntaps * C floats of A.  The K walk is run 0 = taps [0, taps0), then run 1 = taps [taps0 + gap, taps0 + gap + taps1):
// between them the A offset jumps by gap * C floats and the W offset does not — the weights are packed with the live taps only,
// (N, (taps0 + taps1) * C) tap-major.  Masked taps are neither fetched nor multiplied.  C is a multiple of 16: a tap is a whole
// number of 64-byte K steps.
//
// Schedule: gemmt.hip's, for the same arithmetic (v_mfma_f32_32x32x2_f32 on 64-byte K steps, LDS-DMA staging of lane-linear planes
// with the XOR swizzle applied to the source slot, two register sets of fragments around the step's one barrier) on a (128 | 64) x
// 128 tile per (utterance, m-tile, n-tile).  Per output element the order is fixed — runs ascending, taps ascending, the tile GEMM's
// order inside a step — so a row's bits depend neither on B, nor on its place in the batch, nor on the tile height or the n-tile.
// gfx950's fp32 MFMA is an fmaf chain: the same kernel run over all k taps with the masked weights stored as zeros gives equal values
// (tests/test_conv_taps_gpu.py).
//
// Epilogue, one pass, plain vector stores: v = act(acc + bias [+ res]) with the residual BEFORE the activation (npc.py:91-93), written
// to up to three places: the next layer's bordered operand (data rows only — the caller points `dst` at the first data row, the
// border rows are never touched), a contiguous state slot, and a running sum (sum = init ? v : sum + v).
#include "kernels.h"

namespace s3 {

namespace {

constexpr int BN = 128, ROWB = 64;
typedef int i32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ void mma4(const uint4& a, const uint4& b, f32x16& c) {  // k order x, y, z, w (gemm_kernel<float>'s)
    c = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.x), __uint_as_float(b.x), c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.y), __uint_as_float(b.y), c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.z), __uint_as_float(b.z), c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.w), __uint_as_float(b.w), c, 0, 0, 0);
}

__device__ __forceinline__ float act1(float v, int act) {
    if (act == 1) return v < 0.f ? 0.f : v;  // ReLU; a NaN stays a NaN
    if (act == 2) return tanhf(v);           // libm: odd, exact at 0, x for tiny x, +-1 when saturated
    return v;
}

template <int TM>
__global__ __launch_bounds__(256, 2) void conv_taps_kernel(ConvTapsParams p) {
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

    const int n_tiles = (p.N + BN - 1) / BN;
    const int m_tiles = (p.T + BM - 1) / BM;
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
    const int Kw = (p.taps0 + p.taps1) * p.C;     // floats per weight row
    const int nk0 = (p.taps0 * p.C) >> 4;         // 64-byte steps of run 0
    const int nk = Kw >> 4;
    const unsigned jump = (unsigned)p.gap * (unsigned)p.C * 4u;  // A bytes skipped between the runs

    i32x4 rsrc_a, rsrc_w;
    {
        const unsigned long ua = (unsigned long)(p.src + (long)b * p.src_bs), uw = (unsigned long)p.W;
        rsrc_a = (i32x4){(int)__builtin_amdgcn_readfirstlane((unsigned)ua), (int)__builtin_amdgcn_readfirstlane((unsigned)(ua >> 32)),
                         -1, 0x00020000};
        rsrc_w = (i32x4){(int)__builtin_amdgcn_readfirstlane((unsigned)uw), (int)__builtin_amdgcn_readfirstlane((unsigned)(uw >> 32)),
                         -1, 0x00020000};
    }
    // rows past T / N are clamped to the last one (never stored): every fetch stays inside the utterance's bordered rows
    const int src_slot = (lane & 3) ^ ((lane >> 4) & 3);
    unsigned voff[NPASS];
#pragma unroll
    for (int i = 0; i < NPASS; ++i) {
        if (i < APASS) {
            int r = m0 + 16 * wave + 64 * i + (lane >> 2);
            r = r < p.T ? r : p.T - 1;
            voff[i] = (unsigned)r * (unsigned)(p.C * 4) + src_slot * 16;
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
        const unsigned ka = kw + (kt >= nk0 ? jump : 0u);
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

    // ---- epilogue: each 32 x 64 block through a wave-private LDS transpose, then 16 lanes x 4 columns per row ----
    float* stg = (float*)(smem + wave * 8192);
    const int c4 = (lane & 15) * 4;
    const int n = n0 + wc * 64 + c4;
    const bool n_ok = n < p.N;
    float4 bias4 = make_float4(0.f, 0.f, 0.f, 0.f);
    if (p.bias && n_ok) bias4 = *(const float4*)(p.bias + n);
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
            if (m < p.T && n_ok) {
                v.x += bias4.x; v.y += bias4.y; v.z += bias4.z; v.w += bias4.w;
                if (p.res) {
                    const float4 rs = *(const float4*)(p.res + (long)b * p.res_bs + (long)m * p.ld_res + n);
                    v.x += rs.x; v.y += rs.y; v.z += rs.z; v.w += rs.w;
                }
                v.x = act1(v.x, p.act); v.y = act1(v.y, p.act); v.z = act1(v.z, p.act); v.w = act1(v.w, p.act);
                if (p.dst) *(float4*)(p.dst + (long)b * p.dst_bs + (long)m * p.ld_dst + n) = v;
                if (p.state) *(float4*)(p.state + (long)b * p.state_bs + (long)m * p.ld_state + n) = v;
                if (p.sum) {
                    float4* sp = (float4*)(p.sum + (long)b * p.sum_bs + (long)m * p.ld_sum + n);
                    if (!p.sum_init) {
                        const float4 s = *sp;
                        v.x += s.x; v.y += s.y; v.z += s.z; v.w += s.w;
                    }
                    *sp = v;
                }
            }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    }
}

template <int TM>
hipError_t go(const ConvTapsParams& p, hipStream_t stream) {
    constexpr int BM = 64 * TM;
    constexpr int plane2 = 2 * (BM + BN) * ROWB;
    constexpr int lds = plane2 > 4 * 8192 ? plane2 : 4 * 8192;
    hipError_t e = ensure_dynamic_lds<conv_taps_kernel<TM>>(lds);
    if (e != hipSuccess) return e;
    dim3 grid(((p.T + BM - 1) / BM) * ((p.N + BN - 1) / BN) * p.B);
    hipLaunchKernelGGL((conv_taps_kernel<TM>), grid, dim3(256), lds, stream, p);
    return hipGetLastError();
}

}  // namespace

void pack_conv_taps(const float* w, int N, int C, int k, int mask, bool dense, std::vector<float>& out) {
    const int head = (k - mask) / 2, tail = head + mask;
    const int live = dense ? k : k - mask;
    out.assign((size_t)N * live * C, 0.f);
    for (int n = 0; n < N; ++n) {
        int li = 0;
        for (int j = 0; j < k; ++j) {
            const bool masked = j >= head && j < tail;
            if (masked && !dense) continue;
            if (!masked)
                for (int c = 0; c < C; ++c) out[((size_t)n * live + li) * C + c] = w[((size_t)n * C + c) * k + j];
            ++li;
        }
    }
}

const char* conv_taps_refusal(const ConvTapsParams& p) {
    if (!p.src || !p.W) return "null operand";
    if (!p.dst && !p.state && !p.sum) return "no destination";
    if (p.B < 1 || p.T < 1 || p.N < 4 || p.C < 16) return "bad shape";
    if (p.B > 65535) return "B above 65535";
    if (p.C & 15) return "C must be a multiple of 16 (a tap is a whole number of 64-byte K steps)";
    if (p.N & 3) return "N must be a multiple of 4 (vector stores)";
    if (p.taps0 < 0 || p.taps1 < 0 || p.gap < 0 || p.taps0 + p.taps1 < 1) return "no live tap";
    if (p.act < 0 || p.act > 2) return "act must be 0 (none), 1 (ReLU) or 2 (tanh)";
    if (p.src_bs & 3) return "src batch stride must be a multiple of 4 floats";
    if ((p.ld_dst | p.dst_bs | p.ld_state | p.state_bs | p.ld_sum | p.sum_bs | p.ld_res | p.res_bs) & 3)
        return "row and batch strides must be multiples of 4 floats (vector accesses)";
    if ((p.dst && p.ld_dst < p.N) || (p.state && p.ld_state < p.N) || (p.sum && p.ld_sum < p.N) || (p.res && p.ld_res < p.N))
        return "a row stride is smaller than N";
    if (((uintptr_t)p.src | (uintptr_t)p.W | (uintptr_t)p.bias | (uintptr_t)p.res | (uintptr_t)p.dst | (uintptr_t)p.state | (uintptr_t)p.sum) & 15)
        return "operands must be 16-byte aligned";
    const unsigned long a_span = ((unsigned long)p.T + p.taps0 + p.gap + p.taps1) * (unsigned long)p.C * 4ul;
    const unsigned long w_span = (unsigned long)p.N * (unsigned long)(p.taps0 + p.taps1) * (unsigned long)p.C * 4ul;
    if (a_span >= (1ul << 32) - 64 || w_span >= (1ul << 32) - 64) return "an operand is not addressable with 32-bit offsets";
    const long tiles = (long)p.B * ((p.T + 63) / 64) * ((p.N + BN - 1) / BN);
    if (tiles > 0x7fffffffL) return "too many tiles";
    return nullptr;
}

hipError_t launch_conv_taps(const ConvTapsParams& p, hipStream_t stream) {
    if (conv_taps_refusal(p)) return hipErrorInvalidValue;
    // 128-row tiles once they fill the chip, 64-row tiles for short or few utterances (the bits are the same)
    const long t128 = (long)p.B * ((p.T + 127) / 128) * ((p.N + BN - 1) / BN);
    return (p.T > 64 && t128 >= device_cus()) ? go<2>(p, stream) : go<1>(p, stream);
}

}  // namespace s3
