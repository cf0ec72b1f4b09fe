// rnnb.hip — the batch-shared, bidirectional, length-aware LSTM step, exact fp32, for the wide recurrent upstreams (DeCoAR:
// upstream/decoar/decoar.py — a forward and a backward stack of unidirectional nn.LSTM at H = 1024 on packed sequences).
// rnn.hip gives every utterance workgroups of its own, and each of them streams W_hh every step; at H = 1024 the matrix is 16 MiB per
// layer and direction, so here it is read ONCE per step for the whole batch: the recurrence h_{t-1} (B x H) against W_hh (4H x H) is a
// small GEMM per step, on the exact-fp32 MFMA (v_mfma_f32_32x32x2_f32: bit for bit a k-ordered fmaf chain).
//
// Launch form: one launch per time step on a (S, 2) grid, S = H / 8.  The kernel boundary is the only synchronisation: no flag in
// global memory, no spin wait, no cooperative launch.  Workgroup (s, d) owns the U = 8 hidden units [8 s, 8 s + 8) of direction d
// (0 = the forward stack, 1 = the backward stack) with all four gate rows — 32 rows, one MFMA tile (local row = 8 * gate + unit) — for ALL
// utterances.  At H = 1024 that is 256 workgroups, one per CU; consecutive workgroup ids go round-robin over the XCDs, and a slice's
// rows (contiguous in the packed image, 128 KiB at H = 1024) are asked for by the same workgroup id at every step.
//
// Product: the four waves split K = H into quarters; wave w runs k in [w H / 4, (w + 1) H / 4) as one chain of MFMAs per 32-wide batch
// tile (A = the 32 gate rows, B = h of 32 utterances), starting from zero.  Inside a block of 8 k the pairs are (j, j + 4), j = 0..3, so
// that a lane's operands for four MFMAs are ONE 16-byte load of W and one of h.  The four partial tiles meet in LDS and a gate is
// pre + ((p0 + p1) + (p2 + p3)): the order is a function of H alone — an utterance's bits depend neither on B, nor on its column, nor
// on the other lengths (the MFMA's columns are independent), and S is not tunable.  Batch tiles are walked inside the workgroup: the W
// registers of a k block feed every tile's MFMAs, so W_hh is read once per step whatever B is (B <= RNNB_B_MAX = 128, four tiles).
//
// Where h lives: every element of h_{t-1} is used by a workgroup exactly once per step (its 32 rows are a single MFMA tile), so a copy
// in LDS (128 KiB for 32 utterances at H = 1024) would add a hop and save nothing: h is streamed from L2 as the MFMA's other operand.
// The state buffer is laid out for that: [H / 8][Bp][8] per direction and ping-pong half (Bp = B rounded up to 32), so that a wave's
// load is 1 KiB of consecutive bytes and the workgroup's cell update writes one contiguous Bp x 8 block.  c has the same layout.
// Columns of dead or padding utterances compute on whatever the buffer holds and are never stored.
//
// Time direction without flips: at step t direction 0 handles row t of every utterance with len[b] > t, direction 1 row
// len[b] - 1 - t; both read `pre` and write `out` at that row.  Direction d writes columns [d H, (d + 1) H) of a row of stride ldo; the
// t = 0 launch writes rows [len[b], T) of both halves as zeros with 16-byte stores (pad_packed_sequence).  At t = 0 the product is
// skipped (h = 0).  Cell update: the same fmaf expressions and accurate expf / tanhf as rnn.hip.
//
// Cost per step at H = 1024, B = 32, both directions — DERIVED: 537 MFLOP, 3.4 us at the 157 TF fp32 matrix peak; each workgroup
// reads 128 KiB of W and 128 KiB of h from L2, ~1.9 us at the ~135 GB/s per CU rnn.hip quotes, under the MFMA time.
// MEASURED (profiles/decoar_fp32.md, tools/decoar_bench.py, B = 32): 11.4 us per step at H = 1024 and 6.5 us at H = 512, both
// directions per launch — at H = 512 that is 3.2 us per step and direction against 8.9 us for rnn.hip's step-split form (S = 8) and
// 33.2 us for its one-launch form.  About 4.8 us of a step do not scale with H^2; what they consist of has not been measured.
#include "kernels.h"

namespace s3 {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

__device__ __forceinline__ float sigmoid_acc(float x) { return 1.f / (1.f + expf(-x)); }

constexpr int RNNB_U = 8;         // hidden units per workgroup: 4 gates x 8 = the MFMA's 32 rows
constexpr int RNNB_LDP = 33;      // LDS row pitch of a partial tile

// NT: batch tiles of 32 (1, 2, 4); UNR: k blocks (of 8) per register stage — changes the schedule, not the order of any chain
template <int NT, int UNR>
__global__ __launch_bounds__(256) void rnnb_step_kernel(RnnbParams p) {
    __shared__ float part[4][32][RNNB_LDP];
    const int H = p.H, B = p.B, T = p.T, t = p.t;
    const int Bp = NT * 32;
    const int s = blockIdx.x, d = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* pre = d ? p.pre_bwd : p.pre_fwd;
    const long HB = (long)H * Bp;
    const float* hin = p.hbuf + ((long)d * 2 + ((t + 1) & 1)) * HB;  // written by the launch of step t - 1
    float* hout = p.hbuf + ((long)d * 2 + (t & 1)) * HB;
    float* cst = p.cbuf + (long)d * HB;

    f32x16 acc[NT];
#pragma unroll
    for (int n = 0; n < NT; ++n)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[n][i] = 0.f;

    if (t > 0) {
        const int KB = H >> 5;  // k blocks of this wave: (H / 4) / 8, a multiple of UNR
        const float4* W = (const float4*)(d ? p.w_bwd : p.w_fwd) + ((long)s * (H >> 3) + (long)wave * KB) * 64 + lane;
        // lane l of a k block: 16 bytes at [kb][column][4 (l >> 5)], column = 32 n + (l & 31)
        const float* hl = hin + ((long)wave * KB * Bp + (lane & 31)) * 8 + 4 * (lane >> 5);
        float4 wv[UNR], hv[NT][UNR], wn[UNR], hn[NT][UNR];
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
            wv[u] = W[(long)u * 64];
#pragma unroll
            for (int n = 0; n < NT; ++n) hv[n][u] = *(const float4*)(hl + ((long)u * Bp + 32 * n) * 8);
        }
        for (int kb = 0; kb < KB; kb += UNR) {
            const bool more = kb + UNR < KB;
            if (more) {  // the next stage's loads are in flight under this stage's MFMAs
#pragma unroll
                for (int u = 0; u < UNR; ++u) {
                    wn[u] = W[(long)(kb + UNR + u) * 64];
#pragma unroll
                    for (int n = 0; n < NT; ++n) hn[n][u] = *(const float4*)(hl + ((long)(kb + UNR + u) * Bp + 32 * n) * 8);
                }
            }
#pragma unroll
            for (int u = 0; u < UNR; ++u) {
#pragma unroll
                for (int n = 0; n < NT; ++n) {
                    acc[n] = __builtin_amdgcn_mfma_f32_32x32x2f32(wv[u].x, hv[n][u].x, acc[n], 0, 0, 0);
                    acc[n] = __builtin_amdgcn_mfma_f32_32x32x2f32(wv[u].y, hv[n][u].y, acc[n], 0, 0, 0);
                    acc[n] = __builtin_amdgcn_mfma_f32_32x32x2f32(wv[u].z, hv[n][u].z, acc[n], 0, 0, 0);
                    acc[n] = __builtin_amdgcn_mfma_f32_32x32x2f32(wv[u].w, hv[n][u].w, acc[n], 0, 0, 0);
                }
            }
            if (more) {
#pragma unroll
                for (int u = 0; u < UNR; ++u) {
                    wv[u] = wn[u];
#pragma unroll
                    for (int n = 0; n < NT; ++n) hv[n][u] = hn[n][u];
                }
            }
        }
    }

    // cell update: thread = (column tid >> 3, unit tid & 7) of the tile
    const int u = tid & 7, cb = tid >> 3;
    const int j = s * RNNB_U + u;
#pragma unroll
    for (int n = 0; n < NT; ++n) {
        if (n) __syncthreads();
#pragma unroll
        for (int i = 0; i < 16; ++i)  // C/D map of the 32x32 MFMA: column = lane & 31, row = (i & 3) + 8 (i >> 2) + 4 (lane >> 5)
            part[wave][(i & 3) + 8 * (i >> 2) + 4 * (lane >> 5)][lane & 31] = acc[n][i];
        __syncthreads();
        const int b = 32 * n + cb;
        if (b < B) {
            const int steps = min(max(p.len[b], 0), T);
            if (t < steps) {
                const long row = (long)b * T + (d ? steps - 1 - t : t);
                const float* pt = pre + row * p.ld_pre + j;
                float g[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int r = q * RNNB_U + u;
                    g[q] = pt[(long)q * H] + ((part[0][r][cb] + part[1][r][cb]) + (part[2][r][cb] + part[3][r][cb]));
                }
                const float gi = sigmoid_acc(g[0]), gf = sigmoid_acc(g[1]);
                const float gg = tanhf(g[2]), go = sigmoid_acc(g[3]);
                const long si = ((long)s * Bp + b) * RNNB_U + u;
                float c = t ? cst[si] : 0.f;
                c = fmaf(gf, c, gi * gg);
                const float h = go * tanhf(c);
                cst[si] = c;
                hout[si] = h;
                p.out[row * p.ldo + (long)d * H + j] = h;
            }
        }
    }

    if (t == 0) {  // pad_packed_sequence: this workgroup's 8 columns of the rows behind every utterance's length, once per layer
        for (int b = 0; b < B; ++b) {
            const int steps = min(max(p.len[b], 0), T);
            const int n = (T - steps) * 2;
            for (int i = tid; i < n; i += 256)
                *(float4*)(p.out + ((long)b * T + steps + (i >> 1)) * p.ldo + (long)d * H + s * RNNB_U + 4 * (i & 1)) =
                    make_float4(0.f, 0.f, 0.f, 0.f);
        }
    }
}

template <int NT, int UNR>
hipError_t rnnb_launch(const RnnbParams& p0, hipStream_t st) {
    RnnbParams p = p0;
    for (int t = 0; t < p.max_len; ++t) {
        p.t = t;
        hipLaunchKernelGGL((rnnb_step_kernel<NT, UNR>), dim3(p.H / RNNB_U, 2), dim3(256), 0, st, p);
    }
    return hipGetLastError();
}

template <int NT>
hipError_t rnnb_launch_u(const RnnbParams& p, hipStream_t st) {
    return (p.H >> 5) % 4 == 0 ? rnnb_launch<NT, 4>(p, st) : rnnb_launch<NT, 2>(p, st);  // H / 32 is even
}

}  // namespace

void pack_rnnb_whh(const float* w, int H, std::vector<float>& out) {
    const int S = H / RNNB_U, KB = H >> 3;
    out.resize((size_t)4 * H * H);
    for (int s = 0; s < S; ++s)
        for (int kb = 0; kb < KB; ++kb)
            for (int l = 0; l < 64; ++l) {
                const int r = l & 31, g = r >> 3, u = r & 7;
                const float* src = w + ((long)g * H + s * RNNB_U + u) * H + 8 * kb + 4 * (l >> 5);
                float* dst = out.data() + (((long)s * KB + kb) * 64 + l) * 4;
                for (int j = 0; j < 4; ++j) dst[j] = src[j];
            }
}

int rnnb_batch_pad(int B) { return B <= 32 ? 32 : (B <= 64 ? 64 : 128); }

size_t rnnb_state_elems(int B, int H) { return (size_t)2 * rnnb_batch_pad(B) * H; }

const char* rnnb_refusal(const RnnbParams& p) {
    if (p.H < 64 || (p.H & 63) || p.H > RNNB_H_MAX) return "H must be a multiple of 64, at most 1024";
    if (p.B > RNNB_B_MAX) return "B above 128 (the state buffers and the batch tiles of a workgroup)";
    if (!p.pre_fwd || !p.pre_bwd || !p.w_fwd || !p.w_bwd || !p.len || !p.out || !p.hbuf || !p.cbuf) return "null argument";
    if (p.ld_pre < 4L * p.H || p.ldo < 2L * p.H) return "ld_pre / ldo smaller than the row";
    if ((((uintptr_t)p.w_fwd) | ((uintptr_t)p.w_bwd) | ((uintptr_t)p.hbuf) | ((uintptr_t)p.out)) & 15)
        return "W_hh, out and the h state must be 16-byte aligned";
    if (p.ldo & 3) return "ldo must be a multiple of 4";
    if (p.max_len > p.T) return "max_len above T";
    return nullptr;
}

hipError_t launch_rnnb(const RnnbParams& p, hipStream_t st) {
    if (p.B <= 0 || p.T <= 0 || p.max_len <= 0) return hipSuccess;
    if (rnnb_refusal(p)) return hipErrorInvalidValue;
    if (p.B <= 32) return rnnb_launch_u<1>(p, st);
    if (p.B <= 64) return rnnb_launch_u<2>(p, st);
    return rnnb_launch_u<4>(p, st);
}

}  // namespace s3
