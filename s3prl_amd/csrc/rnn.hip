// rnn.hip — the recurrence of torch's nn.LSTM / nn.GRU (batch_first, zero initial state), exact fp32, for the recurrent
// upstreams (modified CPC: upstream/cpc/model.py:146-191).  The input projection x W_ih^T + b is a GEMM over all B * T rows
// and is NOT part of this file: the kernel takes its result (`pre`) and runs what cannot be batched over time,
//   LSTM (i, f, g, o):  a = pre_t + W_hh h;  c = sig(a_f) c + sig(a_i) tanh(a_g);  h = sig(a_o) tanh(c)
//   GRU  (r, z, n):     r = sig(pre_r + W_hr h), z = sig(pre_z + W_hz h), n = tanh(pre_n + r (W_hn h + b_hn));  h = (1 - z) n + z h
//
// Schedule: one launch per layer runs all T steps; the recurrence of utterance b belongs to workgroup b from t = 0 to T - 1 —
// no workgroup ever waits for another, there is no global-memory flag and no launch per step.  Thread r owns gate row r (rows
// r and r + 1024 when gates * H > 1024): per step it streams its row of W_hh — packed [H / 4][gates * H][4], so that the
// threads of a wave read 1 KiB of consecutive bytes per k-quad — against h broadcast from LDS, with four accumulators per row
// summed as (a0 + a1) + (a2 + a3): the order is a function of H alone, so a result depends neither on B nor on where the
// utterance sits in the batch.  Gate values go to LDS, the first H threads do the cell update (c and the previous h stay in
// their registers) and write h_t to LDS and to `out`: two barriers per step.  Sigmoid and tanh are the accurate expf / tanhf.
//
// Cost (derived): W_hh of an LSTM at H = 256 is 1 MiB; a CU has 512 KiB of registers and 160 KiB of LDS, so every step
// re-reads the matrix from L2: at ~135 GB/s of L2 bandwidth per CU that is ~8 us per step.  Measured: profiles/cpc_modified_fp32.md.
#include "kernels.h"

namespace s3 {
namespace {

__device__ __forceinline__ float sigmoid_acc(float x) { return 1.f / (1.f + expf(-x)); }

template <int CELL, int RPT>
__global__ __launch_bounds__(1024) void rnn_kernel(RnnParams p) {
    constexpr int G = CELL == 0 ? 4 : 3;
    extern __shared__ __align__(16) float rnn_sm[];  // h[H] | gates[G * H]
    const int H = p.H, R = G * H, NT = blockDim.x, tid = threadIdx.x;
    const int b = blockIdx.x;
    float* hs = rnn_sm;
    float* gs = rnn_sm + H;
    const float4* W = (const float4*)p.w;
    const float* pre = p.pre + (long)b * p.T * p.ld_pre;
    float* out = p.out + (long)b * p.T * p.ldo;
    int row[RPT];
    bool live[RPT], nrow[RPT];
    float bh[RPT];
#pragma unroll
    for (int i = 0; i < RPT; ++i) {
        const int r = tid + i * NT;
        live[i] = r < R;
        row[i] = live[i] ? r : R - 1;  // (an idle second row re-reads the last one: no branch in the stream loop)
        nrow[i] = CELL == 1 && row[i] >= 2 * H;
        bh[i] = nrow[i] ? p.b_hn[row[i] - 2 * H] : 0.f;
    }
    const bool cell_thread = tid < H;  // NT >= min(1024, 3 H) >= H for H <= RNN_H_MAX
    if (cell_thread) hs[tid] = 0.f;
    float c = 0.f, hprev = 0.f;
    __syncthreads();
    const int KQ = H >> 2;
    for (int t = 0; t < p.T; ++t) {
        const float* pt = pre + (long)t * p.ld_pre;
        float pv[RPT];
#pragma unroll
        for (int i = 0; i < RPT; ++i) pv[i] = nrow[i] ? bh[i] : pt[row[i]];
        const float pn = (CELL == 1 && cell_thread) ? pt[2 * H + tid] : 0.f;
        float a[RPT][4];
#pragma unroll
        for (int i = 0; i < RPT; ++i) a[i][0] = a[i][1] = a[i][2] = a[i][3] = 0.f;
#pragma unroll 8
        for (int kq = 0; kq < KQ; ++kq) {
            const float4 hv = *(const float4*)(hs + 4 * kq);
#pragma unroll
            for (int i = 0; i < RPT; ++i) {
                const float4 w = W[(long)kq * R + row[i]];
                a[i][0] = fmaf(w.x, hv.x, a[i][0]);
                a[i][1] = fmaf(w.y, hv.y, a[i][1]);
                a[i][2] = fmaf(w.z, hv.z, a[i][2]);
                a[i][3] = fmaf(w.w, hv.w, a[i][3]);
            }
        }
#pragma unroll
        for (int i = 0; i < RPT; ++i)
            if (live[i]) gs[row[i]] = pv[i] + ((a[i][0] + a[i][1]) + (a[i][2] + a[i][3]));
        __syncthreads();
        if (cell_thread) {
            float h;
            if (CELL == 0) {
                const float gi = sigmoid_acc(gs[tid]), gf = sigmoid_acc(gs[H + tid]);
                const float gg = tanhf(gs[2 * H + tid]), go = sigmoid_acc(gs[3 * H + tid]);
                c = fmaf(gf, c, gi * gg);
                h = go * tanhf(c);
            } else {
                const float gr = sigmoid_acc(gs[tid]), gz = sigmoid_acc(gs[H + tid]);
                const float gn = tanhf(fmaf(gr, gs[2 * H + tid], pn));
                h = fmaf(gz, hprev, (1.f - gz) * gn);
                hprev = h;
            }
            hs[tid] = h;
            out[(long)t * p.ldo + tid] = h;
        }
        __syncthreads();
    }
}

template <int CELL, int RPT>
hipError_t rnn_launch(const RnnParams& p, int threads, int lds, hipStream_t s) {
    hipLaunchKernelGGL((rnn_kernel<CELL, RPT>), dim3(p.B), dim3(threads), lds, s, p);
    return hipGetLastError();
}

}  // namespace

void pack_rnn_whh(const float* w, int gates, int H, std::vector<float>& out) {
    const long R = (long)gates * H;
    out.resize((size_t)R * H);
    for (long r = 0; r < R; ++r)
        for (int k = 0; k < H; ++k) out[(((long)(k >> 2)) * R + r) * 4 + (k & 3)] = w[r * H + k];
}

hipError_t launch_rnn(const RnnParams& p, hipStream_t s) {
    if (p.B <= 0 || p.T <= 0) return hipSuccess;
    if (p.cell < 0 || p.cell > 1 || p.H < 64 || (p.H & 63) || p.H > RNN_H_MAX) return hipErrorInvalidValue;
    const int G = p.cell == 0 ? 4 : 3, R = G * p.H;
    if (!p.pre || !p.w || !p.out || (p.cell == 1 && !p.b_hn) || p.ld_pre < R || p.ldo < p.H) return hipErrorInvalidValue;
    if (((uintptr_t)p.w) & 15) return hipErrorInvalidValue;
    const int threads = R < 1024 ? R : 1024;
    const int lds = (p.H + R) * 4;
    if (R <= 1024) return p.cell == 0 ? rnn_launch<0, 1>(p, threads, lds, s) : rnn_launch<1, 1>(p, threads, lds, s);
    return p.cell == 0 ? rnn_launch<0, 2>(p, threads, lds, s) : rnn_launch<1, 2>(p, threads, lds, s);
}

}  // namespace s3
