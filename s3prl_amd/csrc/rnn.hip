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
//
// Length-aware form (launch_rnn_len; APC: upstream/apc/apc.py:118-139 runs pack_padded_sequence / pad_packed_sequence): the same
// kernel under a compile-time flag — workgroup b stops its step loop at len[b], the row written is h_t (+ the residual operand's
// row; the carried state stays the un-summed h_t), and all its threads then write rows [len[b], T) as zeros with 16-byte stores.
// The flag is the parameter struct's type, so launch_rnn's instantiations keep their code and their argument block.
#include <type_traits>

#include "kernels.h"

namespace s3 {
namespace {

__device__ __forceinline__ float sigmoid_acc(float x) { return 1.f / (1.f + expf(-x)); }

template <int CELL, int RPT, typename P>
__global__ __launch_bounds__(1024) void rnn_kernel(P p) {
    constexpr int G = CELL == 0 ? 4 : 3;
    constexpr bool LEN = std::is_same<P, RnnLenParams>::value;
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
    int steps = p.T;
    const float* res = nullptr;
    if constexpr (LEN) {
        steps = min(max(p.len[b], 0), p.T);
        if (p.res) res = p.res + (long)b * p.T * p.ld_res;
    }
    for (int t = 0; t < steps; ++t) {
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
            if constexpr (LEN) {
                out[(long)t * p.ldo + tid] = res ? h + res[(long)t * p.ld_res + tid] : h;
            } else {
                out[(long)t * p.ldo + tid] = h;
            }
        }
        __syncthreads();
    }
    if constexpr (LEN) {  // pad_packed_sequence: the rows behind the utterance's length are zeros
        const int hq = H >> 2;
        const long n = (long)(p.T - steps) * hq;
        for (long i = tid; i < n; i += NT) {
            const long r = i / hq;
            const int q = (int)(i - r * hq);
            *(float4*)(out + (steps + r) * p.ldo + 4 * q) = make_float4(0.f, 0.f, 0.f, 0.f);
        }
    }
}

template <int CELL, int RPT, typename P>
hipError_t rnn_launch(const P& p, int threads, int lds, hipStream_t s) {
    hipLaunchKernelGGL((rnn_kernel<CELL, RPT, P>), dim3(p.B), dim3(threads), lds, s, p);
    return hipGetLastError();
}

// ---- the step-split form: one launch per time step, (S, B) workgroups ------------------------------------------------------
// Workgroup (s, b) owns hidden units [s U, (s + 1) U), U = H / S, of utterance b with ALL their gate rows, so the cell update is
// local: per step it reads h_{t-1} (H floats) from a (2, B, H) ping-pong buffer, streams its G U rows of the packed W_hh and writes
// its slice of h_t and of the output row.  Nobody waits for anybody: the kernel boundary is the only synchronisation (no flags,
// no cooperative launch); workgroups of an utterance with t >= len[b] return at once; the zero tail is written by the t = 0
// launch.  A gate row's dot product keeps rnn_kernel's order — four accumulators over the k-quads, (a0 + a1) + (a2 + a3) — and the
// cell expressions are the same fmafs, so the result is bit-identical to the one-launch form for every S (tested).
//
// A step is bound by loads in flight, not by bytes.  Written as rnn_kernel's loop, the compiler waits for every row load before it
// issues the next (one KiB outstanding per wave): 128 round trips to L2 per step at H = 512 — measured 17.0 us with S = 4 and 17.3 us
// with S = 8, twice the waves on twice the bytes.  So the loop is blocked: the UNR loads of a block are issued into registers first,
// then multiplied in the same order (measured: 9.8 us with S = 4, 8.1 us with S = 8).  Workgroups of at most 512 threads take
// 16 k-quads per block, the larger ones 8.
template <int CELL, int RPT, int UNR, int MAXT>
__global__ __launch_bounds__(MAXT) void rnn_step_kernel(RnnStepParams p) {
    constexpr int G = CELL == 0 ? 4 : 3;
    extern __shared__ __align__(16) float rnn_sm[];  // h[H] | gates[G * U]
    const int H = p.H, R = G * H, NT = blockDim.x, tid = threadIdx.x;
    const int U = H / p.S, RL = G * U;
    const int s = blockIdx.x, b = blockIdx.y, t = p.t;
    const int steps = min(max(p.len[b], 0), p.T);
    if (t >= steps) return;
    float* hs = rnn_sm;
    float* gs = rnn_sm + H;
    const float4* W = (const float4*)p.w;
    const float* pt = p.pre + ((long)b * p.T + t) * p.ld_pre;
    float* out = p.out + (long)b * p.T * p.ldo;
    const float* hin = p.hbuf + ((long)((t + 1) & 1) * p.B + b) * H;  // written by the launch of step t - 1
    float* hout = p.hbuf + ((long)(t & 1) * p.B + b) * H;
    for (int i = tid; i < H; i += NT) hs[i] = t ? hin[i] : 0.f;
    int row[RPT], lrow[RPT];
    bool live[RPT], nrow[RPT];
    float pv[RPT];
#pragma unroll
    for (int i = 0; i < RPT; ++i) {
        const int lr = tid + i * NT;
        live[i] = lr < RL;
        lrow[i] = live[i] ? lr : RL - 1;
        const int g = lrow[i] / U, u = lrow[i] - g * U;
        row[i] = g * H + s * U + u;
        nrow[i] = CELL == 1 && g == 2;
        pv[i] = nrow[i] ? p.b_hn[row[i] - 2 * H] : pt[row[i]];
    }
    __syncthreads();
    const int KQ = H >> 2;
    float a[RPT][4];
#pragma unroll
    for (int i = 0; i < RPT; ++i) a[i][0] = a[i][1] = a[i][2] = a[i][3] = 0.f;
    for (int kq0 = 0; kq0 < KQ; kq0 += UNR) {  // KQ = H / 4 is a multiple of 16
        float4 w[RPT][UNR];  // all UNR loads of a row are issued before the first product waits for one
#pragma unroll
        for (int u = 0; u < UNR; ++u)
#pragma unroll
            for (int i = 0; i < RPT; ++i) w[i][u] = W[(long)(kq0 + u) * R + row[i]];
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
            const float4 hv = *(const float4*)(hs + 4 * (kq0 + u));
#pragma unroll
            for (int i = 0; i < RPT; ++i) {
                a[i][0] = fmaf(w[i][u].x, hv.x, a[i][0]);
                a[i][1] = fmaf(w[i][u].y, hv.y, a[i][1]);
                a[i][2] = fmaf(w[i][u].z, hv.z, a[i][2]);
                a[i][3] = fmaf(w[i][u].w, hv.w, a[i][3]);
            }
        }
    }
#pragma unroll
    for (int i = 0; i < RPT; ++i)
        if (live[i]) gs[lrow[i]] = pv[i] + ((a[i][0] + a[i][1]) + (a[i][2] + a[i][3]));
    __syncthreads();
    if (tid < U) {  // NT >= min(1024, G U) >= U
        const int j = s * U + tid;
        float h;
        if (CELL == 0) {
            const float gi = sigmoid_acc(gs[tid]), gf = sigmoid_acc(gs[U + tid]);
            const float gg = tanhf(gs[2 * U + tid]), go = sigmoid_acc(gs[3 * U + tid]);
            float c = t ? p.cbuf[(long)b * H + j] : 0.f;
            c = fmaf(gf, c, gi * gg);
            h = go * tanhf(c);
            p.cbuf[(long)b * H + j] = c;
        } else {
            const float pn = pt[2 * H + j];
            const float hprev = hs[j];
            const float gr = sigmoid_acc(gs[tid]), gz = sigmoid_acc(gs[U + tid]);
            const float gn = tanhf(fmaf(gr, gs[2 * U + tid], pn));
            h = fmaf(gz, hprev, (1.f - gz) * gn);
        }
        hout[j] = h;
        out[(long)t * p.ldo + j] = p.res ? h + p.res[((long)b * p.T + t) * p.ld_res + j] : h;
    }
    if (t == 0) {  // pad_packed_sequence: this workgroup's columns of the rows behind the utterance's length, once per layer
        const int uq = U >> 2;
        const long n = (long)(p.T - steps) * uq;
        for (long i = tid; i < n; i += NT) {
            const long r = i / uq;
            const int q = (int)(i - r * uq);
            *(float4*)(out + (steps + r) * p.ldo + s * U + 4 * q) = make_float4(0.f, 0.f, 0.f, 0.f);
        }
    }
}

template <int CELL, int RPT, int UNR, int MAXT>
hipError_t rnn_step_launch(const RnnStepParams& p0, int threads, int lds, hipStream_t s) {
    RnnStepParams p = p0;
    for (int t = 0; t < p.max_len; ++t) {
        p.t = t;
        hipLaunchKernelGGL((rnn_step_kernel<CELL, RPT, UNR, MAXT>), dim3(p.S, p.B), dim3(threads), lds, s, p);
    }
    return hipGetLastError();
}

template <typename P>
hipError_t rnn_dispatch(const P& p, hipStream_t s) {
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

}  // namespace

void pack_rnn_whh(const float* w, int gates, int H, std::vector<float>& out) {
    const long R = (long)gates * H;
    out.resize((size_t)R * H);
    for (long r = 0; r < R; ++r)
        for (int k = 0; k < H; ++k) out[(((long)(k >> 2)) * R + r) * 4 + (k & 3)] = w[r * H + k];
}

hipError_t launch_rnn(const RnnParams& p, hipStream_t s) { return rnn_dispatch(p, s); }

hipError_t launch_rnn_len(const RnnLenParams& p, hipStream_t s) {
    if (!p.len || (p.res && p.ld_res < p.H)) return hipErrorInvalidValue;
    if ((((uintptr_t)p.out) & 15) || (p.ldo & 3)) return hipErrorInvalidValue;  // the zero tail's 16-byte stores
    return rnn_dispatch(p, s);
}

bool rnn_split_ok(int H, int B, int S) {
    return S >= 1 && S <= 8 && !(S & (S - 1)) && H % S == 0 && (H / S) % 64 == 0 && (long)S * B <= 256;
}

int rnn_split_pick(int cell, int H, int B) {
    const int S = tuning().rnn_split;
    if (S >= 0) return S;
    // measured (profiles/apc_360hr_fp32.md): the GRU at H = 512 — 8.1 us per step with S = 8 against 28.7 us in one launch
    return (cell == 1 && H == 512 && rnn_split_ok(H, B, 8)) ? 8 : 0;
}

hipError_t launch_rnn_step(const RnnStepParams& p, hipStream_t s) {
    if (p.B <= 0 || p.T <= 0 || p.max_len <= 0) return hipSuccess;
    if (p.cell < 0 || p.cell > 1 || p.H < 64 || (p.H & 63) || p.H > RNN_H_MAX) return hipErrorInvalidValue;
    const int G = p.cell == 0 ? 4 : 3, R = G * p.H;
    if (!p.pre || !p.w || !p.out || (p.cell == 1 && !p.b_hn) || p.ld_pre < R || p.ldo < p.H) return hipErrorInvalidValue;
    if (!p.len || (p.res && p.ld_res < p.H) || !p.hbuf || (p.cell == 0 && !p.cbuf) || p.max_len > p.T) return hipErrorInvalidValue;
    if ((((uintptr_t)p.w) & 15) || (((uintptr_t)p.out) & 15) || (p.ldo & 3)) return hipErrorInvalidValue;
    if (!rnn_split_ok(p.H, p.B, p.S)) return hipErrorInvalidValue;
    const int RL = G * (p.H / p.S);
    const int threads = RL < 1024 ? RL : 1024;
    const int lds = (p.H + RL) * 4;
    if (RL <= 512) return p.cell == 0 ? rnn_step_launch<0, 1, 16, 512>(p, threads, lds, s) : rnn_step_launch<1, 1, 16, 512>(p, threads, lds, s);
    if (RL <= 1024) return p.cell == 0 ? rnn_step_launch<0, 1, 8, 1024>(p, threads, lds, s) : rnn_step_launch<1, 1, 8, 1024>(p, threads, lds, s);
    return p.cell == 0 ? rnn_step_launch<0, 2, 8, 1024>(p, threads, lds, s) : rnn_step_launch<1, 2, 8, 1024>(p, threads, lds, s);
}

}  // namespace s3
