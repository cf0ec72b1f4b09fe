// cpc.hip — modified CPC (upstream/cpc/model.py:62-104,146-191, expert.py:25-49), exact fp32: five strided convolutions with
// symmetric zero padding, each followed by ChannelNorm (per frame over the C channels, unbiased variance, eps 1e-5) and ReLU,
// then a multi-layer LSTM or GRU over the whole padded time axis (rnn.hip).  No waveform normalisation, no frame mask.
//
// Schedule (all on the caller's stream, no host synchronisation):
//   conv0: one kernel from the waveform table — convolution, bias, ChannelNorm, ReLU — written channel-last into conv1's
//          operand: per utterance pad_1 zero rows, the L0 frames, pad_1 zero rows;
//   conv1..: an implicit GEMM on those zero-bordered rows (launch_gemm: K = k C, lda = stride C, a_batch_stride =
//          (pad + L + pad) C, bias in the epilogue, weights tap-major) -> channelnorm_relu: a wave per frame, written to the next
//          operand with its border rows; the last layer writes the recurrent network's input and state 0;
//   recurrent layers: pre = x W_ih^T + b over the B * T rows (launch_gemm), then launch_rnn: one launch per layer.
// States: the encoder output (B, T, C) and the last recurrent layer's output (B, T, H), H = C.
#include "engine_internal.h"

namespace s3 {
namespace {

constexpr float CN_EPS = 1e-5f;

// ChannelNorm + ReLU of one frame held as NCH channel quads per lane (quad index lane + 64 i); every lane of the wave takes part
template <int NCH>
__device__ __forceinline__ void channelnorm_relu_row(float4 (&v)[NCH], int lane, int nch, int C, const float* gamma, const float* beta) {
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < NCH; ++i)
        if (lane + 64 * i < nch) sum += (v[i].x + v[i].y) + (v[i].z + v[i].w);
    const float mean = wave_sum(sum) / (float)C;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < NCH; ++i)
        if (lane + 64 * i < nch) {
            const float d0 = v[i].x - mean, d1 = v[i].y - mean, d2 = v[i].z - mean, d3 = v[i].w - mean;
            q += (d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3);
        }
    const float var = wave_sum(q) / (float)(C - 1);  // torch.var: unbiased
    const float rs = 1.f / sqrtf(var + CN_EPS);
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
        const int ch = lane + 64 * i;
        if (ch >= nch) continue;
        const float4 g = gamma ? *(const float4*)(gamma + 4 * ch) : make_float4(1.f, 1.f, 1.f, 1.f);
        const float4 be = beta ? *(const float4*)(beta + 4 * ch) : make_float4(0.f, 0.f, 0.f, 0.f);
        v[i].x = fmaxf(fmaf((v[i].x - mean) * rs, g.x, be.x), 0.f);
        v[i].y = fmaxf(fmaf((v[i].y - mean) * rs, g.y, be.y), 0.f);
        v[i].z = fmaxf(fmaf((v[i].z - mean) * rs, g.z, be.z), 0.f);
        v[i].w = fmaxf(fmaf((v[i].w - mean) * rs, g.w, be.w), 0.f);
    }
}

// a wave per row of dst: row r of utterance b is a border row (zeros) or frame r - pad
template <int NCH>
__global__ __launch_bounds__(256) void channelnorm_relu_kernel(ChannelNormParams p) {
    const int R = p.pad + p.rows + p.pad;
    const long gr = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (gr >= (long)p.B * R) return;
    const int lane = threadIdx.x & 63;
    const int b = (int)(gr / R), r = (int)(gr - (long)b * R);
    const int nch = p.C >> 2;
    float* drow = p.dst ? p.dst + ((long)b * R + r) * p.C : nullptr;
    if (r < p.pad || r >= p.pad + p.rows) {
#pragma unroll
        for (int i = 0; i < NCH; ++i) {
            const int ch = lane + 64 * i;
            if (ch < nch) *(float4*)(drow + 4 * ch) = make_float4(0.f, 0.f, 0.f, 0.f);  // (pad > 0 only with dst)
        }
        return;
    }
    const int t = r - p.pad;
    const float* xr = p.x + ((long)b * p.rows + t) * p.C;
    float4 v[NCH];
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
        const int ch = lane + 64 * i;
        v[i] = ch < nch ? *(const float4*)(xr + 4 * ch) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    channelnorm_relu_row<NCH>(v, lane, nch, p.C, p.gamma, p.beta);
    float* srow = p.state ? p.state + ((long)b * p.rows + t) * p.C : nullptr;
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
        const int ch = lane + 64 * i;
        if (ch >= nch) continue;
        if (drow) *(float4*)(drow + 4 * ch) = v[i];
        if (srow) *(float4*)(srow + 4 * ch) = v[i];
    }
}

// conv0: a workgroup takes CONV0_ROWS consecutive rows of one utterance's operand, a wave a row at a time; the taps
// (transposed to [10][C]) and the bias sit in LDS
constexpr int CONV0_K = 10;
constexpr int CONV0_ROWS = 64;
template <int NCH>
__global__ __launch_bounds__(256) void cpc_conv0_kernel(CpcConv0Params p) {
    extern __shared__ __align__(16) float c0_sm[];  // w[10][C] | bias[C]
    const int C = p.C, nch = C >> 2;
    for (int i = threadIdx.x; i < CONV0_K * C; i += 256) {
        const int j = i / C, c = i - j * C;
        c0_sm[i] = p.w0[c * CONV0_K + j];
    }
    for (int i = threadIdx.x; i < C; i += 256) c0_sm[CONV0_K * C + i] = p.bias[i];
    __syncthreads();
    const int b = blockIdx.y, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long R = p.pad + p.L0 + p.pad;
    const float* wav = p.wav.ptrs[b];
    const long len = p.wav.lens[b];
    const long r_end = min((long)(blockIdx.x + 1) * CONV0_ROWS, R);
    for (long r = (long)blockIdx.x * CONV0_ROWS + wave; r < r_end; r += 4) {
        float* drow = p.dst + ((long)b * R + r) * C;
        float4 v[NCH];
        if (r < p.pad || r >= p.pad + p.L0) {
#pragma unroll
            for (int i = 0; i < NCH; ++i) {
                const int ch = lane + 64 * i;
                if (ch < nch) *(float4*)(drow + 4 * ch) = make_float4(0.f, 0.f, 0.f, 0.f);
            }
            continue;
        }
        const long s0 = (r - p.pad) * p.s0 - p.pad0;
        float x[CONV0_K];
#pragma unroll
        for (int j = 0; j < CONV0_K; ++j) {
            const long s = s0 + j;
            x[j] = (s >= 0 && s < len) ? wav[s] : 0.f;
        }
#pragma unroll
        for (int i = 0; i < NCH; ++i) {
            const int ch = lane + 64 * i;
            v[i] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (ch >= nch) continue;
            float4 acc = *(const float4*)(c0_sm + CONV0_K * C + 4 * ch);
#pragma unroll
            for (int j = 0; j < CONV0_K; ++j) {
                const float4 w = *(const float4*)(c0_sm + j * C + 4 * ch);
                acc.x = fmaf(w.x, x[j], acc.x);
                acc.y = fmaf(w.y, x[j], acc.y);
                acc.z = fmaf(w.z, x[j], acc.z);
                acc.w = fmaf(w.w, x[j], acc.w);
            }
            v[i] = acc;
        }
        channelnorm_relu_row<NCH>(v, lane, nch, C, p.gamma, p.beta);
#pragma unroll
        for (int i = 0; i < NCH; ++i) {
            const int ch = lane + 64 * i;
            if (ch < nch) *(float4*)(drow + 4 * ch) = v[i];
        }
    }
}

}  // namespace

hipError_t launch_channelnorm_relu(const ChannelNormParams& p, hipStream_t s) {
    if (p.B <= 0 || p.rows <= 0) return hipSuccess;
    if (!p.x || p.C < 8 || (p.C & 3) || p.C > 1024 || p.pad < 0 || (!p.dst && p.pad) || (!p.dst && !p.state)) return hipErrorInvalidValue;
    const long R = (long)p.B * (p.pad + p.rows + p.pad);
    if ((R + 3) / 4 > 0x7fffffffL) return hipErrorInvalidValue;
    dim3 grid((unsigned)((R + 3) / 4)), block(256);
    switch (((p.C >> 2) + 63) / 64) {
        case 1: hipLaunchKernelGGL(channelnorm_relu_kernel<1>, grid, block, 0, s, p); break;
        case 2: hipLaunchKernelGGL(channelnorm_relu_kernel<2>, grid, block, 0, s, p); break;
        case 3: hipLaunchKernelGGL(channelnorm_relu_kernel<3>, grid, block, 0, s, p); break;
        default: hipLaunchKernelGGL(channelnorm_relu_kernel<4>, grid, block, 0, s, p); break;
    }
    return hipGetLastError();
}

hipError_t launch_cpc_conv0(const CpcConv0Params& p, hipStream_t s) {
    if (p.wav.B <= 0 || p.L0 <= 0) return hipSuccess;
    if (!p.w0 || !p.bias || !p.dst || p.C < 8 || (p.C & 3) || p.C > 1024 || p.s0 < 1 || p.pad0 < 0 || p.pad < 0 || p.wav.B > 65535)
        return hipErrorInvalidValue;
    const long R = p.pad + p.L0 + p.pad;
    dim3 grid((unsigned)((R + CONV0_ROWS - 1) / CONV0_ROWS), p.wav.B), block(256);
    const int lds = (CONV0_K + 1) * p.C * 4;
    switch (((p.C >> 2) + 63) / 64) {
        case 1: hipLaunchKernelGGL(cpc_conv0_kernel<1>, grid, block, lds, s, p); break;
        case 2: hipLaunchKernelGGL(cpc_conv0_kernel<2>, grid, block, lds, s, p); break;
        case 3: hipLaunchKernelGGL(cpc_conv0_kernel<3>, grid, block, lds, s, p); break;
        default: hipLaunchKernelGGL(cpc_conv0_kernel<4>, grid, block, lds, s, p); break;
    }
    return hipGetLastError();
}

}  // namespace s3

// ---- the handle's side: configuration, weights, forward ------------------------------------------------------------------
namespace s3e {

static long cpc_conv_len(const s3enc_config& c, const s3enc_cpc_config& x, long n, int upto /*exclusive*/) {
    for (int i = 0; i < upto; ++i) {
        const long padded = n + 2L * x.conv_pad[i];
        n = (n > 0 && padded >= c.conv_kernel[i]) ? (padded - c.conv_kernel[i]) / c.conv_stride[i] + 1 : 0;
    }
    return n;
}

static int cpc_check_config(const s3enc_config& c, const s3enc_cpc_config& x) {
    static const char* dt[] = {"fp32", "bf16", "fp16", "fp32x3", "fp16x2"};
    if (c.compute_dtype < 0 || c.compute_dtype > 4) return fail("config: unknown compute_dtype");
    if (c.compute_dtype != S3ENC_F32)
        return fail(std::string("config: modified CPC (conv encoder + LSTM / GRU) is built for compute dtype fp32 only; ") +
                    dt[c.compute_dtype] + " is not built");
    static const char* nm[] = {"layerNorm", "instanceNorm", "ID", "batchNorm"};
    if (x.norm_mode < 0 || x.norm_mode > 3) return fail("config: unknown cpc norm_mode");
    if (x.norm_mode != 0) return fail(std::string("config: cpc normMode=\"") + nm[x.norm_mode] + "\" is not built (only \"layerNorm\", the channel norm)");
    static const char* am[] = {"LSTM", "GRU", "RNN", "transformer", "no_ar"};
    if (x.ar_mode < 0 || x.ar_mode > 4) return fail("config: unknown cpc ar_mode");
    if (x.ar_mode > 1) return fail(std::string("config: cpc arMode=\"") + am[x.ar_mode] + "\" is not built (only \"LSTM\" and \"GRU\")");
    if (x.reverse) return fail("config: cpc_mode=\"reverse\" is not built");
    if (x.keep_hidden) return fail("config: cpc samplingType=\"sequential\" (the recurrent state carried between forwards) is not built");
    if (x.ar_hidden != c.conv_dim)
        return fail("config: cpc hiddenGar != hiddenEncoder is not built (the two states share one width)");
    if (c.conv_dim < 64 || c.conv_dim % 64 || c.conv_dim > RNN_H_MAX)
        return fail("config: cpc widths must be a multiple of 64, at most " + std::to_string(RNN_H_MAX) + " (the recurrent kernel's limit)");
    if (x.ar_layers < 1 || x.ar_layers > 4) return fail("config: cpc nLevelsGRU must be 1..4 recurrent layers");
    if (c.n_conv < 2 || c.n_conv > S3ENC_MAX_CONV) return fail("config: n_conv out of range");
    if (c.conv_kernel[0] != 10) return fail("config: the conv0 kernel is specialised for kernel width 10");
    if (c.conv_stride[0] < 1 || c.conv_stride[0] > 16) return fail("config: conv0 stride out of range");
    for (int i = 0; i < c.n_conv; ++i) {
        if (c.conv_kernel[i] < 1 || c.conv_kernel[i] > 64 || c.conv_stride[i] < 1 || c.conv_stride[i] > 16)
            return fail("config: conv kernel / stride out of range");
        if (x.conv_pad[i] < 0 || x.conv_pad[i] >= c.conv_kernel[i]) return fail("config: cpc conv padding must be 0 .. kernel - 1");
    }
    if (c.encoder_layers != 1 || c.embed_dim != c.conv_dim) return fail("config: cpc encoder_layers must be 1 and embed_dim the conv width");
    return 0;
}

static int cpc_create(s3enc_encoder* e, const Ckpt& ck) {
    const s3enc_config& c = e->cfg;
    const s3enc_cpc_config& x = e->cpc_cfg;
    const int C = c.conv_dim, H = x.ar_hidden, G = x.ar_mode == 0 ? 4 : 3;
    e->cpc.reset(new CpcW());
    CpcW& w = *e->cpc;
    std::vector<float> t, t2;
    w.conv_w.resize(c.n_conv);
    w.conv_b.resize(c.n_conv);
    w.cn_g.resize(c.n_conv);
    w.cn_b.resize(c.n_conv);
    for (int i = 0; i < c.n_conv; ++i) {
        const std::string n = std::to_string(i);
        const int cin = i == 0 ? 1 : C, k = c.conv_kernel[i];
        GET("gEncoder.conv" + n + ".weight", (long)C * cin * k, t);
        if (i == 0) {
            UP(upload_f32(w.conv_w[i], t));  // [C][10]
        } else {
            tap_major(t, C, C, k, t2);
            UP(upload_f32(w.conv_w[i], t2));
        }
        GET("gEncoder.conv" + n + ".bias", C, t);
        UP(upload_f32(w.conv_b[i], t));
        GET("gEncoder.batchNorm" + n + ".weight", C, t);  // (1, C, 1)
        UP(upload_f32(w.cn_g[i], t));
        GET("gEncoder.batchNorm" + n + ".bias", C, t);
        UP(upload_f32(w.cn_b[i], t));
    }
    for (int l = 0; l < x.ar_layers; ++l)  // layer 0 reads the encoder output: C == H
        if (load_rnn_layer(ck, "gAR.baseNet.", "_l" + std::to_string(l), G, H, H, w)) return 1;
    return 0;
}

static int cpc_forward(s3enc_handle e, const float* const* wav_ptrs_host, const int64_t* lengths, int32_t B, int64_t n_max_in,
                const FwdOpts& fo, void* out, int64_t layer_stride, hipStream_t st) {
    const s3enc_config& c = e->cfg;
    const s3enc_cpc_config& x = e->cpc_cfg;
    const CpcW& w = *e->cpc;
    const int C = c.conv_dim, H = x.ar_hidden, G = x.ar_mode == 0 ? 4 : 3, NC = c.n_conv, NL = x.ar_layers;
    if (fo.selection != S3ENC_SEL_HIDDEN)
        return fail("s3enc_forward: feature_selection is not defined for modified CPC (the reference expert has one hidden_states list)");
    if (fo.featurize && !fo.w) return fail("s3enc_forward: featurize needs feat_w");
    if (!fo.featurize && fo.out_dtype != F32) return fail("s3enc_forward: out_dtype must be S3ENC_F32 for a modified-CPC handle");
    if (e->aux_codewords || e->aux_codeids) return fail("s3enc_forward_aux: codewords / codeids are outputs of a wav2vec handle with a vector quantizer");
    long n_max;
    if (batch_n_max(wav_ptrs_host, lengths, B, n_max_in, n_max)) return 1;
    std::vector<long> L(NC);
    for (int i = 0; i < NC; ++i) L[i] = cpc_conv_len(c, x, n_max, i + 1);
    const long T = L[NC - 1];
    if (T < 1) return fail("s3enc_forward: input shorter than the receptive field of the conv stack (modified CPC needs 159 samples)");
    const long M = (long)B * T;
    if (B > 65535) return fail("s3enc_forward: batch too large");
    if (check_out(out, fo, layer_stride, M * C)) return 1;
    // operand i (i = 1 .. NC - 1): conv i's input, (B, pad_i + L[i-1] + pad_i, C)
    long op_max = 0, raw_max = 0;
    for (int i = 1; i < NC; ++i) {
        op_max = std::max(op_max, L[i - 1] + 2L * x.conv_pad[i]);
        raw_max = std::max(raw_max, L[i]);
    }
    if ((long)B * op_max * C >= (1L << 40) || M > 0x7fffffffL) return fail("s3enc_forward: batch too large");
    DeviceGuard dg(e->device);
    if (!dg.ok) return fail("s3enc_forward: hipSetDevice failed");

    // ---- small device state: the waveform table ----
    const size_t tbl_bytes = (size_t)B * 16;
    HIP_TRY(e->small.ensure_on_stream(tbl_bytes + 1024, st));
    char* d_tbl = (char*)e->small.p;
    char* hp;
    if (stage_begin(e, tbl_bytes, st, hp)) return 1;
    memcpy(hp, wav_ptrs_host, (size_t)B * 8);
    for (int b = 0; b < B; ++b) ((long*)(hp + (size_t)B * 8))[b] = (long)lengths[b];
    if (stage_commit(e, hp, d_tbl, tbl_bytes, st)) return 1;
    WavTable wt{(const float* const*)d_tbl, (const long*)(d_tbl + (size_t)B * 8), B, n_max};

    // ---- workspace ----
    float *opA, *opB, *raw, *enc, *pre, *hA, *hB;
    for (int pass = 0; pass < 2; ++pass) {
        Bump wb(pass ? e->ws.p : nullptr);
        opA = (float*)wb.take((size_t)B * op_max * C * 4);
        opB = (float*)wb.take((size_t)B * op_max * C * 4);
        raw = (float*)wb.take((size_t)B * raw_max * C * 4);
        enc = (float*)wb.take((size_t)M * C * 4);
        pre = (float*)wb.take((size_t)M * G * H * 4);
        hA = (float*)wb.take((size_t)M * H * 4);
        hB = (float*)wb.take((size_t)M * H * 4);
        if (!pass) HIP_TRY(e->ws.ensure_on_stream(wb.off + 4096, st));
    }
    e->taps.clear();

    // ---- where the states go ----
    Sink sink{e, st, fo.featurize ? 2 : 0, out, (long)layer_stride, F32, M, C, fo.w, fo.feat_norm};
    HIP_TRY(sink.zero_without_terms(2, M));

    // ---- conv0 into conv1's zero-bordered operand ----
    {
        CpcConv0Params p{};
        p.wav = wt;
        p.w0 = (const float*)w.conv_w[0].p;
        p.bias = (const float*)w.conv_b[0].p;
        p.gamma = (const float*)w.cn_g[0].p;
        p.beta = (const float*)w.cn_b[0].p;
        p.C = C;
        p.s0 = c.conv_stride[0];
        p.pad0 = x.conv_pad[0];
        p.L0 = L[0];
        p.pad = x.conv_pad[1];
        p.dst = opA;
        Prof pr(e, st, "cpc_conv0", 2.0 * B * L[0] * C * 10, 4.0 * B * n_max + 4.0 * B * L[0] * C);
        HIP_TRY(launch_cpc_conv0(p, st));
    }
    // ---- conv1..: implicit GEMM on the bordered rows, then ChannelNorm + ReLU into the next operand ----
    float* cur = opA;
    float* state0 = sink.slot32(0) ? sink.slot32(0) : enc;
    for (int i = 1; i < NC; ++i) {
        const bool last = i == NC - 1;
        const int k = c.conv_kernel[i], pad = x.conv_pad[i];
        GemmParams g{};
        g.A = cur;
        g.lda = (long)c.conv_stride[i] * C;
        g.a_bs = (L[i - 1] + 2L * pad) * C;
        g.W = w.conv_w[i].p;
        g.bias = (const float*)w.conv_b[i].p;
        g.M = (int)L[i];
        g.N = C;
        g.K = k * C;
        g.batches = B;
        g.out32 = raw;
        g.ldo = C;
        g.o_bs = L[i] * C;
        {
            char kind[32];
            snprintf(kind, sizeof(kind), "gemm:cpc_conv%d", i);
            Prof pr(e, st, kind, 2.0 * B * L[i] * C * g.K, 4.0 * ((double)B * (L[i - 1] + 2 * pad) * C + (double)C * g.K + (double)B * L[i] * C));
            HIP_TRY(launch_gemm(F32, g, st));
        }
        ChannelNormParams a{};
        a.x = raw;
        a.gamma = (const float*)w.cn_g[i].p;
        a.beta = (const float*)w.cn_b[i].p;
        a.B = B;
        a.rows = (int)L[i];
        a.C = C;
        float* nxt = cur == opA ? opB : opA;
        if (!last) {
            a.pad = x.conv_pad[i + 1];
            a.dst = nxt;
        } else {
            a.state = state0;  // state 0, read back by the first recurrent layer's input projection
        }
        {
            Prof pr(e, st, "channelnorm_relu", 0, 4.0 * B * L[i] * C * 2);
            HIP_TRY(launch_channelnorm_relu(a, st));
        }
        cur = nxt;
    }
    if (sink.term(0)) {  // featurize: the state's term of the weighted sum
        Prof pr(e, st, "emit_state", 0, 4.0 * M * C * 2);
        HIP_TRY(sink.emit(0, state0));
    }
    HIP_TRY(sink.done(0));

    // ---- recurrent layers ----
    const float* xin = state0;
    for (int l = 0; l < NL; ++l) {
        const bool last = l == NL - 1;
        HIP_TRY(linear_f32(e, st, {"gemm:cpc_ar_in", xin, w.w_ih[l].p, w.b_pre[l].p, M, G * H, H, 0, nullptr, pre}));
        float* hout = (last && sink.slot32(1)) ? sink.slot32(1) : ((l & 1) ? hB : hA);
        RnnParams r{};
        r.cell = x.ar_mode;
        r.pre = pre;
        r.w = (const float*)w.w_hh[l].p;
        r.b_hn = (const float*)w.b_hn[l].p;
        r.B = B;
        r.T = (int)T;
        r.H = H;
        r.ld_pre = (long)G * H;
        r.out = hout;
        r.ldo = H;
        {
            Prof pr(e, st, x.ar_mode == 0 ? "rnn_lstm" : "rnn_gru", 2.0 * M * G * H * H, 4.0 * ((double)M * G * H + (double)M * H));
            HIP_TRY(launch_rnn(r, st));
        }
        xin = hout;
    }
    if (sink.term(1)) {  // featurize: the state's term of the weighted sum
        Prof pr(e, st, "emit_state", 0, 4.0 * M * C * 2);
        HIP_TRY(sink.emit(1, xin));
    }
    HIP_TRY(sink.done(1));
    return 0;
}


// no mask: the frames the utterance's own samples reach through the padded stack (the wav2vec convention)
FamilyOps kCpcFamily = {
    S3ENC_CPC, "cpc", "S3ENC_CPC", "s3enc_create_cpc", "the modified-CPC family needs its padding / recurrent-network block",
    "modified CPC (one hidden_states list of 2 states)",
    [](const s3enc_config& c, const void* b) { return cpc_check_config(c, *(const s3enc_cpc_config*)b); },
    [](s3enc_encoder* e, const Ckpt& ck, const void* b) { e->cpc_cfg = *(const s3enc_cpc_config*)b; return cpc_create(e, ck); },
    cpc_forward,
    [](const s3enc_encoder* h, long n) { return cpc_conv_len(h->cfg, h->cpc_cfg, n, h->cfg.n_conv); }};

}  // namespace s3e
