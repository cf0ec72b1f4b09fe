// wav2vec.hip — wav2vec / vq-wav2vec (upstream/wav2vec/wav2vec_model.py, expert.py:15-62), exact fp32: a convolutional feature
// extractor, an optional vector quantizer (gumbel: wav2vec2_model.py:1591-1782 in eval; k-means: wav2vec_model.py:117-232) and a
// causal convolutional aggregator.  Every block is Conv1d -> Fp32GroupNorm(1, C) over ALL C x L values of the utterance (the
// zero-padded time included) -> ReLU.
//
// Schedule (all on the caller's stream, no host synchronisation):
//   conv0: the GroupNorm statistics in closed form from the waveform's lag sums (launch_gn1_stats), normalisation + ReLU inside
//          the conv0 kernel;
//   every other convolution: an implicit GEMM on channel-last rows (launch_gemm, raw output) -> launch_group1_stats (double, fixed
//          partition) -> gn1_apply: normalise, ReLU, [skip connection], [log compression], written to the next convolution's
//          operand (k - 1 replicated / zero rows in front of each utterance), the hidden-state slot and the Featurizer term;
//   quantizers: projection GEMM(s) -> argmax_gather (gumbel), or grouped 1x1 GEMMs -> per-(b, group) statistics -> negated squared
//          distances -> argmax_gather (k-means).
// States: z (the un-quantized extractor output), the output of every aggregator layer (= the input of the next one, then c).
#include "engine_internal.h"

#include <climits>

namespace s3 {
namespace {

template <int NCH>
__global__ __launch_bounds__(256) void gn1_apply_kernel(Gn1ApplyParams p) {
    const int R = p.pad + p.rows;
    const long gr = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (gr >= (long)p.B * R) return;
    const int lane = threadIdx.x & 63;
    const int b = (int)(gr / R), r = (int)(gr - (long)b * R);
    const int nch = p.C >> 2;
    const bool padrow = r < p.pad;
    const int t = padrow ? 0 : r - p.pad;
    float* drow = p.dst ? p.dst + (long)b * p.dst_bs + (long)r * p.C : nullptr;
    if (padrow && p.pad_zero) {
#pragma unroll
        for (int i = 0; i < NCH; ++i) {
            const int ch = lane + 64 * i;
            if (ch < nch) *(float4*)(drow + 4 * ch) = make_float4(0.f, 0.f, 0.f, 0.f);
        }
        return;
    }
    // GroupNorm(1, C) statistics of utterance b from the GS_BLOCKS (= one wave of) double partials: biased variance, eps 1e-5
    const double* pp = p.partial + ((long)b * GS_BLOCKS + lane) * 2;
    const double s = wave_sum_d(pp[0]), q = wave_sum_d(pp[1]);
    const double mud = s / p.count;
    double var = q / p.count - mud * mud;
    var = var > 0.0 ? var : 0.0;
    const float mu = (float)mud, rs = (float)(1.0 / sqrt(var + (double)LN_EPS));
    const float* xr = p.x + (long)b * p.x_bs + (long)t * p.C;
    const float* rr = p.res ? p.res + (long)b * p.res_bs + (long)t * p.C : nullptr;
    float4 y[NCH];
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
        const int ch = lane + 64 * i;
        y[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (ch >= nch) continue;
        const float4 v = *(const float4*)(xr + 4 * ch);
        const float4 g = p.gamma ? *(const float4*)(p.gamma + 4 * ch) : make_float4(1.f, 1.f, 1.f, 1.f);
        const float4 be = p.beta ? *(const float4*)(p.beta + 4 * ch) : make_float4(0.f, 0.f, 0.f, 0.f);
        float a0 = fmaxf(fmaf((v.x - mu) * rs, g.x, be.x), 0.f), a1 = fmaxf(fmaf((v.y - mu) * rs, g.y, be.y), 0.f);
        float a2 = fmaxf(fmaf((v.z - mu) * rs, g.z, be.z), 0.f), a3 = fmaxf(fmaf((v.w - mu) * rs, g.w, be.w), 0.f);
        if (rr) {
            const float4 x1 = *(const float4*)(rr + 4 * ch);
            a0 = (a0 + x1.x) * p.scale; a1 = (a1 + x1.y) * p.scale; a2 = (a2 + x1.z) * p.scale; a3 = (a3 + x1.w) * p.scale;
        }
        if (p.log) {
            a0 = log1pf(fabsf(a0)); a1 = log1pf(fabsf(a1)); a2 = log1pf(fabsf(a2)); a3 = log1pf(fabsf(a3));
        }
        y[i] = make_float4(a0, a1, a2, a3);
        sum += (a0 + a1) + (a2 + a3);
        if (drow) *(float4*)(drow + 4 * ch) = y[i];
    }
    if (padrow) return;
    const long srow = ((long)b * p.rows + t) * p.C;
    if (p.state) {
#pragma unroll
        for (int i = 0; i < NCH; ++i) {
            const int ch = lane + 64 * i;
            if (ch < nch) *(float4*)(p.state + srow + 4 * ch) = y[i];
        }
    }
    if (p.acc.mode) {  // Featurizer term (the arithmetic of the emit kernels, norm.hip / adapter.hip)
        float a = p.acc.w, c0 = 0.f;
        if (p.acc.norm) {
            const float invC = 1.f / (float)p.C;
            const float m = wave_sum(sum) * invC;
            float qq = 0.f;
#pragma unroll
            for (int i = 0; i < NCH; ++i) {
                const int ch = lane + 64 * i;
                if (ch < nch) {
                    const float d0 = y[i].x - m, d1 = y[i].y - m, d2 = y[i].z - m, d3 = y[i].w - m;
                    qq += (d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3);
                }
            }
            a = p.acc.w * rsqrtf(wave_sum(qq) * invC + LN_EPS);
            c0 = -m * a;
        }
#pragma unroll
        for (int i = 0; i < NCH; ++i) {
            const int ch = lane + 64 * i;
            if (ch >= nch) continue;
            float4* d = (float4*)(p.acc.acc + srow + 4 * ch);
            float4 tt = p.acc.init ? make_float4(0.f, 0.f, 0.f, 0.f) : *d;
            tt.x += fmaf(y[i].x, a, c0);
            tt.y += fmaf(y[i].y, a, c0);
            tt.z += fmaf(y[i].z, a, c0);
            tt.w += fmaf(y[i].w, a, c0);
            *d = tt;
        }
    }
}

// a wave per (row, group)
__global__ __launch_bounds__(256) void argmax_gather_kernel(ArgmaxGatherParams p) {
    const long item = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (item >= p.rows * p.G) return;
    const int lane = threadIdx.x & 63;
    const int g = (int)(item % p.G);
    const float* sc = p.scores + item * p.V;
    float bv = -INFINITY;
    int bi = INT_MAX;
    for (int v = lane; v < p.V; v += 64) {
        const float x = sc[v];
        if (x > bv || bi == INT_MAX) {  // strict: the lowest index of equal values stays
            bv = x;
            bi = v;
        }
    }
    for (int o = 32; o; o >>= 1) {
        const float ov = __shfl_xor(bv, o);
        const int oi = __shfl_xor(bi, o);
        if (oi != INT_MAX && (bi == INT_MAX || ov > bv || (ov == bv && oi < bi))) {
            bv = ov;
            bi = oi;
        }
    }
    if (p.ids && lane == 0) p.ids[item] = (long long)bi;
    if (p.out) {
        const float* src = p.table + ((long)(p.shared ? 0 : g) * p.V + bi) * p.Dv;
        float* dst = p.out + item * p.Dv;  // (rows, G, Dv)
        for (int j = lane; j < p.Dv; j += 64) dst[j] = src[j];
    }
}

__global__ __launch_bounds__(256) void relu_kernel(float4* x, long n4) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n4) return;
    float4 v = x[i];
    x[i] = make_float4(fmaxf(v.x, 0.f), fmaxf(v.y, 0.f), fmaxf(v.z, 0.f), fmaxf(v.w, 0.f));
}

__global__ __launch_bounds__(256) void w2v_pad_rows_kernel(const float* x, int rows, int C, int pad, int pad_zero, float* dst) {
    const int r = blockIdx.x, b = blockIdx.y;
    const int t = r < pad ? 0 : r - pad;
    const bool zero = r < pad && pad_zero;
    const float* src = x + ((long)b * rows + t) * C;
    float* d = dst + ((long)b * (pad + rows) + r) * C;
    for (int ch = threadIdx.x; ch < (C >> 2); ch += 256)
        *(float4*)(d + 4 * ch) = zero ? make_float4(0.f, 0.f, 0.f, 0.f) : *(const float4*)(src + 4 * ch);
}

// block (group, utterance): {mean, rstd} of the rows x Cg block, double sums in a fixed order
__global__ __launch_bounds__(256) void kmeans_stats_kernel(const float* proj, int rows, int C, int G, float2* stats) {
    const int g = blockIdx.x, b = blockIdx.y;
    const int Cg = C / G, q4 = Cg >> 2;
    const float* base = proj + (long)b * rows * C + (long)g * Cg;
    double s = 0, q = 0;
    for (long i = threadIdx.x; i < (long)rows * q4; i += 256) {
        const long t = i / q4;
        const int j = (int)(i - t * q4);
        const float4 v = *(const float4*)(base + t * C + 4 * j);
        s += ((double)v.x + (double)v.y) + ((double)v.z + (double)v.w);
        q += ((double)v.x * v.x + (double)v.y * v.y) + ((double)v.z * v.z + (double)v.w * v.w);
    }
    s = wave_sum_d(s);
    q = wave_sum_d(q);
    __shared__ double sh[8];
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        sh[2 * w] = s;
        sh[2 * w + 1] = q;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const double n = (double)rows * Cg;
        const double mu = ((sh[0] + sh[2]) + (sh[4] + sh[6])) / n;
        double var = ((sh[1] + sh[3]) + (sh[5] + sh[7])) / n - mu * mu;
        var = var > 0 ? var : 0;
        stats[(long)b * G + g] = make_float2((float)mu, (float)(1.0 / sqrt(var + (double)LN_EPS)));
    }
}

constexpr int KM_CG_MAX = 512;
// a wave per (row, group): the normalised projection in LDS, lane v walks codeword v (emb_t is (G, Cg, V): consecutive lanes read
// consecutive addresses)
__global__ __launch_bounds__(256) void kmeans_scores_kernel(const float* proj, const float2* stats, const float* gamma, const float* beta,
                                                            const float* emb_t, long items, int rows, int C, int G, int V,
                                                            float* scores) {
    __shared__ float zs[4][KM_CG_MAX];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long item = (long)blockIdx.x * 4 + wave;
    const bool active = item < items;
    const int Cg = C / G;
    int g = 0;
    if (active) {
        const long row = item / G;
        g = (int)(item - row * G);
        const int b = (int)(row / rows);
        const float2 st = stats[(long)b * G + g];
        const float* xr = proj + row * C + (long)g * Cg;
        for (int j = lane; j < Cg; j += 64) {
            const int c = g * Cg + j;
            zs[wave][j] = fmaf((xr[j] - st.x) * st.y, gamma[c], beta[c]);
        }
    }
    __syncthreads();
    if (!active) return;
    const float* eg = emb_t + (long)g * Cg * V;
    for (int v = lane; v < V; v += 64) {
        float d = 0.f;
        for (int j = 0; j < Cg; ++j) {
            const float df = zs[wave][j] - eg[(long)j * V + v];
            d = fmaf(df, df, d);
        }
        scores[item * V + v] = -d;
    }
}

}  // namespace

hipError_t launch_gn1_apply(const Gn1ApplyParams& p, hipStream_t s) {
    if (p.B <= 0 || p.rows <= 0) return hipSuccess;
    if ((p.C & 3) || p.C > 1024 || p.pad < 0 || (!p.dst && p.pad) || (p.x_bs & 3) || (p.dst_bs & 3) || (p.res_bs & 3))
        return hipErrorInvalidValue;
    const long R = (long)p.B * (p.pad + p.rows);
    dim3 grid((unsigned)((R + 3) / 4)), block(256);
    const int per_lane = ((p.C >> 2) + 63) / 64;
    switch (per_lane) {
        case 1: hipLaunchKernelGGL(gn1_apply_kernel<1>, grid, block, 0, s, p); break;
        case 2: hipLaunchKernelGGL(gn1_apply_kernel<2>, grid, block, 0, s, p); break;
        case 3: hipLaunchKernelGGL(gn1_apply_kernel<3>, grid, block, 0, s, p); break;
        default: hipLaunchKernelGGL(gn1_apply_kernel<4>, grid, block, 0, s, p); break;
    }
    return hipGetLastError();
}

hipError_t launch_argmax_gather(const ArgmaxGatherParams& p, hipStream_t s) {
    if (p.rows <= 0) return hipSuccess;
    if (p.G < 1 || p.V < 1 || p.Dv < 1 || !p.scores || (p.out && !p.table)) return hipErrorInvalidValue;
    const long items = p.rows * p.G;
    hipLaunchKernelGGL(argmax_gather_kernel, dim3((unsigned)((items + 3) / 4)), dim3(256), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_relu(float* x, long n, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    if (n & 3) return hipErrorInvalidValue;
    hipLaunchKernelGGL(relu_kernel, dim3((unsigned)((n / 4 + 255) / 256)), dim3(256), 0, s, (float4*)x, n / 4);
    return hipGetLastError();
}

hipError_t launch_w2v_pad_rows(const float* x, int B, int rows, int C, int pad, int pad_zero, float* dst, hipStream_t s) {
    if (B <= 0 || rows <= 0) return hipSuccess;
    if ((C & 3) || pad < 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(w2v_pad_rows_kernel, dim3(pad + rows, B), dim3(256), 0, s, x, rows, C, pad, pad_zero, dst);
    return hipGetLastError();
}

hipError_t launch_kmeans_stats(const float* proj, int B, int rows, int C, int G, float2* stats, hipStream_t s) {
    if (B <= 0 || rows <= 0) return hipSuccess;
    if (G < 1 || C % G || ((C / G) & 3)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(kmeans_stats_kernel, dim3(G, B), dim3(256), 0, s, proj, rows, C, G, stats);
    return hipGetLastError();
}

hipError_t launch_kmeans_scores(const float* proj, const float2* stats, const float* gamma, const float* beta, const float* emb_t,
                                int B, int rows, int C, int G, int V, float* scores, hipStream_t s) {
    if (B <= 0 || rows <= 0) return hipSuccess;
    if (G < 1 || C % G || C / G > KM_CG_MAX || V < 1) return hipErrorInvalidValue;
    const long items = (long)B * rows * G;
    hipLaunchKernelGGL(kmeans_scores_kernel, dim3((unsigned)((items + 3) / 4)), dim3(256), 0, s, proj, stats, gamma, beta, emb_t, items,
                       rows, C, G, V, scores);
    return hipGetLastError();
}

}  // namespace s3

// ---- the handle's side: configuration, weights, forward ------------------------------------------------------------------
namespace s3e {

static const char* dtype_name(int d) { return d == 1 ? "bf16" : d == 2 ? "fp16" : d == 3 ? "fp32x3" : d == 4 ? "fp16x2" : "fp32"; }

// the family's configuration as one object: the extractor fields of s3enc_config beside the aggregator / quantizer block
struct W2vCfg : s3enc_config, s3enc_wav2vec_config {
    W2vCfg(const s3enc_config& a, const s3enc_wav2vec_config& b) : s3enc_config(a), s3enc_wav2vec_config(b) {}
};

static int wav2vec_check_config(const W2vCfg& c) {
    if (c.compute_dtype < 0 || c.compute_dtype > 4) return fail("config: unknown compute_dtype");
    if (c.compute_dtype != S3ENC_F32)
        return fail(std::string("config: wav2vec / vq-wav2vec (conv extractor + aggregator) are built for compute dtype fp32 only; ") +
                    dtype_name(c.compute_dtype) + " is not built");
    if (c.w2v_aggregator != 0) return fail("config: wav2vec aggregator=\"gru\" is not built (only the convolutional aggregator \"cnn\")");
    if (c.w2v_activation != 0) return fail("config: wav2vec activation=\"gelu\" is not built (only \"relu\", the released models)");
    if (c.w2v_skip_feat) return fail("config: wav2vec skip_connections_feat is not built (off in the released models)");
    if (c.n_conv < 2 || c.n_conv > S3ENC_MAX_CONV) return fail("config: n_conv out of range");
    if (c.conv_kernel[0] != 10) return fail("config: the conv0 kernel is specialised for kernel width 10");
    if (c.conv_stride[0] < 1 || c.conv_stride[0] > 8) return fail("config: conv0 stride must be 1..8");
    if (c.conv_dim < 32 || c.conv_dim % 32 || c.conv_dim > 1024) return fail("config: conv_dim must be a multiple of 32, <= 1024");
    for (int i = 1; i < c.n_conv; ++i)
        if (c.conv_kernel[i] < 1 || c.conv_kernel[i] > 64 || c.conv_stride[i] < 1 || c.conv_stride[i] > 16)
            return fail("config: conv kernel / stride out of range");
    if (c.n_agg < 1 || c.n_agg > S3ENC_MAX_CONV) return fail("config: wav2vec needs 1..16 aggregator layers");
    if (c.encoder_layers != c.n_agg) return fail("config: wav2vec encoder_layers must equal the aggregator layer count");
    for (int j = 0; j < c.n_agg; ++j) {
        if (c.agg_dim[j] != c.conv_dim)
            return fail("config: wav2vec layers of unequal widths are not built (the aggregator would need residual_proj)");
        if (c.agg_stride[j] != 1) return fail("config: wav2vec aggregator strides other than 1 are not built");
        if (c.agg_kernel[j] < 1 || c.agg_kernel[j] > 64) return fail("config: wav2vec aggregator kernel out of range (1..64)");
    }
    if (!(c.residual_scale > 0.f)) return fail("config: wav2vec residual_scale must be positive");
    if (c.vq_type < 0 || c.vq_type > 2) return fail("config: unknown vq_type (0 none, 1 gumbel, 2 kmeans)");
    if (c.vq_type) {
        if (c.vq_groups < 1 || c.vq_groups > 16 || c.conv_dim % c.vq_groups || ((c.conv_dim / c.vq_groups) & 3))
            return fail("config: vq_groups must divide the width into multiples of 4");
        if (c.vq_dim != c.conv_dim) return fail("config: vq_dim must equal the extractor width (the aggregator reads the codewords)");
        if (c.vq_vars < 1 || c.vq_vars > 65536) return fail("config: vq_vars out of range");
        if (c.vq_depth < 1 || c.vq_depth > 8) return fail("config: vq_depth out of range (1..8)");
        if (c.vq_type == 2 && c.conv_dim / c.vq_groups > 512) return fail("config: k-means group width > 512");
    }
    return 0;
}

static int wav2vec_create(s3enc_encoder* e, const Ckpt& ck) {
    const W2vCfg c(e->cfg, e->w2v_cfg);
    const int C = c.conv_dim;
    e->w2v.reset(new W2vW());
    W2vW& w = *e->w2v;
    std::vector<float> t, t2;
    const bool affine = !c.non_affine_group_norm;
    w.ext_w.resize(c.n_conv);
    w.ext_g.resize(c.n_conv);
    w.ext_b.resize(c.n_conv);
    for (int i = 0; i < c.n_conv; ++i) {
        const std::string p = "feature_extractor.conv_layers." + std::to_string(i);
        const int cin = i == 0 ? 1 : C, k = c.conv_kernel[i];
        GET(p + ".0.weight", (long)C * cin * k, t);
        if (i == 0) {
            UP(upload_f32(w.ext_w[i], t));  // [C][k]
        } else {
            tap_major(t, C, cin, k, t2);
            UP(upload_f32(w.ext_w[i], t2));
        }
        if (affine) {
            GET(p + ".2.weight", C, t);
            UP(upload_f32(w.ext_g[i], t));
            GET(p + ".2.bias", C, t);
            UP(upload_f32(w.ext_b[i], t));
        }
    }
    w.agg_w.resize(c.n_agg);
    w.agg_bias.resize(c.n_agg);
    w.agg_g.resize(c.n_agg);
    w.agg_b.resize(c.n_agg);
    for (int j = 0; j < c.n_agg; ++j) {
        const std::string p = "feature_aggregator.conv_layers." + std::to_string(j);
        const int k = c.agg_kernel[j];
        GET(p + ".1.weight", (long)C * C * k, t);
        tap_major(t, C, C, k, t2);
        UP(upload_f32(w.agg_w[j], t2));
        if (!c.no_conv_bias) {
            GET(p + ".1.bias", C, t);
            UP(upload_f32(w.agg_bias[j], t));
        }
        if (affine) {
            GET(p + ".3.weight", C, t);
            UP(upload_f32(w.agg_g[j], t));
            GET(p + ".3.bias", C, t);
            UP(upload_f32(w.agg_b[j], t));
        }
    }
    const int G = c.vq_groups, V = c.vq_vars, Gt = c.combine_groups ? 1 : G;
    const int Dv = c.vq_type ? C / G : 0;
    if (c.vq_type == 1) {
        const int d = c.vq_depth;
        w.vq_w.resize(d);
        w.vq_b.resize(d);
        for (int i = 0; i < d; ++i) {
            const bool last = i == d - 1;
            const long in = i == 0 ? C : 2L * C, outn = last ? (long)G * V : 2L * C;
            const std::string p = d == 1 ? std::string("vector_quantizer.weight_proj")
                                         : "vector_quantizer.weight_proj." + std::to_string(i) + (last ? "" : ".0");
            GET(p + ".weight", outn * in, t);
            UP(upload_f32(w.vq_w[i], t));
            GET(p + ".bias", outn, t);
            UP(upload_f32(w.vq_b[i], t));
        }
        GET("vector_quantizer.vars", (long)Gt * V * Dv, t);  // (1, Gt * V, Dv)
        UP(upload_f32(w.table, t));
    } else if (c.vq_type == 2) {
        GET("vector_quantizer.embedding", (long)V * Gt * Dv, t);  // (V, Gt, Dv)
        t2.resize(t.size());
        for (int v = 0; v < V; ++v)
            for (int g = 0; g < Gt; ++g)
                for (int j = 0; j < Dv; ++j) t2[((long)g * V + v) * Dv + j] = t[((long)v * Gt + g) * Dv + j];
        UP(upload_f32(w.table, t2));  // (Gt, V, Dv): the gather table
        std::vector<float> et((size_t)G * Dv * V);  // (G, Dv, V), shared variables repeated: the distance kernel's operand
        for (int g = 0; g < G; ++g)
            for (int j = 0; j < Dv; ++j)
                for (int v = 0; v < V; ++v) et[((long)g * Dv + j) * V + v] = t[((long)v * Gt + (c.combine_groups ? 0 : g)) * Dv + j];
        UP(upload_f32(w.emb_t, et));
        GET("vector_quantizer.projection.0.weight", (long)C * Dv, t);  // Conv1d(C, C, 1, groups = G): (C, C / G, 1)
        w.km_w.resize(G);
        for (int g = 0; g < G; ++g) {
            t2.assign(t.begin() + (long)g * Dv * Dv, t.begin() + (long)(g + 1) * Dv * Dv);
            UP(upload_f32(w.km_w[g], t2));
        }
        GET("vector_quantizer.projection.1.weight", C, t);
        UP(upload_f32(w.km_g, t));
        GET("vector_quantizer.projection.1.bias", C, t);
        UP(upload_f32(w.km_b, t));
    }
    return 0;
}

static int wav2vec_forward(s3enc_handle e, const float* const* wav_ptrs_host, const int64_t* lengths, int32_t B, int64_t n_max_in,
                    const FwdOpts& fo, void* out, int64_t layer_stride, hipStream_t st) {
    const W2vCfg c(e->cfg, e->w2v_cfg);
    const W2vW& w = *e->w2v;
    const int C = c.conv_dim, NA = c.n_agg, NS = NA + 1;
    if (fo.selection != S3ENC_SEL_HIDDEN)
        return fail("s3enc_forward: feature_selection is not defined for wav2vec / vq-wav2vec (the reference expert has one hidden_states list)");
    if (fo.featurize && !fo.w) return fail("s3enc_forward: featurize needs feat_w");
    if (!fo.featurize && fo.out_dtype != F32) return fail("s3enc_forward: out_dtype must be S3ENC_F32 for a wav2vec handle");
    if ((e->aux_codewords || e->aux_codeids) && !c.vq_type)
        return fail("s3enc_forward_aux: codewords / codeids need a vector quantizer (vq_type gumbel or kmeans)");
    long n_max;
    if (batch_n_max(wav_ptrs_host, lengths, B, n_max_in, n_max)) return 1;
    std::vector<long> L(c.n_conv);
    for (int i = 0; i < c.n_conv; ++i) L[i] = conv_len(c, n_max, i + 1);
    const long T = L[c.n_conv - 1];
    if (T < 1) return fail("s3enc_forward: input shorter than the receptive field of the conv stack");
    const long M = (long)B * T;
    if (check_out(out, fo, layer_stride, M * C)) return 1;
    if (((uintptr_t)e->aux_codewords & 15) || ((uintptr_t)e->aux_codeids & 7)) return fail("s3enc_forward_aux: misaligned output");
    long max_rows = 0;
    for (int i = 0; i < c.n_conv; ++i) max_rows = std::max(max_rows, L[i]);
    if ((long)B * max_rows * C >= (1L << 40)) return fail("s3enc_forward: batch too large");
    DeviceGuard dg(e->device);
    if (!dg.ok) return fail("s3enc_forward: hipSetDevice failed");

    // ---- small device state: waveform table, conv0's table, statistics partials ----
    const size_t tbl_bytes = (size_t)B * 16;
    const size_t part_elems = stats_partial_elems(B, n_max);
    const int G = c.vq_groups;
    char* d_tbl;
    float2 *d_norm, *d_gn, *d_kst;
    double *d_part, *d_gpart;
    for (int pass = 0; pass < 2; ++pass) {
        Bump sb(pass ? e->small.p : nullptr);
        d_tbl = (char*)sb.take(tbl_bytes);
        d_norm = (float2*)sb.take((size_t)B * sizeof(float2));
        d_gn = (float2*)sb.take((size_t)B * C * sizeof(float2));
        d_part = (double*)sb.take(part_elems * 8);
        d_gpart = (double*)sb.take((size_t)B * GS_BLOCKS * 2 * 8);
        d_kst = (float2*)sb.take((size_t)B * (G > 0 ? G : 1) * sizeof(float2));
        if (!pass) HIP_TRY(e->small.ensure_on_stream(sb.off + 1024, st));
    }
    char* hp;
    if (stage_begin(e, tbl_bytes, st, hp)) return 1;
    memcpy(hp, wav_ptrs_host, (size_t)B * 8);
    for (int b = 0; b < B; ++b) ((long*)(hp + (size_t)B * 8))[b] = (long)lengths[b];
    if (stage_commit(e, hp, d_tbl, tbl_bytes, st)) return 1;
    const float* const* d_ptrs = (const float* const*)d_tbl;
    const long* d_lens = (const long*)(d_tbl + (size_t)B * 8);

    // ---- workspace ----
    int maxpad = 0;
    for (int j = 0; j < NA; ++j) maxpad = std::max(maxpad, c.agg_kernel[j] - 1);
    const int V = c.vq_vars, Dv = c.vq_type ? C / G : 0;
    float *actA, *actB, *P0, *P1, *Rg, *zbuf = nullptr, *h0 = nullptr, *h1 = nullptr, *scores = nullptr, *cw = nullptr, *proj = nullptr;
    long long* ids = nullptr;
    for (int pass = 0; pass < 2; ++pass) {
        Bump wb(pass ? e->ws.p : nullptr);
        actA = (float*)wb.take((size_t)B * L[0] * C * 4);
        actB = (float*)wb.take((size_t)B * L[1] * C * 4);
        P0 = (float*)wb.take((size_t)B * (maxpad + T) * C * 4);
        P1 = (float*)wb.take((size_t)B * (maxpad + T) * C * 4);
        Rg = (float*)wb.take((size_t)M * C * 4);
        if (c.vq_type) {
            zbuf = (float*)wb.take((size_t)M * C * 4);
            scores = (float*)wb.take((size_t)M * G * V * 4);
            cw = (float*)wb.take((size_t)M * C * 4);
            ids = (long long*)wb.take((size_t)M * G * 8);
            if (c.vq_type == 1 && c.vq_depth > 1) {
                h0 = (float*)wb.take((size_t)M * 2 * C * 4);
                h1 = (float*)wb.take((size_t)M * 2 * C * 4);
            }
            if (c.vq_type == 2) proj = (float*)wb.take((size_t)M * C * 4);
        }
        if (!pass) HIP_TRY(e->ws.ensure_on_stream(wb.off + 4096, st));
    }
    e->taps.clear();
    if (e->aux_codewords) cw = e->aux_codewords;
    if (e->aux_codeids) ids = e->aux_codeids;

    // ---- where the states go ----
    Sink sink{e, st, fo.featurize ? 2 : 0, out, (long)layer_stride, F32, M, C, fo.w, fo.feat_norm};
    HIP_TRY(sink.zero_without_terms(NS, M));
    auto stats = [&](const float* x, long rows) -> hipError_t {
        Prof pr(e, st, "gn1_stats", 0, 4.0 * B * rows * C);
        return launch_group1_stats(x, rows * C, rows * C, B, d_gpart, st);
    };

    // ---- conv0: closed-form GroupNorm(1, C) statistics, normalisation + ReLU in the conv kernel ----
    WavTable wt{d_ptrs, d_lens, B, n_max};
    HIP_TRY(launch_wav_norm_stats(wt, 0, d_part, d_norm, st, 0.f));  // (no waveform normalisation: identity {0, 1})
    {
        Prof pr(e, st, "gn1_wav_stats", 0, 4.0 * B * n_max);
        HIP_TRY(launch_gn1_stats(wt, d_norm, (const float*)w.ext_w[0].p, (const float*)w.ext_g[0].p, (const float*)w.ext_b[0].p, C,
                                 c.conv_kernel[0], c.conv_stride[0], L[0], d_part, d_gn, st));
    }
    {
        Conv0Params p{};
        p.wav = wt;
        p.norm = d_norm;
        p.w0 = (const float*)w.ext_w[0].p;
        p.gn = d_gn;
        p.C = C;
        p.k0 = c.conv_kernel[0];
        p.s0 = c.conv_stride[0];
        p.L0 = L[0];
        p.out = actA;
        p.nt = tuning().conv0_nt;
        p.relu = 1;
        Prof pr(e, st, "conv0", 2.0 * B * L[0] * C * p.k0, 4.0 * B * n_max + 4.0 * B * L[0] * C);
        HIP_TRY(launch_conv0(F32, p, st));
    }
    const int pad0 = c.agg_kernel[0] - 1;
    const float rscale = std::sqrt(c.residual_scale);
    // ---- extractor layers 1..: raw implicit GEMM, statistics, apply (in place; the last one into the aggregator's operand) ----
    float* cur = actA;
    for (int i = 1; i < c.n_conv; ++i) {
        const bool last = i == c.n_conv - 1;
        float* raw = cur == actA ? actB : actA;
        GemmParams g{};
        g.A = cur;
        g.lda = (long)c.conv_stride[i] * C;
        g.a_bs = L[i - 1] * C;
        g.W = w.ext_w[i].p;
        g.M = (int)L[i];
        g.N = C;
        g.K = c.conv_kernel[i] * C;
        g.batches = B;
        g.out32 = raw;
        g.ldo = C;
        g.o_bs = L[i] * C;
        {
            char kind[32];
            snprintf(kind, sizeof(kind), "gemm:w2v_conv%d", i);
            Prof pr(e, st, kind, 2.0 * B * L[i] * C * g.K, 4.0 * ((double)B * L[i - 1] * C + (double)C * g.K + (double)B * L[i] * C));
            HIP_TRY(launch_gemm(F32, g, st));
        }
        HIP_TRY(stats(raw, L[i]));
        Gn1ApplyParams a{};
        a.x = raw;
        a.x_bs = L[i] * C;
        a.partial = d_gpart;
        a.count = (double)L[i] * C;
        a.gamma = (const float*)w.ext_g[i].p;
        a.beta = (const float*)w.ext_b[i].p;
        a.B = B;
        a.rows = (int)L[i];
        a.C = C;
        if (!last) {
            a.dst = raw;
            a.dst_bs = L[i] * C;
        } else {
            a.log = c.log_compression;
            if (c.vq_type) {  // the quantizer reads z as contiguous rows
                a.dst = zbuf;
                a.dst_bs = T * C;
            } else {
                a.dst = P0;
                a.pad = pad0;
                a.pad_zero = c.agg_zero_pad;
                a.dst_bs = (long)(pad0 + T) * C;
            }
            a.state = sink.slot32(0);
            a.acc = sink.acc(0, 2);
        }
        {
            Prof pr(e, st, "gn1_apply", 0, 4.0 * B * L[i] * C * (last ? 3 : 2));
            HIP_TRY(launch_gn1_apply(a, st));
        }
        cur = raw;
    }
    HIP_TRY(sink.done(0));

    // ---- vector quantizer: codewords replace z as the aggregator's input ----
    if (c.vq_type) {
        if (c.vq_type == 1) {
            const float* h = zbuf;
            int in = C;
            for (int i = 0; i + 1 < c.vq_depth; ++i) {
                float* o = (i & 1) ? h1 : h0;
                HIP_TRY(linear_f32(e, st, {"gemm:w2v_vq_proj", h, w.vq_w[i].p, w.vq_b[i].p, M, 2 * C, in, 0, nullptr, o}));
                {
                    Prof pr(e, st, "w2v_relu", 0, 8.0 * M * 2 * C);
                    HIP_TRY(launch_relu(o, M * 2L * C, st));
                }
                h = o;
                in = 2 * C;
            }
            const int d = c.vq_depth - 1;
            HIP_TRY(linear_f32(e, st, {"gemm:w2v_vq_logits", h, w.vq_w[d].p, w.vq_b[d].p, M, G * V, in, 0, nullptr, scores}));
        } else {
            for (int g = 0; g < G; ++g)
                HIP_TRY(linear_f32(e, st, {"gemm:w2v_km_proj", zbuf + (long)g * Dv, w.km_w[g].p, nullptr, M, Dv, Dv, 0, nullptr, proj + (long)g * Dv, nullptr, C, C}));
            Prof pr(e, st, "w2v_kmeans", 3.0 * M * G * V * Dv, 4.0 * ((double)M * C * 2 + (double)M * G * V));
            HIP_TRY(launch_kmeans_stats(proj, B, (int)T, C, G, d_kst, st));
            HIP_TRY(launch_kmeans_scores(proj, d_kst, (const float*)w.km_g.p, (const float*)w.km_b.p, (const float*)w.emb_t.p, B, (int)T,
                                         C, G, V, scores, st));
        }
        {
            ArgmaxGatherParams ag{};
            ag.scores = scores;
            ag.table = (const float*)w.table.p;
            ag.shared = c.combine_groups;
            ag.rows = M;
            ag.G = G;
            ag.V = V;
            ag.Dv = Dv;
            ag.ids = ids;
            ag.out = cw;
            Prof pr(e, st, "w2v_argmax_gather", 0, 4.0 * ((double)M * G * V + (double)M * C));
            HIP_TRY(launch_argmax_gather(ag, st));
        }
        Prof pr(e, st, "w2v_pad_rows", 0, 8.0 * M * C);
        HIP_TRY(launch_w2v_pad_rows(cw, B, (int)T, C, pad0, c.agg_zero_pad, P0, st));
    }

    // ---- aggregator: causal convolutions over k - 1 pad rows + T frames, skip connections ----
    float* pin = P0;
    for (int j = 0; j < NA; ++j) {
        const int k = c.agg_kernel[j], pad = k - 1;
        const bool last = j == NA - 1;
        const int npad = last ? 0 : c.agg_kernel[j + 1] - 1;
        float* pout = pin == P0 ? P1 : P0;
        GemmParams g{};
        g.A = pin;
        g.lda = C;
        g.a_bs = (long)(pad + T) * C;
        g.W = w.agg_w[j].p;
        g.bias = (const float*)w.agg_bias[j].p;
        g.M = (int)T;
        g.N = C;
        g.K = k * C;
        g.batches = B;
        g.out32 = Rg;
        g.ldo = C;
        g.o_bs = T * C;
        {
            Prof pr(e, st, "gemm:w2v_agg", 2.0 * M * C * g.K, 4.0 * ((double)B * (pad + T) * C + (double)C * g.K + (double)M * C));
            HIP_TRY(launch_gemm(F32, g, st));
        }
        HIP_TRY(stats(Rg, T));
        Gn1ApplyParams a{};
        a.x = Rg;
        a.x_bs = T * C;
        a.partial = d_gpart;
        a.count = (double)T * C;
        a.gamma = (const float*)w.agg_g[j].p;
        a.beta = (const float*)w.agg_b[j].p;
        if (c.skip_connections_agg) {
            a.res = pin + (long)pad * C;
            a.res_bs = (long)(pad + T) * C;
            a.scale = rscale;
        }
        a.B = B;
        a.rows = (int)T;
        a.C = C;
        if (!last) {
            a.dst = pout;
            a.pad = npad;
            a.pad_zero = c.agg_zero_pad;
            a.dst_bs = (long)(npad + T) * C;
        }
        a.state = sink.slot32(j + 1);
        a.acc = sink.acc(j + 1, 2);
        {
            Prof pr(e, st, "gn1_apply", 0, 4.0 * M * C * (2 + (a.res ? 1 : 0) + (a.dst ? 1 : 0)));
            HIP_TRY(launch_gn1_apply(a, st));
        }
        HIP_TRY(sink.done(j + 1));
        pin = pout;
    }
    return 0;
}


// every selection is defined; frames, mask rule and rate are the conv stack's (valid_frames: the frames an utterance's own samples reach)
FamilyOps kWav2vecFamily = {
    S3ENC_WAV2VEC, "wav2vec", "S3ENC_WAV2VEC", "s3enc_create_ex", "the wav2vec family needs its aggregator / quantizer block", nullptr,
    [](const s3enc_config& c, const void* b) { return wav2vec_check_config(W2vCfg(c, *(const s3enc_wav2vec_config*)b)); },
    [](s3enc_encoder* e, const Ckpt& ck, const void* b) { e->w2v_cfg = *(const s3enc_wav2vec_config*)b; return wav2vec_create(e, ck); },
    wav2vec_forward};

}  // namespace s3e
