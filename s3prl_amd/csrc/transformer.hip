// transformer.hip — what every Transformer encoder of the engine shares (declared in engine_internal.h): the un-batched Linear, the
// layer's weights from a checkpoint, and the schedule of one layer in either LayerNorm order.
#include "engine_internal.h"

namespace s3e {

static GemmParams gemm_of(const Linear& l) {
    GemmParams g{};
    g.A = l.A;
    g.lda = l.lda ? l.lda : l.K;
    g.W = l.W;
    g.W_x3 = l.W_x3;
    g.bias = (const float*)l.bias;
    g.M = (int)l.M;
    g.N = l.N;
    g.K = l.K;
    g.batches = 1;
    g.act = l.act;
    g.residual = l.residual;
    g.res_ln_stats = l.res_ln_stats;
    g.res_ln_g = l.res_ln_g;
    g.res_ln_b = l.res_ln_b;
    g.out32 = l.out32;
    g.out16 = l.out16;
    g.ldo = l.ldo ? l.ldo : l.N;
    return g;
}
// the record every Linear opens: 2 M N K flops; bytes: both operands, the output and the fp32 residual
static double linear_flops(const Linear& l) { return 2.0 * l.M * l.N * l.K; }
static double linear_bytes(const Linear& l, int es_in, int es_out) {
    const double M = (double)l.M, N = l.N, K = l.K;
    return (M * K + N * K) * es_in + M * N * es_out + (l.residual ? 4.0 * M * N : 0.0);
}

hipError_t linear_f32(s3enc_encoder* e, hipStream_t st, const Linear& l) {
    Prof pr(e, st, l.kind, linear_flops(l), linear_bytes(l, 4, 4));
    return launch_gemm(F32, gemm_of(l), st);
}

GemmParams linear_params(const s3enc_encoder* e, const Linear& l) { return wsplit_of(e, gemm_of(l)); }

int linear(s3enc_encoder* e, hipStream_t st, const Linear& l) {
    Prof pr(e, st, l.kind, linear_flops(l), linear_bytes(l, e->es, l.out32 ? 4 : e->es));
    if (l.x3_or_fail) {
        const GemmParams g = gemm_of(l);
        if (!gemm_x3_eligible(g)) return fail(std::string(l.x3_or_fail) + " is not a shape of the three-term GEMM (internal)");
        HIP_TRY(launch_gemm(F32, g, st));
    } else {
        HIP_TRY(launch_gemm(e->dtype, linear_params(e, l), st));
    }
    return 0;
}

// ---- the layer's weights ------------------------------------------------------------------------------------------------------------
const LayerNames kFairseqLayer = {{"self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj"}, "self_attn.out_proj", "self_attn_layer_norm",
                                  "fc1", "fc2", "final_layer_norm"};
const LayerNames kBertLayer = {{"attention.self.query", "attention.self.key", "attention.self.value"}, "attention.output.dense",
                               "attention.output.LayerNorm", "intermediate.dense", "output.dense", "output.LayerNorm"};
// timm's VisionTransformer Block (SSAST): one fused attn.qkv Linear, rows q | k | v
const LayerNames kTimmLayer = {{nullptr, nullptr, nullptr}, "attn.proj", "norm1", "mlp.fc1", "mlp.fc2", "norm2", "attn.qkv"};

hipError_t upload_gemm_w_mx(s3enc_encoder* e, DevBuf& buf, const std::vector<float>& v, long N, long K, int kind) {
    hipError_t err = upload_gemm_w(buf, v, N, K, e->dtype, e->x2);
    if (err != hipSuccess || !e->x2 || !(tuning().gemm16_mx & (kind | 16))) return err;
    if (!gemm16_mx_weight_rule(N, K) && !((tuning().gemm16_mx & 16) && !(K & 127) && N >= 128)) return err;
    std::unique_ptr<MxImage> img(new MxImage());
    err = upload_mx4_lo(*img, v, N, K);
    if (err != hipSuccess) return err;
    img->kind = kind;
    e->mx_images[buf.p] = std::move(img);
    return hipSuccess;
}

int load_layer(s3enc_encoder* e, const Ckpt& ck, const std::string& p, const LayerNames& n, float qscale, bool gate, LayerW& L) {
    const long D = e->cfg.embed_dim, F = e->cfg.ffn_dim;
    std::vector<float> t, t2, w(3 * D * D), bb(3 * D);
    auto vec = [&](const std::string& name, long elems, DevBuf& d) -> int {
        GET(name, elems, t);
        UP(upload_f32(d, t));
        return 0;
    };
    if (n.qkv_fused) {  // q *= head_dim^-0.5 folded into the first D rows and their bias
        GET(p + n.qkv_fused + ".weight", 3 * D * D, w);
        GET(p + n.qkv_fused + ".bias", 3 * D, bb);
        for (long i = 0; i < D * D; ++i) w[i] *= qscale;
        for (long i = 0; i < D; ++i) bb[i] *= qscale;
    }
    for (int s = 0; s < 3 && !n.qkv_fused; ++s) {
        GET(p + n.qkv[s] + ".weight", D * D, t);
        GET(p + n.qkv[s] + ".bias", D, t2);
        const float sc = s == 0 ? qscale : 1.f;  // q *= head_dim^-0.5 folded into W_q, b_q
        for (long i = 0; i < D * D; ++i) w[s * D * D + i] = t[i] * sc;
        for (long i = 0; i < D; ++i) bb[s * D + i] = t2[i] * sc;
    }
    UP(upload_gemm_w_mx(e, L.wqkv, w, 3 * D, D, 2));
    if (e->x3) UP(upload_x3(L.wqkv3, w, 3 * D, D));
    UP(upload_f32(L.bqkv, bb));
    GET(p + n.out + ".weight", D * D, t);
    UP(upload_gemm_w(L.wo, t, D, D, e->dtype, e->x2));
    if (e->x3 || e->x2_attn_f32) UP(upload_x3(L.wo3, t, D, D));
    if (vec(p + n.out + ".bias", D, L.bo) || vec(p + n.ln1 + ".weight", D, L.ln1g) || vec(p + n.ln1 + ".bias", D, L.ln1b)) return 1;
    GET(p + n.fc1 + ".weight", F * D, t);
    UP(upload_gemm_w_mx(e, L.w1, t, F, D, 4));
    if (e->x3) UP(upload_x3(L.w13, t, F, D));
    if (vec(p + n.fc1 + ".bias", F, L.b1)) return 1;
    GET(p + n.fc2 + ".weight", D * F, t);
    UP(upload_gemm_w_mx(e, L.w2, t, D, F, 8));
    if (e->x3) UP(upload_x3(L.w23, t, D, F));
    if (vec(p + n.fc2 + ".bias", D, L.b2) || vec(p + n.ln2 + ".weight", D, L.ln2g) || vec(p + n.ln2 + ".bias", D, L.ln2b)) return 1;
    if (gate && (vec(p + "self_attn.grep_linear.weight", 8 * 64, L.grep_w) || vec(p + "self_attn.grep_linear.bias", 8, L.grep_b) ||
                 vec(p + "self_attn.grep_a", e->cfg.heads, L.grep_a)))
        return 1;
    return 0;
}

// ---- one layer ----------------------------------------------------------------------------------------------------------------------
// post-LN: q|k|v(x) -> attention -> out_proj + x -> LN1 -> fc1 + GELU -> fc2 + LN1's output -> LN2 = the layer's output
// pre-LN:  LN1(x) -> q|k|v -> attention -> out_proj + x = y -> LN2(y) -> fc1 + GELU -> fc2 + y = the layer's output
int encoder_layer(s3enc_encoder* e, hipStream_t st, const LayerW& Lw, const LayerRun& r) {
    const int D = e->cfg.embed_dim, F = e->cfg.ffn_dim, H = e->cfg.heads, dt = e->dtype, es = e->es;
    const bool f32 = dt == F32, prel = r.pre_ln, ffn_tap = r.ffn_out32 != nullptr;
    const long M = (long)r.B * r.T;
    const double gM = (double)M;
    // a LayerNorm of the layer: fp32 operand modes write out32 alone, the 16-bit ones out16 (and out32 where it is asked for)
    auto ln = [&](const char* kind, int bytes, const float* x, const DevBuf& g, const DevBuf& b, float* out32, void* out16, const LnAcc& fa,
                  const LnGate& gt, float2* stats) -> hipError_t {
        Prof pr(e, st, kind, 0, gM * D * bytes);
        if (r.ln_eps > 0.f) {  // the checkpoint's own eps: the eps-taking row LayerNorm (fp32 in, fp32 out, nothing fused)
            if (!f32 || !prel || !out32 || out16 || fa.acc || gt.gate || stats) return hipErrorInvalidValue;
            LnEpsParams q{};
            q.x = x;
            q.gamma = (const float*)g.p;
            q.beta = (const float*)b.p;
            q.eps = r.ln_eps;
            q.rows = M;
            q.C = D;
            q.out = out32;
            return launch_layernorm_eps(q, st);
        }
        return launch_layernorm(dt, x, (const float*)g.p, (const float*)b.p, M, D, 0, out32, out16, st, fa, gt, stats);
    };
    const void* a_in = f32 ? (const void*)r.x : r.x16;  // operand of the q|k|v GEMM
    if (prel) {
        // WavLM: the gate reads LN1's output — computed inside this pass (no fp32 copy, no separate kernel)
        HIP_TRY(ln("layernorm:ln1", 4 + es, r.x, Lw.ln1g, Lw.ln1b, f32 ? (float*)r.xT : nullptr, f32 ? nullptr : r.xT, r.acc_in, r.gate_here,
                   nullptr));
        a_in = r.xT;
    }
    {
        Linear q{"gemm:qkv", a_in, Lw.wqkv.p, Lw.bqkv.p, M, 3 * D, D};
        q.W_x3 = Lw.wqkv3.p;
        if (f32) q.out32 = (float*)r.qkv; else q.out16 = r.qkv;
        if (linear(e, st, q)) return LAYER_FAILED;
        if (r.taps) e->taps["qkv0"] = {r.qkv, M * 3 * D, dt};
        if (r.stop_after == 30) return LAYER_STOPPED;
    }
    {
        AttnParams a{};
        a.qkv = r.qkv;
        a.out = r.attn;
        a.valid = r.valid;
        a.B = r.B;
        a.T = (int)r.T;
        a.H = H;
        a.bias_table = r.bias_table;
        a.table_R = r.table_R;
        a.gate = r.gate;
        a.out_f32 = e->x2_attn_f32 ? 1 : 0;
        Prof pr(e, st, "attention", 4.0 * r.B * H * (double)r.T * r.T * 64, gM * 4 * D * es);
        HIP_TRY(launch_attention(e->x3 ? 3 : dt, a, st));
        if (r.taps) e->taps["attn0"] = {r.attn, M * D, e->x2_attn_f32 ? (int)F32 : dt};
        if (r.stop_after == 31) return LAYER_STOPPED;
    }
    {   // out_proj + bias + residual
        Linear q{"gemm:out_proj", r.attn, Lw.wo.p, Lw.bo.p, M, D, D};
        q.W_x3 = Lw.wo3.p;
        q.residual = r.x;
        q.out32 = r.tmp1;
        q.x3_or_fail = e->x2_attn_f32 ? "out_proj" : nullptr;
        if (linear(e, st, q)) return LAYER_FAILED;
    }
    if (r.stop_after == 32) return LAYER_STOPPED;  // (behind out_proj)
    Linear fc2{"gemm:fc2", r.hbuf, Lw.w2.p, Lw.b2.p, M, D, F};
    fc2.W_x3 = Lw.w23.p;
    // In the 16-bit modes a post-LN layer's LayerNorm 1 need not write its fp32 output — that tensor is only fc2's residual, and fc2's
    // epilogue can rebuild it from the row it reads anyway and two numbers per row (GemmParams::res_ln_*; -49 MB of stores per layer at
    // the reference batch).  Decided from fc2's shape class (gemm16_res_ln_ok), never from M
    bool ln1_fold = false;
    if (r.allow_ln1_fold && !prel && !f32 && !ffn_tap) {
        Linear probe = fc2;
        probe.residual = r.tmp1;
        probe.out32 = r.tmp1;
        ln1_fold = gemm16_res_ln_ok(dt, linear_params(e, probe));
    }
    const void* ffn_in = r.xT;
    if (prel) {  // b = LN2(y) feeds fc1; residual is y itself
        HIP_TRY(ln("layernorm:ln2", 4 + es, r.tmp1, Lw.ln2g, Lw.ln2b, f32 ? (float*)r.xT : nullptr, f32 ? nullptr : r.xT, LnAcc(), LnGate(),
                   nullptr));
        fc2.residual = r.tmp1;
    } else if (ln1_fold) {  // LN1 writes the fc1 operand and the rows' (mean, rstd); fc2's epilogue rebuilds x1 = LN1(y)
        HIP_TRY(ln("layernorm:ln1", 4 + es, r.tmp1, Lw.ln1g, Lw.ln1b, nullptr, r.xT, LnAcc(), LnGate(), r.lnst));
        fc2.residual = r.tmp1;  // (y itself: fc2 normalises the rows it adds, then overwrites them in place)
        fc2.res_ln_stats = r.lnst;
        fc2.res_ln_g = (const float*)Lw.ln1g.p;
        fc2.res_ln_b = (const float*)Lw.ln1b.p;
    } else {  // x1 = LN1(y): both the fc1 operand and the FFN residual
        // (ln1_inplace: LayerNorm 1 overwrites its input — a wave reads its whole row before it writes — and fc2 then adds its
        //  product onto that buffer in place: every element is read and written by the same lane)
        float* x1 = r.ln1_inplace ? r.tmp1 : r.tmp2;
        HIP_TRY(ln("layernorm:ln1", 8 + (f32 ? 0 : es), r.tmp1, Lw.ln1g, Lw.ln1b, x1, f32 ? nullptr : r.xT, LnAcc(), LnGate(), nullptr));
        fc2.residual = x1;
        if (f32) ffn_in = x1;
    }
    if (r.stop_after == 33) return LAYER_STOPPED;  // (behind LayerNorm 1 / 2)
    {   // fc1 + bias + GELU
        Linear q{"gemm:fc1", ffn_in, Lw.w1.p, Lw.b1.p, M, F, D, 1};
        q.W_x3 = Lw.w13.p;
        if (f32) q.out32 = (float*)r.hbuf; else q.out16 = r.hbuf;
        if (linear(e, st, q)) return LAYER_FAILED;
    }
    if (r.stop_after == 34) return LAYER_STOPPED;  // (behind fc1)
    // fc2 + bias + residual.  pre-LN: the result IS the residual stream after the layer; post-LN: it feeds final_layer_norm
    float* fc2_dst = prel ? r.x_next : r.tmp1;
    if (ffn_tap) {
        // the GEMM exports fc2(x) + bias, the residual is re-applied by an elementwise add in the same order as the fused
        // epilogue (bit-identical stream)
        const float* ffn_res = fc2.residual;
        fc2.residual = nullptr;
        fc2.out32 = r.ffn_out32;
        fc2.out16 = r.ffn_out16;
        if (linear(e, st, fc2)) return LAYER_FAILED;
        if (r.ffn_exported && r.ffn_exported()) return LAYER_FAILED;
        Prof pr(e, st, "residual_add", 0, gM * D * 12);
        HIP_TRY(launch_add(r.ffn_out32, ffn_res, fc2_dst, M * D, st));
    } else {
        fc2.out32 = fc2_dst;
        fc2.out16 = prel ? r.x16_next : nullptr;
        if (linear(e, st, fc2)) return LAYER_FAILED;
    }
    if (!prel)
        HIP_TRY(ln("layernorm:ln2", 8 + (f32 ? 0 : es), r.tmp1, Lw.ln2g, Lw.ln2b, r.x_next, r.x16_next, r.acc_out, r.gate_next, nullptr));
    return LAYER_DONE;
}

}  // namespace s3e
