// mae_ast.hip — MAE-AST (upstream/mae_ast/{expert,mae_ast}.py; mae_ast_frame, mae_ast_patch), exact fp32: a kaldi log-mel front end
// at 128 bins, the eval BatchNorm2d(1) times 0.5, nn.Unfold into kt x kc patches, Linear(kt * kc, D), the checkpoint's sinusoidal
// position rows on the live tokens, and encoder_layers Transformer layers with the padded tokens masked as keys.
//
// Schedule (all on the caller's stream, no host synchronisation):
//   front end   launch_fbank per utterance (fbank.hip, its bits unchanged) into a zero-filled (B, F_max, 128) image;
//   embedding   launch_patch_embed (patchembed.hip): unfold + Linear + position row in one implicit GEMM that reads the image in
//               place.  The BatchNorm is folded into the Linear at create time (W' = s W, b' = b - s mean rowsum(W), s = 0.5 /
//               sqrt(var + eps), float64), so the image stays raw log-mel and the rows behind an utterance's frames stay the memset;
//               tuning key patch_embed_fused = 0: gather + tile GEMM + position add;
//   layers      post-LN (layer_norm_first = 0): encoder.layer_norm, then per layer q|k|v GEMM (q and its bias pre-scaled by 1 / 8:
//               a power of two), launch_attention over B sequences of Ttok tokens with valid = kv, out-proj GEMM + residual,
//               LayerNorm, fc1 GEMM + GELU, fc2 GEMM + residual, LayerNorm — the state.  Pre-LN (layer_norm_first = 1): LayerNorm,
//               q|k|v, attention, out-proj + residual, LayerNorm, fc1 + GELU, fc2 + residual — the state; the encoder's final
//               LayerNorm reaches none of the returned states (mae_ast.py:652-688) and is not computed.
// States: the encoder_layers layer outputs, (B, Ttok, D) — the same bytes as the expert's (B, Tt, V * D) reshape.  Where the
// caller asks for an fp32 slab the producing kernel writes the state's slot and the next layer reads it there.
// Padding (forward_padding_mask, mae_ast.py:305-325): utterance b keeps kv_b = min(ceil(F_b / kt) * V, Ttok) leading tokens as keys.
// Tokens at or behind kv_b are the reference's values: zero image rows through the folded Linear (= BatchNorm'd zeros through the
// Linear), no position row (SinusoidalPositionalEncoding zeroes them), queries over the live keys, never keys.
#include "engine_internal.h"

namespace s3e {

namespace {
s3::FbankParams mae_fbank_params() {  // torchaudio.compliance.kaldi.fbank's defaults with num_mel_bins = 128 (expert.py:60-66)
    s3::FbankParams f;
    f.sample_rate = 16000;
    f.num_mel_bins = 128;
    f.frame_length_ms = 25.f;
    f.frame_shift_ms = 10.f;
    f.preemph = 0.97f;
    f.delta_order = 0;
    f.delta_win = 5;
    f.use_cmvn = 0;
    f.window = 0;
    return f;
}
long mae_frames(long n) { return n < 400 ? 0 : 1 + (n - 400) / 160; }
}  // namespace

static long mae_ast_num_steps(const s3enc_mae_ast_config& x, long n_samples) { return mae_frames(n_samples) / x.kt; }

// min(ceil(F(length) / kt), F(n_max) / kt)
static long mae_ast_valid_steps(const s3enc_mae_ast_config& x, long length, long n_max) {
    const long Tt = mae_frames(n_max) / x.kt, v = (mae_frames(length) + x.kt - 1) / x.kt;
    return std::max(0L, std::min(v, Tt));
}

static int mae_ast_check_config(const s3enc_config& c, const s3enc_mae_ast_config& x) {
    static const char* dt[] = {"fp32", "bf16", "fp16", "fp32x3", "fp16x2"};
    if (c.compute_dtype < 0 || c.compute_dtype > 4) return fail("config: unknown compute_dtype");
    if (c.compute_dtype != S3ENC_F32)
        return fail(std::string("config: MAE-AST is built for compute dtype fp32 only; ") + dt[c.compute_dtype] + " is not built");
    if (x.feature_dim != 128)
        return fail("config: mae_ast feature_dim must be 128 (the reference's padding-mask rule hard-codes 128 mel bins), got " +
                    std::to_string(x.feature_dim));
    if (x.kc != 16 && x.kc != 32 && x.kc != 64 && x.kc != 128)
        return fail("config: mae_ast ast_kernel_size_chan must be 16, 32, 64 or 128 (the patch kernel's set), got " + std::to_string(x.kc));
    if (x.kt < 1 || x.kt > 32) return fail("config: mae_ast ast_kernel_size_time must be 1..32 (the patch kernel's set), got " + std::to_string(x.kt));
    if (c.heads < 1 || c.embed_dim != c.heads * 64)
        return fail("config: mae_ast encoder_embed_dim / encoder_attention_heads must be 64 (the attention kernel's head width)");
    if (c.encoder_layers < 1 || c.encoder_layers > 64) return fail("config: mae_ast encoder_layers out of range");
    if (c.ffn_dim < 4 || (c.ffn_dim & 3)) return fail("config: mae_ast encoder_ffn_embed_dim must be a multiple of 4");
    if (!(x.bn_eps > 0.f) || !(x.bn_var >= 0.f) || !std::isfinite(x.bn_mean) || !std::isfinite(x.bn_var))
        return fail("config: mae_ast BatchNorm statistics out of range");
    if (x.pos_rows < 1 || x.pos_rows > 8192) return fail("config: mae_ast pos_rows must be 1..8192");
    return 0;
}

static int mae_ast_create(s3enc_encoder* e, const Ckpt& ck) {
    const s3enc_mae_ast_config& x = e->mae_ast_cfg;
    const s3enc_config& c = e->cfg;
    const int D = c.embed_dim, FF = c.ffn_dim, K = x.kt * x.kc;
    e->mae_ast.reset(new MaeAstW());
    MaeAstW& w = *e->mae_ast;
    std::vector<float> t, t2;
    {   // the eval BatchNorm (affine = False) times 0.5, folded into the Linear in float64
        GET("post_extract_proj.weight", (long)D * K, t);
        GET("post_extract_proj.bias", D, t2);
        const double s = 0.5 / std::sqrt((double)x.bn_var + (double)x.bn_eps);
        for (int n = 0; n < D; ++n) {
            double rs = 0.0;
            for (int k = 0; k < K; ++k) rs += (double)t[(size_t)n * K + k];
            t2[n] = (float)((double)t2[n] - s * (double)x.bn_mean * rs);
            for (int k = 0; k < K; ++k) t[(size_t)n * K + k] = (float)(s * (double)t[(size_t)n * K + k]);
        }
        UP(upload_f32(w.pw, t));
        UP(upload_f32(w.pb, t2));
    }
    GET("enc_sine_pos_embed.pe", (long)x.pos_rows * D, t);  // the leading rows of the file's own table
    UP(upload_f32(w.pos, t));
    if (!c.layer_norm_first) {
        GET("encoder.layer_norm.weight", D, t);
        UP(upload_f32(w.eln_g, t));
        GET("encoder.layer_norm.bias", D, t);
        UP(upload_f32(w.eln_b, t));
    }
    w.layers.resize(c.encoder_layers);
    for (int l = 0; l < c.encoder_layers; ++l)  // head_dim^-0.5 = 1 / sqrt(64): exact
        if (load_layer(e, ck, "encoder.layers." + std::to_string(l) + ".", kFairseqLayer, 0.125f, false, w.layers[l])) return 1;
    return 0;
}

static int mae_ast_forward(s3enc_handle e, const float* const* wav_ptrs_host, const int64_t* lengths, int32_t B, int64_t n_max_in,
                    const FwdOpts& fo, void* out, int64_t layer_stride, hipStream_t st) {
    const s3enc_mae_ast_config& x = e->mae_ast_cfg;
    const s3enc_config& c = e->cfg;
    MaeAstW& w = *e->mae_ast;
    const int D = c.embed_dim, FF = c.ffn_dim, NL = c.encoder_layers, H = c.heads, kt = x.kt, kc = x.kc, V = 128 / kc;
    const bool prel = c.layer_norm_first != 0;
    if (fo.selection != S3ENC_SEL_HIDDEN)
        return fail("s3enc_forward: feature_selection is not defined for MAE-AST (the reference expert has one hidden_states list)");
    if (fo.featurize && !fo.w) return fail("s3enc_forward: featurize needs feat_w");
    if (fo.featurize && fo.feat_norm && V > 1)
        return fail("s3enc_forward: feat_normalize is not built for an MAE-AST handle with more than one token per state row (the "
                    "reference normalises rows of V * D)");
    if (!fo.featurize && fo.out_dtype != F32) return fail("s3enc_forward: out_dtype must be S3ENC_F32 for an MAE-AST handle");
    if (e->aux_codewords || e->aux_codeids) return fail("s3enc_forward_aux: codewords / codeids are outputs of a wav2vec handle with a vector quantizer");
    if (B > 65535) return fail("s3enc_forward: batch too large");
    long n_max;
    if (batch_n_max(wav_ptrs_host, lengths, B, n_max_in, n_max)) return 1;
    for (int b = 0; b < B; ++b)
        if (lengths[b] < 400)
            return fail("s3enc_forward: utterance " + std::to_string(b) + " has " + std::to_string((long)lengths[b]) +
                        " samples, fewer than one 400-sample analysis window of the MAE-AST front end");
    const long Fmax = mae_frames(n_max);
    const long Tt = Fmax / kt, Ttok = Tt * V;
    if (Tt < 1)
        return fail("s3enc_forward: the batch has " + std::to_string(Fmax) + " frames, fewer than one patch of " + std::to_string(kt) +
                    " frames (F_max < kt)");
    if (Ttok > x.pos_rows)
        return fail("s3enc_forward: the batch needs " + std::to_string(Ttok) + " position rows, the handle holds " +
                    std::to_string(x.pos_rows) + " (the leading rows of the checkpoint's enc_sine_pos_embed.pe)");
    // the expert's cut to len(range(0, max_len, kt * 160)) rows never binds for utterances of at least 400 samples
    if (Tt > (n_max + (long)kt * 160 - 1) / ((long)kt * 160)) return fail("s3enc_forward: more time steps than the expert's cut keeps (internal)");
    const long M = (long)B * Ttok;
    if (M > 0x7fffffffL / 4) return fail("s3enc_forward: batch too large");
    if (check_out(out, fo, layer_stride, M * D)) return 1;
    DeviceGuard dg(e->device);
    if (!dg.ok) return fail("s3enc_forward: hipSetDevice failed");

    // ---- small device state: per-utterance key counts ----
    const size_t tbl_bytes = ((size_t)B * 4 + 15) & ~(size_t)15;
    HIP_TRY(e->small.ensure_on_stream(tbl_bytes + 1024, st));
    char* dsm = (char*)e->small.p;
    char* hp;
    if (stage_begin(e, tbl_bytes, st, hp)) return 1;
    for (int b = 0; b < B; ++b) {
        const long Fb = mae_frames((long)lengths[b]);
        ((int*)hp)[b] = (int)std::min(((Fb + kt - 1) / kt) * V, Ttok);  // forward_padding_mask: a partly real patch counts as real
    }
    if (stage_commit(e, hp, dsm, tbl_bytes, st)) return 1;
    const int* d_kv = (const int*)dsm;

    // ---- workspace ----
    const bool feat_sum = fo.featurize;
    const bool fused = tuning().patch_embed_fused != 0;
    PatchEmbedParams pe{};
    pe.img_bs = Fmax * 128;
    pe.W = (const float*)w.pw.p;
    pe.bias = (const float*)w.pb.p;
    pe.pos = (const float*)w.pos.p;
    pe.kv = d_kv;
    pe.B = B;
    pe.Tt = (int)Tt;
    pe.kt = kt;
    pe.kc = kc;
    pe.N = D;
    patch_embed_geometry(pe);
    float *img, *xa, *xb, *tmp, *xn, *qkv, *ctx, *hbuf, *rows = nullptr;
    for (int pass = 0; pass < 2; ++pass) {
        Bump wb(pass ? e->ws.p : nullptr);
        img = (float*)wb.take((size_t)B * Fmax * 128 * 4);
        xa = (float*)wb.take((size_t)M * D * 4);
        xb = (float*)wb.take((size_t)M * D * 4);
        tmp = (float*)wb.take((size_t)M * D * 4);
        xn = (float*)wb.take((size_t)M * D * 4);
        qkv = (float*)wb.take((size_t)M * 3 * D * 4);
        ctx = (float*)wb.take((size_t)M * D * 4);
        hbuf = (float*)wb.take((size_t)M * FF * 4);
        if (!fused) rows = (float*)wb.take(patch_embed_rows_elems(pe) * 4);
        if (!pass) HIP_TRY(e->ws.ensure_on_stream(wb.off + 4096, st));
    }
    pe.img = img;
    e->taps.clear();

    // ---- where the states go ----
    Sink sink{e, st, feat_sum ? 2 : 0, out, (long)layer_stride, F32, M, D, fo.w, fo.feat_norm};
    HIP_TRY(sink.zero_without_terms(NL, M));

    // ---- front end: (B, F_max, 128) raw log-mel, zeros behind every utterance's frames ----
    {
        Prof pr(e, st, "mae_fbank", 0, 4.0 * ((double)B * n_max + (double)B * Fmax * 128));
        HIP_TRY(hipMemsetAsync(img, 0, (size_t)B * Fmax * 128 * 4, st));
        const s3::FbankParams fp = mae_fbank_params();
        for (int b = 0; b < B; ++b) HIP_TRY(s3::launch_fbank(fp, wav_ptrs_host[b], lengths[b], img + (size_t)b * Fmax * 128, 128, st));
    }

    // ---- patch embedding + position rows ----
    const int Kp = kt * kc;
    pe.out = prel ? xa : tmp;
    if (fused) {
        Prof pr(e, st, "patch_embed", 2.0 * M * D * Kp, 4.0 * ((double)M * Kp + (double)D * Kp + 2.0 * M * D));
        HIP_TRY(launch_patch_embed(pe, st));
    } else {
        Prof pr(e, st, "patch_embed_two_step", 2.0 * M * D * Kp, 4.0 * (3.0 * M * Kp + (double)D * Kp + 4.0 * M * D));
        HIP_TRY(launch_patch_embed_two_step(pe, rows, st));
    }
    if (!prel) {
        Prof pr(e, st, "layernorm:enc", 0, 4.0 * M * D * 2);
        HIP_TRY(launch_layernorm(F32, tmp, (const float*)w.eln_g.p, (const float*)w.eln_b.p, M, D, 0, xa, nullptr, st));
    }

    // ---- Transformer layers over B sequences of Ttok tokens; x_cur is the layer's input ----
    float* x_cur = xa;
    LayerRun run{B, Ttok, d_kv, prel};
    run.xT = xn;
    run.qkv = qkv;
    run.attn = ctx;
    run.hbuf = hbuf;
    run.tmp1 = tmp;
    run.tmp2 = xn;
    for (int l = 0; l < NL; ++l) {
        // the state's home: its slot of the caller's slab (the next layer reads it there), or the buffer x_cur does not occupy
        float* x_next = sink.slot32(l) ? sink.slot32(l) : (x_cur == xa ? xb : xa);
        run.x = x_cur;
        run.x_next = x_next;
        run.acc_out = prel ? LnAcc() : sink.acc(l, 2);
        if (encoder_layer(e, st, w.layers[l], run)) return 1;
        if (prel && sink.term(l)) {
            Prof pr(e, st, "emit_state", 0, 4.0 * M * D * 2);
            HIP_TRY(sink.emit(l, x_next));
        }
        HIP_TRY(sink.done(l));
        x_cur = x_next;
    }
    return 0;
}


// frames: time steps of kt frames (a state row is the V tokens of one step); valid: forward_padding_mask, a step that is only partly
// real counts as real; rate: mae_ast/expert.py:57-58; states: the layer outputs, the embedding is not among them (mae_ast.py:671-677)
FamilyOps kMaeAstFamily = {
    S3ENC_MAE_AST, "mae_ast", "S3ENC_MAE_AST", "s3enc_create_mae_ast", "the MAE-AST family needs its patch / BatchNorm block",
    "MAE-AST (one hidden_states list)",
    [](const s3enc_config& c, const void* b) { return mae_ast_check_config(c, *(const s3enc_mae_ast_config*)b); },
    [](s3enc_encoder* e, const Ckpt& ck, const void* b) { e->mae_ast_cfg = *(const s3enc_mae_ast_config*)b; return mae_ast_create(e, ck); },
    mae_ast_forward,
    [](const s3enc_encoder* h, long n) { return mae_ast_num_steps(h->mae_ast_cfg, n); },
    [](const s3enc_encoder* h, long length, long n_max) { return (int)mae_ast_valid_steps(h->mae_ast_cfg, length, n_max); },
    [](const s3enc_encoder* h) { return h->mae_ast_cfg.kt * 160; },
    [](const s3enc_encoder* h) { return h->cfg.encoder_layers; }};

}  // namespace s3e
