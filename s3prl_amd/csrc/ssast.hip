// ssast.hip — SSAST (upstream/ssast/{expert,ast_models,audio}.py; ssast_frame_base, ssast_patch_base), exact fp32: every utterance cut
// into fixed windows, per window a hanning kaldi log-mel front end at 128 bins with an affine normalisation, a Conv2d patch embedding
// with overlapping patches behind a cls and a dist token, the checkpoint's position rows, and encoder_layers pre-LN timm blocks with no
// mask anywhere.
//
// Schedule (all on the caller's stream, no host synchronisation):
//   windows     nseg = ceil(n_max / W) windows per utterance; the padded PCM is staged once as (B * nseg) rows of W samples: one
//               memset, one copy per utterance (window (b, s) is row b * nseg + s);
//   front end   launch_fbank_windows (fbank.hip): ONE overlapping-row GEMM over all windows and one mel pass whose epilogue is
//               (y + 4.2677393) / (4.5689974 * 2) as the reference's two fp32 operations, F_w rows per window into a zero-filled (B *
//               nseg, target_length, 128) image — the trailing rows stay exact zeros;
//   then, per chunk of whole windows (tuning key ssast_chunk: tokens per pass; the workspace does not grow with B * nseg):
//   embedding   launch_patch_strided (patchstrided.hip): conv + bias + position row at the sequence pitch, the two prefix rows
//               written into every sequence; tuning key patch_strided_fused = 0: gather + tile GEMM + position add;
//   layers      encoder_layer (transformer.hip) pre-LN at the block's own LayerNorm eps (LayerRun::ln_eps), q pre-scaled by 1 / 8,
//               valid = all tokens for every sequence;
//   emit        after each layer rows 2 .. of window (b, s) go to state rows s * t_dim .. of utterance b, cut at T_out: the tokens are
//               time-major inside the handle, so every f_dim-row group of a sequence already is one state row of f_dim * D floats
//               and the emit is a copy (or the Featurizer's multiply-add) of whole rows: 2 * 4 * M * D bytes per layer.
// States: encoder_layers layer outputs of (B, T_out, f_dim * D), T_out = min(nseg * t_dim, ceil(n_max / (160 * tstride))).  v.norm
// reaches no returned state and is not computed.  Rows behind an utterance's own length are the reference's values.
#include "engine_internal.h"

namespace s3e {

namespace {
s3::FbankParams ssast_fbank_params() {  // audio.py:88-99: kaldi.fbank's defaults, 128 bins, window_type = "hanning", no dither
    s3::FbankParams f;
    f.sample_rate = 16000;
    f.num_mel_bins = 128;
    f.frame_length_ms = 25.f;
    f.frame_shift_ms = 10.f;
    f.preemph = 0.97f;
    f.delta_order = 0;
    f.delta_win = 5;
    f.use_cmvn = 0;
    f.window = 2;
    return f;
}
constexpr float kNormAdd = 4.2677393f;                     // audio.py:101
const float kNormDiv = (float)(4.5689974 * 2);             // the rounded double product, as torch divides by a Python scalar

struct Geo {
    int f_dim, t_dim, tokens;  // patch tokens per window: f_dim * t_dim (+ 2 prefix rows per sequence)
    long Fw;                   // the window's own frames
};
Geo geo_of(const s3enc_ssast_config& x) {
    Geo g;
    g.f_dim = (128 - x.fshape) / x.fstride + 1;
    g.t_dim = (x.target_length - x.tshape) / x.tstride + 1;
    g.tokens = g.f_dim * g.t_dim;
    g.Fw = 1 + (x.window_samples - 400) / 160;
    return g;
}
long ceil_div(long a, long b) { return (a + b - 1) / b; }
long t_out(const s3enc_ssast_config& x, long n_max) {
    if (n_max <= 0) return 0;
    const Geo g = geo_of(x);
    return std::min(ceil_div(n_max, x.window_samples) * g.t_dim, ceil_div(n_max, 160L * x.tstride));
}

// rows [0, nrows[w]) x width of every window's sequence (behind its two prefix rows) -> the window's place in the state:
// mode 0: dst = src; 1: dst = wgt * src; 2: dst += wgt * src.  One thread per 16-byte piece; grid.y = window of the chunk.
struct EmitParams {
    const float* src;
    long src_ws;   // floats between two windows' first patch rows: (2 + tokens) * D
    float* dst;
    int w0, nseg, t_dim;
    long T_out, width;  // state rows per utterance, floats per state row
    int mode;
    float wgt;
};
__global__ __launch_bounds__(256) void ssast_emit_kernel(EmitParams p) {
    const int w = p.w0 + blockIdx.y;  // window (b, s) = b * nseg + s
    const int b = w / p.nseg, s = w - b * p.nseg;
    long rows = p.T_out - (long)s * p.t_dim;
    rows = rows < 0 ? 0 : (rows > p.t_dim ? p.t_dim : rows);
    const long n4 = rows * p.width / 4;
    const float4* src = (const float4*)(p.src + (long)blockIdx.y * p.src_ws);
    float4* dst = (float4*)(p.dst + ((long)b * p.T_out + (long)s * p.t_dim) * p.width);
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
        float4 v = src[i];
        if (p.mode) {
            v.x *= p.wgt; v.y *= p.wgt; v.z *= p.wgt; v.w *= p.wgt;
            if (p.mode == 2) {
                const float4 a = dst[i];
                v.x += a.x; v.y += a.y; v.z += a.z; v.w += a.w;
            }
        }
        dst[i] = v;
    }
}
}  // namespace

static int ssast_check_config(const s3enc_config& c, const s3enc_ssast_config& x) {
    static const char* dt[] = {"fp32", "bf16", "fp16", "fp32x3", "fp16x2"};
    if (c.compute_dtype < 0 || c.compute_dtype > 4) return fail("config: unknown compute_dtype");
    if (c.compute_dtype != S3ENC_F32)
        return fail(std::string("config: SSAST is built for compute dtype fp32 only; ") + dt[c.compute_dtype] + " is not built");
    if (!c.layer_norm_first) return fail("config: ssast blocks are pre-LN (layer_norm_first must be 1)");
    if (c.heads < 1 || c.embed_dim != c.heads * 64)
        return fail("config: ssast embed_dim / heads must be 64 (the attention kernel's head width)");
    if (c.embed_dim > 2048) return fail("config: ssast embed_dim above 2048 (the eps-taking LayerNorm's row width)");
    if (c.encoder_layers < 1 || c.encoder_layers > 64) return fail("config: ssast encoder_layers out of range");
    if (c.ffn_dim < 4 || (c.ffn_dim & 3)) return fail("config: ssast ffn_dim must be a multiple of 4");
    if (x.window_samples < 400 || (x.window_samples & 3) || x.window_samples > (1 << 24))
        return fail("config: ssast window_samples must be a multiple of 4, at least one 400-sample analysis window, got " +
                    std::to_string(x.window_samples));
    if (x.target_length < 1 || x.target_length > (1 << 16)) return fail("config: ssast target_length out of range");
    if (1 + (x.window_samples - 400) / 160 > x.target_length)
        return fail("config: ssast target_length is below the window's own frame count (the reference would cut the frames)");
    if (!(x.ln_eps > 0.f) || !(x.ln_eps < 1.f)) return fail("config: ssast ln_eps must be in (0, 1)");
    PatchStridedParams p{};
    p.rows = x.target_length;
    p.fshape = x.fshape;
    p.tshape = x.tshape;
    p.fstride = x.fstride;
    p.tstride = x.tstride;
    p.N = c.embed_dim;
    p.nwin = 1;
    p.img_bs = (long)x.target_length * 128;
    alignas(16) static float stand_in[4];
    p.img = p.W = stand_in;
    p.out = stand_in;
    patch_strided_geometry(p);
    if (const char* why = patch_strided_refusal(p)) return fail(std::string("config: ssast patch geometry: ") + why);
    if (x.pos_rows != p.f_dim * p.t_dim)
        return fail("config: ssast pos_rows must be f_dim * t_dim = " + std::to_string(p.f_dim * p.t_dim) + ", got " + std::to_string(x.pos_rows));
    if (p.f_dim * p.t_dim + 2 > 8192) return fail("config: ssast windows of more than 8192 tokens are not built");
    return 0;
}

static int ssast_create(s3enc_encoder* e, const Ckpt& ck) {
    const s3enc_ssast_config& x = e->ssast_cfg;
    const s3enc_config& c = e->cfg;
    const int D = c.embed_dim, K = x.tshape * x.fshape;
    e->ssast.reset(new SsastW());
    SsastW& w = *e->ssast;
    std::vector<float> t;
    GET("patch.weight", (long)D * K, t);
    UP(upload_f32(w.pw, t));
    GET("patch.bias", D, t);
    UP(upload_f32(w.pb, t));
    GET("prefix", 2L * D, t);
    UP(upload_f32(w.prefix, t));
    GET("pos", (long)x.pos_rows * D, t);
    UP(upload_f32(w.pos, t));
    w.layers.resize(c.encoder_layers);
    for (int l = 0; l < c.encoder_layers; ++l)  // head_dim^-0.5 = 1 / sqrt(64): exact
        if (load_layer(e, ck, "blocks." + std::to_string(l) + ".", kTimmLayer, 0.125f, false, w.layers[l])) return 1;
    return 0;
}

static int ssast_forward(s3enc_handle e, const float* const* wav_ptrs_host, const int64_t* lengths, int32_t B, int64_t n_max_in,
                         const FwdOpts& fo, void* out, int64_t layer_stride, hipStream_t st) {
    const s3enc_ssast_config& x = e->ssast_cfg;
    const s3enc_config& c = e->cfg;
    SsastW& w = *e->ssast;
    const int D = c.embed_dim, FF = c.ffn_dim, NL = c.encoder_layers;
    const Geo g = geo_of(x);
    if (fo.selection != S3ENC_SEL_HIDDEN)
        return fail("s3enc_forward: feature_selection is not defined for SSAST (the reference expert has one hidden_states list)");
    if (fo.featurize && !fo.w) return fail("s3enc_forward: featurize needs feat_w");
    if (fo.featurize && fo.feat_norm) return fail("s3enc_forward: feat_normalize is not built for an SSAST handle");
    if (!fo.featurize && fo.out_dtype != F32) return fail("s3enc_forward: out_dtype must be S3ENC_F32 for an SSAST handle");
    if (e->aux_codewords || e->aux_codeids) return fail("s3enc_forward_aux: codewords / codeids are outputs of a wav2vec handle with a vector quantizer");
    if (B > 65535) return fail("s3enc_forward: batch too large");
    long n_max;
    if (batch_n_max(wav_ptrs_host, lengths, B, n_max_in, n_max)) return 1;
    if (n_max < 1) return fail("s3enc_forward: the batch is empty (n_max < 1)");
    const long W = x.window_samples, TL = x.target_length;
    const long nseg = ceil_div(n_max, W), NW = (long)B * nseg, T_out = t_out(x, n_max);
    const long width = (long)g.f_dim * D, seq = g.tokens + 2;
    if (NW > 0x7fffffffL / 4 || NW * seq > 0x7fffffffL / 4 || NW * W > (1L << 40)) return fail("s3enc_forward: batch too large");
    if (check_out(out, fo, layer_stride, (long)B * T_out * width)) return 1;
    DeviceGuard dg(e->device);
    if (!dg.ok) return fail("s3enc_forward: hipSetDevice failed");

    // ---- windows per pass: whole windows, at least one ----
    const long CW = std::max(1L, std::min({NW, (long)tuning().ssast_chunk / seq, 16384L}));
    const long Mc = CW * seq;  // rows of a full chunk

    // ---- small device state: every sequence's key count (all of its tokens) ----
    const size_t tbl_bytes = ((size_t)CW * 4 + 15) & ~(size_t)15;
    HIP_TRY(e->small.ensure_on_stream(tbl_bytes + 1024, st));
    char* dsm = (char*)e->small.p;
    char* hp;
    if (stage_begin(e, tbl_bytes, st, hp)) return 1;
    for (long i = 0; i < CW; ++i) ((int*)hp)[i] = (int)seq;
    if (stage_commit(e, hp, dsm, tbl_bytes, st)) return 1;
    const int* d_valid = (const int*)dsm;

    // ---- workspace ----
    const bool fused = tuning().patch_strided_fused != 0;
    const s3::FbankParams fp = ssast_fbank_params();
    const size_t spec_bytes = fbank_batch_workspace(fp, (int)NW, g.Fw, 0);
    PatchStridedParams pe{};
    pe.img_bs = TL * 128;
    pe.W = (const float*)w.pw.p;
    pe.bias = (const float*)w.pb.p;
    pe.pos = (const float*)w.pos.p;
    pe.prefix = (const float*)w.prefix.p;
    pe.nwin = (int)CW;
    pe.rows = (int)TL;
    pe.fshape = x.fshape;
    pe.tshape = x.tshape;
    pe.fstride = x.fstride;
    pe.tstride = x.tstride;
    pe.N = D;
    patch_strided_geometry(pe);
    float *pcm, *img, *spec, *xa, *xb, *tmp, *xn, *qkv, *ctx, *hbuf, *rows = nullptr;
    for (int pass = 0; pass < 2; ++pass) {
        Bump wb(pass ? e->ws.p : nullptr);
        pcm = (float*)wb.take((size_t)NW * W * 4);
        img = (float*)wb.take((size_t)NW * TL * 128 * 4);
        spec = (float*)wb.take(spec_bytes);
        xa = (float*)wb.take((size_t)Mc * D * 4);
        xb = (float*)wb.take((size_t)Mc * D * 4);
        tmp = (float*)wb.take((size_t)Mc * D * 4);
        xn = (float*)wb.take((size_t)Mc * D * 4);
        qkv = (float*)wb.take((size_t)Mc * 3 * D * 4);
        ctx = (float*)wb.take((size_t)Mc * D * 4);
        hbuf = (float*)wb.take((size_t)Mc * FF * 4);
        if (!fused) rows = (float*)wb.take(patch_strided_rows_elems(pe) * 4);
        if (!pass) HIP_TRY(e->ws.ensure_on_stream(wb.off + 4096, st));
    }
    e->taps.clear();

    // ---- where the states go ----
    const bool feat_sum = fo.featurize;
    Sink sink{e, st, feat_sum ? 2 : 0, out, (long)layer_stride, F32, (long)B * T_out, (int)width, fo.w, 0};
    HIP_TRY(sink.zero_without_terms(NL, (long)B * T_out));
    int first_term = -1;  // the Featurizer sum's first non-zero term writes, the later ones add
    for (int l = 0; feat_sum && l < NL && first_term < 0; ++l)
        if (fo.w[l] != 0.f) first_term = l;

    // ---- the windows: (B * nseg, W) zero-padded PCM ----
    {
        Prof pr(e, st, "ssast_windows", 0, 4.0 * ((double)NW * W + (double)B * n_max));
        HIP_TRY(hipMemsetAsync(pcm, 0, (size_t)NW * W * 4, st));
        for (int b = 0; b < B; ++b)
            if (lengths[b] > 0)
                HIP_TRY(hipMemcpyAsync(pcm + (size_t)b * nseg * W, wav_ptrs_host[b], (size_t)lengths[b] * 4, hipMemcpyDeviceToDevice, st));
    }
    // ---- front end: (B * nseg, target_length, 128), exact zeros behind every window's own F_w frames ----
    {
        Prof pr(e, st, "ssast_fbank", 2.0 * NW * g.Fw * 514.0 * 400.0, 4.0 * ((double)NW * W + (double)NW * TL * 128));
        HIP_TRY(hipMemsetAsync(img, 0, (size_t)NW * TL * 128 * 4, st));
        HIP_TRY(s3::launch_fbank_windows(fp, pcm, W, (int)NW, g.Fw, kNormAdd, kNormDiv, img, TL * 128, 128, spec, spec_bytes, 0, st));
    }

    LayerRun run{(int)CW, seq, d_valid, true};
    run.ln_eps = x.ln_eps;
    run.xT = xn;
    run.qkv = qkv;
    run.attn = ctx;
    run.hbuf = hbuf;
    run.tmp1 = tmp;
    run.tmp2 = xn;
    const int Kp = x.tshape * x.fshape;
    for (long w0 = 0; w0 < NW; w0 += CW) {
        const long nw = std::min(CW, NW - w0), M = nw * seq;
        // ---- patch embedding + position rows + the two prefix rows ----
        pe.img = img + (size_t)w0 * TL * 128;
        pe.nwin = (int)nw;
        pe.out = xa;
        if (fused) {
            Prof pr(e, st, "patch_strided", 2.0 * nw * g.tokens * D * Kp, 4.0 * ((double)nw * TL * 128 + (double)D * Kp + 2.0 * M * D));
            HIP_TRY(launch_patch_strided(pe, st));
        } else {
            Prof pr(e, st, "patch_strided_two_step", 2.0 * nw * g.tokens * D * Kp,
                    4.0 * (3.0 * nw * g.tokens * Kp + (double)D * Kp + 4.0 * M * D));
            HIP_TRY(launch_patch_strided_two_step(pe, rows, st));
        }
        // ---- the blocks over nw sequences of 2 + tokens rows; x_cur is the layer's input ----
        float* x_cur = xa;
        run.B = (int)nw;
        for (int l = 0; l < NL; ++l) {
            float* x_next = x_cur == xa ? xb : xa;
            run.x = x_cur;
            run.x_next = x_next;
            if (encoder_layer(e, st, w.layers[l], run)) return 1;
            if (sink.wanted(l)) {
                Prof pr(e, st, "ssast_emit", 0, 8.0 * nw * g.tokens * D);
                EmitParams ep{};
                ep.src = x_next + 2L * D;
                ep.src_ws = seq * D;
                ep.dst = feat_sum ? (float*)out : sink.slot32(l);
                ep.w0 = (int)w0;
                ep.nseg = (int)nseg;
                ep.t_dim = g.t_dim;
                ep.T_out = T_out;
                ep.width = width;
                ep.mode = feat_sum ? (l == first_term ? 1 : 2) : 0;
                ep.wgt = feat_sum ? fo.w[l] : 1.f;
                const long n4 = (long)g.t_dim * width / 4;
                const unsigned gx = (unsigned)std::min<long>((n4 + 255) / 256, 1024);
                hipLaunchKernelGGL(ssast_emit_kernel, dim3(gx, (unsigned)nw), dim3(256), 0, st, ep);
                HIP_TRY(hipGetLastError());
            }
            x_cur = x_next;
        }
    }
    for (int l = 0; l < NL; ++l) HIP_TRY(sink.done(l));  // (a state is whole once the last chunk has passed)
    return 0;
}

// frames: T_out of a batch padded to n; valid: the wrapper's rule at rate 160 * tstride, clamped to the batch's rows; rate:
// ssast/expert.py:82-83; states: the blocks' outputs (ast_models.py:381-393)
FamilyOps kSsastFamily = {
    S3ENC_SSAST, "ssast", "S3ENC_SSAST", "s3enc_create_ssast", "the SSAST family needs its window / patch block",
    "SSAST (one hidden_states list)",
    [](const s3enc_config& c, const void* b) { return ssast_check_config(c, *(const s3enc_ssast_config*)b); },
    [](s3enc_encoder* e, const Ckpt& ck, const void* b) { e->ssast_cfg = *(const s3enc_ssast_config*)b; return ssast_create(e, ck); },
    ssast_forward,
    [](const s3enc_encoder* h, long n) { return t_out(h->ssast_cfg, n); },
    [](const s3enc_encoder* h, long length, long n_max) {
        return (int)std::max(0L, std::min(ceil_div(std::max(length, 0L), 160L * h->ssast_cfg.tstride), t_out(h->ssast_cfg, n_max)));
    },
    [](const s3enc_encoder* h) { return h->ssast_cfg.tstride * 160; },
    [](const s3enc_encoder* h) { return h->cfg.encoder_layers; }};

}  // namespace s3e
