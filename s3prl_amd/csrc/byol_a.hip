// byol_a.hip — BYOL-A (upstream/byol_a/expert.py:27-125, byol_a.py:36-137), exact fp32: every utterance of the batch cut into
// segments of `window` samples every `stride` samples, each segment through the log-mel front end of melspec.hip, three Conv2d(3 x 3)
// + BatchNorm2d (eval) + ReLU + MaxPool2d(2, 2) layers, Linear + ReLU + Linear + ReLU per pooled time step, and max + mean over time.
//
// Segments (expert.py:83-97): starts = range(0, n_max, stride), S = len(starts); every utterance is zero-padded to starts[-1] +
// window; segment (b, s) is padded[b][starts[s] : starts[s] + window] and is reflect-padded about ITS OWN ends by the front end.
// The state is (B, S, d) and NOTHING is masked: a row (b, s) behind utterance b's own ceil(len_b / stride) segments is the network's
// response to a segment of zeros (or to the utterance's tail followed by zeros), exactly the reference's value and not a zero row —
// NPC's convention.  A segment's row depends on its own `window` samples only (BatchNorm runs in eval mode).
//
// Schedule (all on the caller's stream, no host synchronisation), segment i = b * S + s:
//   front end: launch_melspec writes (log(mel + eps) - mean) / std as (segment, frame, mel) straight into layer 0's operand, the
//              BORDERED single-channel image (nseg, T + 2, 64 + 2).  The convolutions run on the TRANSPOSED image, H = time and W =
//              mel, with the 3 x 3 taps transposed at pack time;
//   layer 0:   conv2d.hip's C = 1 VALU kernel, layers 1 and 2 its MFMA kernel at the 64-wide n-tile; the BatchNorm is the per-channel
//              affine of the epilogue (scale = gamma / sqrt(var + eps), shift = (conv_bias - mean) * scale + beta, float64 on the
//              host, rounded once — not folded into the weights), then ReLU and the FLOOR 2 x 2 max-pool: 101 x 64 -> 50 x 32 -> 25 x
//              16 -> 12 x 8.  The last map is written with dst_pad = 0 as (nseg, T / 8, 8, 64): that IS fc.0's A operand, the
//              reference's permute(0, 3, 2, 1).reshape flattens mel-major and channel-minor, d * 64 + c (byol_a.py:118-121);
//   fc.0 + launch_relu, fc.3: the fp32 tile GEMM over nseg * (T / 8) rows;
//   byol_a_tail_kernel: out[b, s, :] = max_t relu(y) + mean_t relu(y) — the last ReLU fused, the (rows, d) activation read once.
#include <cmath>

#include "engine_internal.h"

namespace s3e {

namespace {

// one thread per (segment, column): rows [seg * T8, (seg + 1) * T8) of y, time ascending
__global__ __launch_bounds__(256) void byol_a_tail_kernel(const float* y, int T8, int d, long nseg, float* out) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= nseg * d) return;
    const long seg = idx / d;
    const int j = (int)(idx - seg * d);
    const float* p = y + seg * T8 * d + j;
    float mx = 0.f, sum = 0.f;
    for (int t = 0; t < T8; ++t) {
        float v = p[(long)t * d];
        v = v < 0.f ? 0.f : v;  // ReLU; a NaN stays a NaN
        mx = (t == 0 || v > mx || v != v) ? v : mx;
        sum += v;
    }
    out[idx] = mx + sum / (float)T8;
}

const int kConvIdx[3] = {0, 4, 8};  // the Conv2d modules of the reference's nn.Sequential; the BatchNorm2d is the next index

}  // namespace

static long byol_a_num_segments(const s3enc_byol_a_config& x, long n_samples) {
    return n_samples < 1 ? 0 : (n_samples + x.stride - 1) / x.stride;  // len(range(0, n, stride))
}

static int byol_a_check_config(const s3enc_config& c, const s3enc_byol_a_config& x) {
    static const char* dt[] = {"fp32", "bf16", "fp16", "fp32x3", "fp16x2"};
    if (c.compute_dtype < 0 || c.compute_dtype > 4) return fail("config: unknown compute_dtype");
    if (c.compute_dtype != S3ENC_F32)
        return fail(std::string("config: BYOL-A (FFT log-mel segments + 3 x 3 convolutions + BatchNorm + Linears) is built for compute dtype "
                                "fp32 only; ") + dt[c.compute_dtype] + " is not built");
    if (x.feature_d < 4 || (x.feature_d & 3) || x.feature_d > 16384)
        return fail("config: byol_a feature_d must be a multiple of 4, at most 16384 (got " + std::to_string(x.feature_d) + ")");
    if (x.window <= 512)
        return fail("config: byol_a window of " + std::to_string(x.window) + " samples is too short: a segment of at most 512 samples cannot be "
                    "reflect-padded by 512 (n_fft / 2)");
    if (x.window < 1120)
        return fail("config: byol_a window of " + std::to_string(x.window) + " samples is too short: fewer than 8 frames (1120 samples), nothing "
                    "survives three 2 x 2 pools");
    if (x.window > (1 << 22)) return fail("config: byol_a window is too long");
    if (x.stride < 1) return fail("config: byol_a stride must be at least one sample");
    if (!(x.norm_std > 0.f)) return fail("config: byol_a norm_std must be positive");
    if (!(x.bn_eps > 0.f)) return fail("config: byol_a bn_eps must be positive");
    if (c.n_conv != 1 || c.conv_kernel[0] != x.window || c.conv_stride[0] != x.stride)
        return fail("config: byol_a carries its segment geometry as n_conv = 1, conv_kernel[0] / conv_stride[0] = window / stride in samples");
    if (c.conv_dim != x.feature_d || c.embed_dim != x.feature_d || c.encoder_layers != 0)
        return fail("config: byol_a conv_dim / embed_dim must be feature_d and encoder_layers 0 (one state)");
    return 0;
}

hipError_t launch_byol_tail(const float* y, int T8, int d, long nseg, float* out, hipStream_t st) {
    hipLaunchKernelGGL(byol_a_tail_kernel, dim3((unsigned)((nseg * d + 255) / 256)), dim3(256), 0, st, y, T8, d, nseg, out);
    return hipGetLastError();
}

// AudioNTT2020's weights (BYOL-S's `default` network is the same module: byol_s.hip)
int byol_a_load(ByolAW& w, const Ckpt& ck, long feature_d, float bn_eps) {
    std::vector<float> t, tt, packed, bias, g, b, rm, rv;
    int cin = 1;
    for (int i = 0; i < 3; ++i) {
        const std::string cv = "features." + std::to_string(kConvIdx[i]), bn = "features." + std::to_string(kConvIdx[i] + 1);
        GET(cv + ".weight", 64L * cin * 9, t);
        tt.resize(t.size());  // the image is transposed (H = time, W = mel): tap (ky, kx) of the reference is tap (kx, ky) here
        for (long nc = 0; nc < 64L * cin; ++nc)
            for (int ky = 0; ky < 3; ++ky)
                for (int kx = 0; kx < 3; ++kx) tt[nc * 9 + kx * 3 + ky] = t[nc * 9 + ky * 3 + kx];
        s3::pack_conv2d3x3(tt.data(), 64, cin, packed);
        UP(upload_f32(w.cw[i], packed));
        GET(cv + ".bias", 64, bias);
        GET(bn + ".weight", 64, g);
        GET(bn + ".bias", 64, b);
        GET(bn + ".running_mean", 64, rm);
        GET(bn + ".running_var", 64, rv);
        std::vector<float> sc(64), sh(64);
        for (int n = 0; n < 64; ++n) {
            const double var = (double)rv[n] + (double)bn_eps;
            if (!(var > 0.0)) return fail("checkpoint: " + bn + ".running_var[" + std::to_string(n) + "] + eps is not positive");
            const double s = (double)g[n] / std::sqrt(var);
            sc[n] = (float)s;
            sh[n] = (float)(((double)bias[n] - (double)rm[n]) * s + (double)b[n]);
        }
        UP(upload_f32(w.scale[i], sc));
        UP(upload_f32(w.shift[i], sh));
        cin = 64;
    }
    const long d = feature_d;
    GET("fc.0.weight", d * 512, t);
    UP(upload_f32(w.fw[0], t));
    GET("fc.0.bias", d, t);
    UP(upload_f32(w.fb[0], t));
    GET("fc.3.weight", d * d, t);
    UP(upload_f32(w.fw[1], t));
    GET("fc.3.bias", d, t);
    UP(upload_f32(w.fb[1], t));
    return 0;
}

static int byol_a_create(s3enc_encoder* e, const Ckpt& ck) {
    e->byol_a.reset(new ByolAW());
    return byol_a_load(*e->byol_a, ck, e->byol_a_cfg.feature_d, e->byol_a_cfg.bn_eps);
}

// ---- the network behind the front end, on nseg bordered (T + 2) x (64 + 2) images: layer geometry with H = time, W = mel ----
namespace {
struct Geo {
    int H, W, C, Ho, Wo, pad;
    size_t out_elems;
};
void net_geo(long nseg, int T, Geo (&geo)[3]) {
    int H = T, W = 64, C = 1;
    for (int i = 0; i < 3; ++i) {
        Geo& g = geo[i];
        g.H = H;
        g.W = W;
        g.C = C;
        g.Ho = H / 2;
        g.Wo = W / 2;
        g.pad = i == 2 ? 0 : 1;
        g.out_elems = (size_t)nseg * (g.Ho + 2 * g.pad) * (g.Wo + 2 * g.pad) * 64;
        H = g.Ho;
        W = g.Wo;
        C = 64;
    }
}
}  // namespace

int byol_a_net_plan(long nseg, int T, int D, Bump& wb, ByolANet& nb) {
    Geo geo[3];
    net_geo(nseg, T, geo);
    for (int i = 0; i < 3; ++i) {
        if (geo[i].out_elems * 4 >= (1ul << 32) - 64)
            return fail("s3enc_forward: batch too large (" + std::to_string(nseg) + " segments: layer " + std::to_string(i) +
                        "'s activation is not addressable with 32-bit offsets)");
        nb.act[i] = (float*)wb.take(geo[i].out_elems * 4);
    }
    for (int i = 0; i < 2; ++i) nb.fcb[i] = (float*)wb.take((size_t)nseg * (T >> 3) * D * 4);
    return 0;
}

int byol_a_net_run(s3enc_encoder* e, const ByolAW& w, int D, const float* img, long nseg, int T, const ByolANet& nb, float* dst,
                   hipStream_t st) {
    Geo geo[3];
    net_geo(nseg, T, geo);
    const int T8 = T >> 3;
    const long rows = nseg * T8;
    float* const* act = nb.act;
    float* const* fcb = nb.fcb;
    // ---- conv + BatchNorm + ReLU + floor pool, three times ----
    for (int i = 0; i < 3; ++i) {
        const Geo& g = geo[i];
        s3::Conv2dParams q{};
        q.src = i == 0 ? img : act[i - 1];
        q.src_bs = (long)(g.H + 2) * (g.W + 2) * g.C;
        q.C = g.C;
        q.Wt = (const float*)w.cw[i].p;
        q.scale = (const float*)w.scale[i].p;
        q.shift = (const float*)w.shift[i].p;
        q.H = g.H;
        q.W = g.W;
        q.N = 64;
        q.B = (int)nseg;
        q.act = 1;
        q.pool = 1;
        q.pool_floor = 1;
        q.n64 = 1;
        q.dst = act[i];
        q.dst_pad = g.pad;
        q.ld_dst = 64;
        q.dst_bs = (long)(g.Ho + 2 * g.pad) * (g.Wo + 2 * g.pad) * 64;
        if (const char* why = s3::conv2d3x3_refusal(q))
            return fail(std::string("s3enc_forward: the 3 x 3 convolution of layer ") + std::to_string(i) + " refuses: " + why);
        const double px = 4.0 * nseg * g.Ho * g.Wo;
        const std::string kind = i == 0 ? std::string("conv2d3x3:first") : "conv2d3x3:L" + std::to_string(i);
        Prof pr(e, st, kind.c_str(), 2.0 * px * 64 * 9 * g.C,
                4.0 * ((double)nseg * q.src_bs + 9.0 * 64 * g.C + (g.pad ? 2.0 : 1.0) * (double)g.out_elems));
        if (g.pad) HIP_TRY(hipMemsetAsync(act[i], 0, g.out_elems * 4, st));
        HIP_TRY(s3::launch_conv2d3x3(q, st));
    }

    // ---- fc.0 + ReLU, fc.3 (its ReLU is the tail kernel's) ----
    for (int i = 0; i < 2; ++i) {
        const std::string kind = "gemm:byol_a_fc" + std::to_string(i);
        HIP_TRY(linear_f32(e, st, {kind.c_str(), i == 0 ? act[2] : fcb[0], w.fw[i].p, w.fb[i].p, rows, D, i == 0 ? 512 : D, 0, nullptr, fcb[i]}));
        if (i == 0) {
            Prof pr(e, st, "relu", 0, 8.0 * rows * D);
            HIP_TRY(launch_relu(fcb[0], rows * D, st));
        }
    }
    Prof pr(e, st, "byol_a_tail", 2.0 * rows * D, 4.0 * ((double)rows * D + (double)nseg * D));
    HIP_TRY(launch_byol_tail(fcb[1], T8, D, nseg, dst, st));
    return 0;
}

static int byol_a_forward(s3enc_handle e, const float* const* wav_ptrs_host, const int64_t* lengths, int32_t B, int64_t n_max_in,
                   const FwdOpts& fo, void* out, int64_t layer_stride, hipStream_t st) {
    const s3enc_byol_a_config& x = e->byol_a_cfg;
    const ByolAW& w = *e->byol_a;
    const int D = x.feature_d, L = x.window;
    if (fo.selection != S3ENC_SEL_HIDDEN)
        return fail("s3enc_forward: feature_selection is not defined for BYOL-A (the reference expert has one hidden_states list)");
    if (fo.featurize && !fo.w) return fail("s3enc_forward: featurize needs feat_w");
    if (!fo.featurize && fo.out_dtype != F32) return fail("s3enc_forward: out_dtype must be S3ENC_F32 for a BYOL-A handle");
    if (e->aux_codewords || e->aux_codeids) return fail("s3enc_forward_aux: codewords / codeids are outputs of a wav2vec handle with a vector quantizer");
    if (B > 65535) return fail("s3enc_forward: batch too large");
    long n_max;
    if (batch_n_max(wav_ptrs_host, lengths, B, n_max_in, n_max)) return 1;
    const long S = byol_a_num_segments(x, n_max);
    if (S < 1) return fail("s3enc_forward: an empty batch has no BYOL-A segment");
    const long nseg = (long)B * S;
    const int T = (int)s3::melspec_num_frames(L), T8 = T >> 3;
    const long rows = nseg * T8;
    if (nseg > (1L << 20) || rows * std::max(D, 512) > 0x7fffffffL) return fail("s3enc_forward: batch too large");
    for (int b = 0; b < B; ++b) {
        if (((uintptr_t)wav_ptrs_host[b]) & 3) return fail("s3enc_forward: utterance " + std::to_string(b) + " is not 4-byte aligned");
        // stride > window only: the reference pads every utterance to starts[-1] + window and raises when that is shorter than it
        if ((long)lengths[b] > (S - 1) * x.stride + L)
            return fail("s3enc_forward: utterance " + std::to_string(b) + " has " + std::to_string((long)lengths[b]) + " samples, more than the " +
                        std::to_string((S - 1) * x.stride + L) + " the " + std::to_string(S) + " segments of this batch reach (stride " +
                        std::to_string(x.stride) + " > window " + std::to_string(L) + ": the reference's zero padding would be negative and it raises)");
    }
    if (check_out(out, fo, layer_stride, nseg * D)) return 1;
    DeviceGuard dg(e->device);
    if (!dg.ok) return fail("s3enc_forward: hipSetDevice failed");

    const size_t img_elems = (size_t)nseg * (T + 2) * 66;
    const int fft = s3::tuning().melspec_fft;

    // ---- the segment table: first sample and readable samples of segment b * S + s ----
    const size_t ptr_bytes = (size_t)nseg * sizeof(const float*), tbl_bytes = ptr_bytes + (size_t)nseg * sizeof(int);
    HIP_TRY(e->small.ensure_on_stream(tbl_bytes + 1024, st));
    char* hp;
    if (stage_begin(e, tbl_bytes, st, hp)) return 1;
    {
        const float** hptr = (const float**)hp;
        int* hval = (int*)(hp + ptr_bytes);
        for (int b = 0; b < B; ++b)
            for (long s = 0; s < S; ++s) {
                const long start = s * x.stride, left = (long)lengths[b] - start;
                hptr[b * S + s] = left > 0 ? wav_ptrs_host[b] + start : wav_ptrs_host[b];
                hval[b * S + s] = (int)(left > L ? L : (left < 0 ? 0 : left));
            }
    }
    if (stage_commit(e, hp, e->small.p, tbl_bytes, st)) return 1;
    const float* const* d_ptr = (const float* const*)e->small.p;
    const int* d_val = (const int*)((char*)e->small.p + ptr_bytes);

    // ---- workspace ----
    float *img, *post = nullptr, *sig = nullptr, *spec = nullptr;
    ByolANet nb;
    for (int pass = 0; pass < 2; ++pass) {
        Bump wb(pass ? e->ws.p : nullptr);
        img = (float*)wb.take(img_elems * 4);
        if (byol_a_net_plan(nseg, T, D, wb, nb)) return 1;
        if (img_elems * 4 >= (1ul << 32) - 64) return fail("s3enc_forward: batch too large");
        if (fo.featurize) post = (float*)wb.take((size_t)nseg * D * 4);
        if (!fft) {
            sig = (float*)wb.take(s3::melspec_sig_elems(nseg, L) * 4);
            spec = (float*)wb.take(s3::melspec_spec_elems(nseg, L) * 4);
        }
        if (!pass) HIP_TRY(e->ws.ensure_on_stream(wb.off + 4096, st));
    }
    e->taps.clear();

    Sink sink{e, st, fo.featurize ? 2 : 0, out, (long)layer_stride, F32, nseg, D, fo.w, fo.feat_norm};
    HIP_TRY(sink.zero_without_terms(1, nseg));

    // ---- front end ----
    {
        const double frames = (double)nseg * T;
        Prof pr(e, st, fft ? "melspec:fft" : "melspec:gemm", fft ? frames * 5e4 : frames * (2.0 * 1026 * 1024 + 4.0 * 513),
                4.0 * ((double)nseg * L + (double)img_elems));
        HIP_TRY(hipMemsetAsync(img, 0, img_elems * 4, st));
        s3::MelspecParams m{};
        m.ptrs = d_ptr;
        m.valid = d_val;
        m.nseg = (int)nseg;
        m.L = L;
        m.mean = x.norm_mean;
        m.std_ = x.norm_std;
        m.out = img + 66 + 1;
        m.o_bs = (long)(T + 2) * 66;
        m.o_row = 66;
        m.fft = fft;
        m.sig = sig;
        m.spec = spec;
        if (const char* why = s3::melspec_refusal(m)) return fail(std::string("s3enc_forward: the BYOL-A front end refuses: ") + why);
        HIP_TRY(s3::launch_melspec(m, st));
    }

    e->taps["logmel"] = {img, (long)img_elems, F32};  // the bordered segments, (B S, frames + 2, 64 + 2)
    e->taps["fc"] = {nb.fcb[1], rows * D, F32};       // fc.3's output before its ReLU, (B S T / 8, d)

    float* dst = fo.featurize ? post : sink.slot32(0);
    if (byol_a_net_run(e, w, D, img, nseg, T, nb, dst, st)) return 1;
    if (sink.term(0)) {
        Prof pr(e, st, "emit_state", 0, 4.0 * nseg * D * 2);
        HIP_TRY(sink.emit(0, dst));
    }
    HIP_TRY(sink.done(0));
    return 0;
}


// frames: segments; valid: the utterance's own segments (the rows behind them are the reference's values, not zeros); rate:
// byol_a/expert.py:64-65, int(stride_secs * 16000)
FamilyOps kByolAFamily = {
    S3ENC_BYOL_A, "byol_a", "S3ENC_BYOL_A", "s3enc_create_byol_a", "the BYOL-A family needs its segment block",
    "BYOL-A (one hidden_states list)",
    [](const s3enc_config& c, const void* b) { return byol_a_check_config(c, *(const s3enc_byol_a_config*)b); },
    [](s3enc_encoder* e, const Ckpt& ck, const void* b) { e->byol_a_cfg = *(const s3enc_byol_a_config*)b; return byol_a_create(e, ck); },
    byol_a_forward,
    [](const s3enc_encoder* h, long n) { return byol_a_num_segments(h->byol_a_cfg, n); },
    nullptr,
    [](const s3enc_encoder* h) { return (int)h->byol_a_cfg.stride; }};

}  // namespace s3e
