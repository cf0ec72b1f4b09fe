// npc.hip — NPC, Non-autoregressive Predictive Coding (upstream/npc/npc.py:21-248, audio.py:53-115, expert.py:18-53), exact fp32:
// APC's kaldi log-mel front end (hamming window, CMVN over time) and a stack of stride-1 convolutions with NO length masking — the
// reference convolves all T = frames(n_max) rows of the padded batch, so the rows behind an utterance's own frames are not zeros
// from the first block on (bias and BatchNorm make them loud) and every row of every state is the reference's value for this T.
//
// Schedule (all on the caller's stream, no host synchronisation), three launches of convtaps.hip's kernel per block:
//   front end: per utterance launch_fbank into a zero-filled BORDERED (B, P + T + P, F) buffer, P = (kernel_size - 1) / 2;
//   block i:   k = 3 conv (+ BN1 folded) + act: x -> h (plain rows);
//              1 x 1 conv (+ BN2 folded) + x (pre-activation residual, i > 0) + act: h -> x, the bordered operand (in place: an
//              element's residual is read by the thread that overwrites it), and the block's state slot;
//              masked conv + tanh: x -> its state slot and the running sum, which lives in the last state's slot.
// The masked convolution reads only its two runs of live taps (8 / 6 / 4 / 2 of 15 at the released shape); tuning key npc_skip_taps
// = 0 runs all k taps over weights with zeros in the hole instead (equal values).  BatchNorm (eval: running statistics, eps 1e-5) is
// folded into the convolution before it in float64 and rounded to fp32 once.
// States in the reference's hook order (expert.py:28-41): blocks[0], masked_convs[0], blocks[1], ..., self.model's output[1] = the
// sum; with disable_cross_layer the hooks on the None entries never fire: the blocks, the last masked conv, and the same tensor again.
// vq_layers.* and postnet.* feed only the prediction the upstream discards: not uploaded.
#include <cmath>

#include "engine_internal.h"

namespace s3e {

namespace {
s3::FbankParams npc_fbank_params(const s3enc_npc_config& x) {
    s3::FbankParams f;
    f.sample_rate = 16000;
    f.num_mel_bins = x.num_mel_bins;
    f.frame_length_ms = x.frame_length_ms;
    f.frame_shift_ms = x.frame_shift_ms;
    f.preemph = 0.97f;
    f.delta_order = 0;
    f.use_cmvn = x.cmvn;
    f.cmvn_eps = 1e-10f;
    f.window = x.window;
    return f;
}
int npc_states(const s3enc_npc_config& x) { return x.disable_cross_layer ? x.n_blocks + 2 : 2 * x.n_blocks + 1; }
bool npc_has_mask(const s3enc_npc_config& x, int i) { return !x.disable_cross_layer || i == x.n_blocks - 1; }
int npc_mask(const s3enc_npc_config& x, int i) { return x.mask_size + 2 * (i + 1); }
}  // namespace

static int npc_check_config(const s3enc_config& c, const s3enc_npc_config& x) {
    static const char* dt[] = {"fp32", "bf16", "fp16", "fp32x3", "fp16x2"};
    if (c.compute_dtype < 0 || c.compute_dtype > 4) return fail("config: unknown compute_dtype");
    if (c.compute_dtype != S3ENC_F32)
        return fail(std::string("config: NPC (log-mel front end + masked convolutions) is built for compute dtype fp32 only; ") +
                    dt[c.compute_dtype] + " is not built");
    if (x.dim_bottleneck) return fail("config: npc dim_bottleneck is not built (the last state would have another width)");
    if (x.n_blocks < 1 || x.n_blocks > 8) return fail("config: npc n_blocks must be 1..8");
    if (x.kernel_size < 1 || !(x.kernel_size & 1)) return fail("config: npc kernel_size must be odd");
    if (x.mask_size < 1 || !(x.mask_size & 1)) return fail("config: npc mask_size must be odd");
    if (x.kernel_size > 63) return fail("config: npc kernel_size above 63 is not built");
    for (int i = 0; i < x.n_blocks; ++i)
        if (npc_has_mask(x, i) && x.kernel_size - npc_mask(x, i) <= 0)
            return fail("config: npc mask leaves no tap in block " + std::to_string(i) + " (mask " + std::to_string(npc_mask(x, i)) +
                        " of kernel_size " + std::to_string(x.kernel_size) + ")");
    if (x.hidden < 64 || x.hidden % 64 || x.hidden > 1024) return fail("config: npc hidden_size must be a multiple of 64, at most 1024");
    if (x.num_mel_bins < 16 || (x.num_mel_bins & 15) || x.num_mel_bins > 256)
        return fail("config: npc num_mel_bins must be a multiple of 16, at most 256 (a tap is a whole number of 64-byte K steps)");
    if (x.activate < 0 || x.activate > 1) return fail("config: npc activate must be 0 (relu) or 1 (tanh)");
    if (x.window < 0 || x.window > 1) return fail("config: npc window must be 0 (povey) or 1 (hamming)");
    const int size = (int)(16000 * x.frame_length_ms * 0.001), shift = (int)(16000 * x.frame_shift_ms * 0.001);
    if (size < 4 || shift < 4 || (size & 3) || (shift & 3) || size > 4096)
        return fail("config: npc frame_length / frame_shift must be a multiple of 4 samples (the front end's GEMM reads 16-byte vectors)");
    if (c.n_conv != 1 || c.conv_kernel[0] != size || c.conv_stride[0] != shift)
        return fail("config: npc carries its frame geometry as n_conv = 1, conv_kernel[0] / conv_stride[0] = window / shift in samples");
    if (c.conv_dim != x.hidden || c.embed_dim != x.hidden || c.encoder_layers != npc_states(x) - 1)
        return fail("config: npc conv_dim / embed_dim must be hidden_size and encoder_layers the number of states - 1");
    return 0;
}

static int npc_create(s3enc_encoder* e, const Ckpt& ck) {
    const s3enc_npc_config& x = e->npc_cfg;
    e->npc.reset(new NpcW());
    NpcW& w = *e->npc;
    const int H = x.hidden, k = x.kernel_size;
    std::vector<float> t, b, g, beta, mean, var, packed;
    // conv (+ BatchNorm on its running statistics) -> one conv: w' = w s, b' = (b - mean) s + beta, s = gamma / sqrt(var + eps)
    auto fold = [&](const std::string& bn, int cin_k) -> int {
        if (!x.batch_norm) return 0;
        GET(bn + ".weight", H, g);
        GET(bn + ".bias", H, beta);
        GET(bn + ".running_mean", H, mean);
        GET(bn + ".running_var", H, var);
        for (int n = 0; n < H; ++n) {
            const double s = (double)g[n] / std::sqrt((double)var[n] + 1e-5);
            for (int j = 0; j < cin_k; ++j) t[(size_t)n * cin_k + j] = (float)((double)t[(size_t)n * cin_k + j] * s);
            b[n] = (float)(((double)b[n] - (double)mean[n]) * s + (double)beta[n]);
        }
        return 0;
    };
    for (int i = 0; i < x.n_blocks; ++i) {
        const int C = i == 0 ? x.num_mel_bins : H;
        const std::string blk = "blocks." + std::to_string(i);
        w.w3.emplace_back(); w.b3.emplace_back(); w.w1.emplace_back(); w.b1.emplace_back();
        w.wm.emplace_back(); w.wm_dense.emplace_back(); w.bm.emplace_back();
        GET(blk + ".conv.weight", (long)H * C * 3, t);
        GET(blk + ".conv.bias", H, b);
        if (fold(blk + ".bn1", C * 3)) return 1;
        pack_conv_taps(t.data(), H, C, 3, 0, false, packed);
        UP(upload_f32(w.w3.back(), packed));
        UP(upload_f32(w.b3.back(), b));
        GET(blk + ".linear.weight", (long)H * H, t);
        GET(blk + ".linear.bias", H, b);
        if (fold(blk + ".bn2", H)) return 1;
        UP(upload_f32(w.w1.back(), t));
        UP(upload_f32(w.b1.back(), b));
        w.has_mask.push_back(npc_has_mask(x, i) ? 1 : 0);
        if (!w.has_mask.back()) continue;
        const std::string mc = "masked_convs." + std::to_string(i);
        const int m = npc_mask(x, i), head = (k - m) / 2;
        GET(mc + ".conv.weight", (long)H * H * k, t);
        GET(mc + ".conv.bias", H, b);
        if (ck.m.count(mc + ".conv_mask")) {  // the registered buffer, when the file carries it: it must be the mask of this configuration
            GET(mc + ".conv_mask", (long)H * H * k, g);
            for (size_t q = 0; q < g.size(); ++q) {
                const int j = (int)(q % k);
                if (g[q] != ((j >= head && j < head + m) ? 0.f : 1.f))
                    return fail("tensor '" + mc + ".conv_mask' is not the mask of kernel_size " + std::to_string(k) + " / mask_size " +
                                std::to_string(x.mask_size) + " (block " + std::to_string(i) + ": taps [" + std::to_string(head) + ", " +
                                std::to_string(head + m) + ") zeroed)");
            }
        }
        pack_conv_taps(t.data(), H, H, k, m, false, packed);
        UP(upload_f32(w.wm.back(), packed));
        pack_conv_taps(t.data(), H, H, k, m, true, packed);
        UP(upload_f32(w.wm_dense.back(), packed));
        UP(upload_f32(w.bm.back(), b));
    }
    return 0;
}

static int npc_forward(s3enc_handle e, const float* const* wav_ptrs_host, const int64_t* lengths, int32_t B, int64_t n_max_in,
                const FwdOpts& fo, void* out, int64_t layer_stride, hipStream_t st) {
    const s3enc_npc_config& x = e->npc_cfg;
    const NpcW& w = *e->npc;
    const int H = x.hidden, F = x.num_mel_bins, NB = x.n_blocks, k = x.kernel_size, P = (k - 1) / 2;
    const int NS = npc_states(x);
    const s3::FbankParams fp = npc_fbank_params(x);
    if (fo.selection != S3ENC_SEL_HIDDEN)
        return fail("s3enc_forward: feature_selection is not defined for NPC (the reference expert has one hidden_states list)");
    if (fo.featurize && !fo.w) return fail("s3enc_forward: featurize needs feat_w");
    if (!fo.featurize && fo.out_dtype != F32) return fail("s3enc_forward: out_dtype must be S3ENC_F32 for an NPC handle");
    if (e->aux_codewords || e->aux_codeids) return fail("s3enc_forward_aux: codewords / codeids are outputs of a wav2vec handle with a vector quantizer");
    if (B > 65535) return fail("s3enc_forward: batch too large");
    long n_max;
    if (batch_n_max(wav_ptrs_host, lengths, B, n_max_in, n_max)) return 1;
    for (int b = 0; b < B; ++b)
        if (s3::fbank_num_frames(lengths[b], fp) < 1)
            return fail("s3enc_forward: an utterance is shorter than one analysis window (NPC's front end keeps whole windows only)");
    const long T = s3::fbank_num_frames(n_max, fp);
    const long M = (long)B * T, TP = T + 2 * P;
    if (M > 0x7fffffffL || TP * std::max(H, F) * 4 >= (1L << 31)) return fail("s3enc_forward: batch too large");
    if (check_out(out, fo, layer_stride, M * H)) return 1;
    DeviceGuard dg(e->device);
    if (!dg.ok) return fail("s3enc_forward: hipSetDevice failed");

    // ---- workspace: the bordered feature rows, the bordered block output x, the plain rows h between a block's two convolutions;
    //      featurize: one state at a time and the running sum live here instead of in the caller's slab ----
    const bool feat_sum = fo.featurize;
    float *featb, *xb, *hb, *sbuf = nullptr, *sumb = nullptr;
    for (int pass = 0; pass < 2; ++pass) {
        Bump wb(pass ? e->ws.p : nullptr);
        featb = (float*)wb.take((size_t)B * TP * F * 4);
        xb = (float*)wb.take((size_t)B * TP * H * 4);
        hb = (float*)wb.take((size_t)M * H * 4);
        if (feat_sum) {
            sbuf = (float*)wb.take((size_t)M * H * 4);
            sumb = (float*)wb.take((size_t)M * H * 4);
        }
        if (!pass) HIP_TRY(e->ws.ensure_on_stream(wb.off + 4096, st));
    }
    e->taps.clear();

    Sink sink{e, st, feat_sum ? 2 : 0, out, (long)layer_stride, F32, M, H, fo.w, fo.feat_norm};
    HIP_TRY(sink.zero_without_terms(NS, M));
    float* sum = feat_sum ? sumb : sink.slot32(NS - 1);

    // ---- front end: zeros in the borders and behind every utterance's own frames (pad_sequence) ----
    {
        Prof pr(e, st, "npc_fbank", 0, 4.0 * ((double)B * n_max + (double)B * TP * (F + H)));
        HIP_TRY(hipMemsetAsync(featb, 0, (size_t)B * TP * F * 4, st));
        HIP_TRY(hipMemsetAsync(xb, 0, (size_t)B * TP * H * 4, st));
        for (int b = 0; b < B; ++b)
            HIP_TRY(s3::launch_fbank(fp, wav_ptrs_host[b], lengths[b], featb + ((size_t)b * TP + P) * F, F, st));
    }

    const bool skip = tuning().npc_skip_taps != 0;
    const int act = x.activate ? 2 : 1;
    for (int i = 0; i < NB; ++i) {
        const int C = i == 0 ? F : H;
        const int si_blk = x.disable_cross_layer ? i : 2 * i;
        // k = 3, padding 1: tap 0 of output row 0 reads bordered row P - 1
        ConvTapsParams q{};
        q.src = (i == 0 ? featb : xb) + (size_t)(P - 1) * C;
        q.src_bs = TP * C;
        q.C = C;
        q.W = (const float*)w.w3[i].p;
        q.bias = (const float*)w.b3[i].p;
        q.T = (int)T;
        q.N = H;
        q.B = B;
        q.taps0 = 3;
        q.act = act;
        q.dst = hb;
        q.dst_bs = T * H;
        q.ld_dst = H;
        {
            Prof pr(e, st, "conv_taps:k3", 2.0 * M * H * 3 * C, 4.0 * ((double)M * C + 3.0 * H * C + (double)M * H));
            HIP_TRY(launch_conv_taps(q, st));
        }
        // 1 x 1 + the block's input before the activation (i > 0) -> x (bordered) and the block's state
        float* sblk = feat_sum ? sbuf : sink.slot32(si_blk);
        ConvTapsParams l{};
        l.src = hb;
        l.src_bs = T * H;
        l.C = H;
        l.W = (const float*)w.w1[i].p;
        l.bias = (const float*)w.b1[i].p;
        l.T = (int)T;
        l.N = H;
        l.B = B;
        l.taps0 = 1;
        l.act = act;
        if (x.residual && i > 0) {
            l.res = xb + (size_t)P * H;
            l.res_bs = TP * H;
            l.ld_res = H;
        }
        l.dst = xb + (size_t)P * H;
        l.dst_bs = TP * H;
        l.ld_dst = H;
        l.state = sblk;
        l.state_bs = T * H;
        l.ld_state = H;
        {
            Prof pr(e, st, "conv_taps:1x1", 2.0 * M * H * H, 4.0 * ((double)M * H * (l.res ? 4 : 3) + (double)H * H));
            HIP_TRY(launch_conv_taps(l, st));
        }
        if (sink.term(si_blk)) {
            Prof pr(e, st, "emit_state", 0, 4.0 * M * H * 2);
            HIP_TRY(sink.emit(si_blk, sblk));
        }
        HIP_TRY(sink.done(si_blk));
        if (!w.has_mask[i]) continue;
        // masked conv + tanh -> its state and the running sum
        const int si_m = x.disable_cross_layer ? NB : 2 * i + 1;
        const int m = npc_mask(x, i), head = (k - m) / 2;
        float* sm = feat_sum ? sbuf : sink.slot32(si_m);
        ConvTapsParams c{};
        c.src = xb;
        c.src_bs = TP * H;
        c.C = H;
        c.W = (const float*)(skip ? w.wm[i].p : w.wm_dense[i].p);
        c.bias = (const float*)w.bm[i].p;
        c.T = (int)T;
        c.N = H;
        c.B = B;
        c.taps0 = skip ? head : k;
        c.gap = skip ? m : 0;
        c.taps1 = skip ? k - head - m : 0;
        c.act = 2;
        c.state = sm;
        c.state_bs = T * H;
        c.ld_state = H;
        c.sum = sum;
        c.sum_bs = T * H;
        c.ld_sum = H;
        c.sum_init = (x.disable_cross_layer || i == 0) ? 1 : 0;
        {
            Prof pr(e, st, "conv_taps:mask", 2.0 * M * H * (double)(c.taps0 + c.taps1) * H,
                    4.0 * ((double)M * H * (c.sum_init ? 3 : 4) + (double)H * H * (c.taps0 + c.taps1)));
            HIP_TRY(launch_conv_taps(c, st));
        }
        if (sink.term(si_m)) {
            Prof pr(e, st, "emit_state", 0, 4.0 * M * H * 2);
            HIP_TRY(sink.emit(si_m, sm));
        }
        HIP_TRY(sink.done(si_m));
    }
    if (sink.term(NS - 1)) {
        Prof pr(e, st, "emit_state", 0, 4.0 * M * H * 2);
        HIP_TRY(sink.emit(NS - 1, sum));
    }
    HIP_TRY(sink.done(NS - 1));
    return 0;
}


// frames, mask rule and rate are those of its one-layer "conv stack" (window, hop), as APC's
FamilyOps kNpcFamily = {
    S3ENC_NPC, "npc", "S3ENC_NPC", "s3enc_create_npc", "the NPC family needs its front-end / convolution block",
    "NPC (one hidden_states list)",
    [](const s3enc_config& c, const void* b) { return npc_check_config(c, *(const s3enc_npc_config*)b); },
    [](s3enc_encoder* e, const Ckpt& ck, const void* b) { e->npc_cfg = *(const s3enc_npc_config*)b; return npc_create(e, ck); },
    npc_forward};

}  // namespace s3e
