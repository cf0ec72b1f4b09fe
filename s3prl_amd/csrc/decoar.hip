// decoar.hip — DeCoAR / DeCoAR-layers (upstream/decoar/{decoar,audio,expert}.py, upstream/decoar_layers/), exact fp32: a kaldi log-mel
// front end (hamming window, no deltas, CMVN over time), Linear 80 -> H, then a forward and a backward stack of unidirectional LSTM
// layers run on PACKED sequences — an utterance's recurrences stop at its own frame count, and pad_packed_sequence leaves zeros
// behind it — and the two stacks' outputs side by side (2 H channels).
//
// Schedule (all on the caller's stream, no host synchronisation):
//   front end: per utterance launch_fbank (fbank.hip) into a zero-filled (B, subsample * T, F) buffer;
//   projection: x = feat W^T + b over the B * T model rows (launch_gemm).  Keeping every `subsample`-th frame costs nothing: the
//              GEMM reads its rows at subsample * F floats apart;
//   layer 0:   pre = x [W_ih_fwd; W_ih_bwd]^T + (b_ih + b_hh): the two stacks share their input — ONE GEMM with N = 8 H;
//   layer l>0: per direction pre_d = y_{l-1}[:, d H : (d + 1) H] W_ih_d^T + b — the forward stack reads the forward half of the layer
//              below, the backward stack the backward half, at the same row: the reference flips every utterance before and after
//              its backward stack (flipBatch), here the recurrence walks the rows backwards instead and nothing is flipped;
//   then launch_rnnb (rnnb.hip): one launch per time step runs both directions for the whole batch, up to the longest length, and
//              writes y_l (B, T, 2 H) — straight into the caller's slab when it is a state — with the zero tail.
// States: `per_layer_states` 0 (decoar): the last layer; 1 (decoar_layers): every layer.
#include "engine_internal.h"

namespace s3e {

namespace {
s3::FbankParams decoar_fbank_params(const s3enc_decoar_config& x) {
    s3::FbankParams f;
    f.sample_rate = 16000;
    f.num_mel_bins = x.num_mel_bins;
    f.frame_length_ms = x.frame_length_ms;
    f.frame_shift_ms = x.frame_shift_ms;
    f.preemph = 0.97f;
    f.delta_order = 0;
    f.use_cmvn = 1;
    f.cmvn_eps = 1e-10f;
    f.window = 1;  // hamming: the reference's WINDOW_TYPE
    return f;
}
}  // namespace

static int decoar_check_config(const s3enc_config& c, const s3enc_decoar_config& x) {
    static const char* dt[] = {"fp32", "bf16", "fp16", "fp32x3", "fp16x2"};
    if (c.compute_dtype < 0 || c.compute_dtype > 4) return fail("config: unknown compute_dtype");
    if (c.compute_dtype != S3ENC_F32)
        return fail(std::string("config: DeCoAR (log-mel front end + LSTM stacks) is built for compute dtype fp32 only; ") +
                    dt[c.compute_dtype] + " is not built");
    if (x.num_layers < 1 || x.num_layers > 4) return fail("config: decoar num_layers must be 1..4");
    if (x.hidden < 64 || x.hidden % 64 || x.hidden > RNNB_H_MAX)
        return fail("config: decoar hidden must be a multiple of 64, at most " + std::to_string(RNNB_H_MAX) +
                    " (the batch-shared recurrent kernel's limit)");
    if (x.subsample < 1 || x.subsample > 2) return fail("config: decoar subsample must be 1 or 2");
    if (x.per_layer_states < 0 || x.per_layer_states > 1) return fail("config: decoar per_layer_states must be 0 or 1");
    if (x.num_mel_bins < 4 || (x.num_mel_bins & 3) || x.num_mel_bins > 256)
        return fail("config: decoar num_mel_bins must be a multiple of 4, at most 256");
    const int size = (int)(16000 * x.frame_length_ms * 0.001), shift = (int)(16000 * x.frame_shift_ms * 0.001);
    if (size < 4 || shift < 4 || (size & 3) || (shift & 3) || size > 4096)
        return fail("config: decoar frame_length / frame_shift must be a multiple of 4 samples (the front end's GEMM reads 16-byte vectors)");
    if (c.n_conv != 1 || c.conv_kernel[0] != size || c.conv_stride[0] != shift)
        return fail("config: decoar carries its frame geometry as n_conv = 1, conv_kernel[0] / conv_stride[0] = window / shift in samples");
    if (c.conv_dim != 2 * x.hidden || c.embed_dim != 2 * x.hidden || c.encoder_layers != (x.per_layer_states ? x.num_layers - 1 : 0))
        return fail("config: decoar conv_dim / embed_dim must be 2 * hidden and encoder_layers the number of states - 1");
    return 0;
}

static int decoar_create(s3enc_encoder* e, const Ckpt& ck) {
    const s3enc_decoar_config& x = e->decoar_cfg;
    const int H = x.hidden, F = x.num_mel_bins;
    e->decoar.reset(new DecoarW());
    DecoarW& w = *e->decoar;
    std::vector<float> t, t2, packed, w0, b0;
    GET("post_extract_proj.weight", (long)H * F, t);
    UP(upload_f32(w.proj_w, t));
    GET("post_extract_proj.bias", (long)H, t);
    UP(upload_f32(w.proj_b, t));
    static const char* stack[2] = {"forward_lstm.", "backward_lstm."};
    for (int l = 0; l < x.num_layers; ++l)
        for (int d = 0; d < 2; ++d) {
            const std::string p = stack[d], s = "_l" + std::to_string(l);
            w.w_ih[d].emplace_back();
            w.b_pre[d].emplace_back();
            w.w_hh[d].emplace_back();
            GET(p + "weight_hh" + s, 4L * H * H, t);
            s3::pack_rnnb_whh(t.data(), H, packed);
            UP(upload_f32(w.w_hh[d].back(), packed));
            GET(p + "bias_ih" + s, 4L * H, t2);
            GET(p + "bias_hh" + s, 4L * H, t);
            for (int i = 0; i < 4 * H; ++i) t2[i] += t[i];  // an LSTM's b_hh folds into the input projection's bias
            GET(p + "weight_ih" + s, 4L * H * H, t);
            if (l == 0) {  // both stacks read x: one (8 H, H) operand
                w0.insert(w0.end(), t.begin(), t.end());
                b0.insert(b0.end(), t2.begin(), t2.end());
            } else {
                UP(upload_f32(w.w_ih[d].back(), t));
                UP(upload_f32(w.b_pre[d].back(), t2));
            }
        }
    UP(upload_f32(w.w_ih0, w0));
    UP(upload_f32(w.b_pre0, b0));
    return 0;
}

// ceil(fbank frames / subsample)
static long decoar_num_frames(const s3enc_config&, const s3enc_decoar_config& x, long n_samples) {
    const long f = s3::fbank_num_frames(n_samples, decoar_fbank_params(x));
    return f < 1 ? 0 : (f + x.subsample - 1) / x.subsample;
}

static int decoar_forward(s3enc_handle e, const float* const* wav_ptrs_host, const int64_t* lengths, int32_t B, int64_t n_max_in,
                   const FwdOpts& fo, void* out, int64_t layer_stride, hipStream_t st) {
    const s3enc_decoar_config& x = e->decoar_cfg;
    const DecoarW& w = *e->decoar;
    const int H = x.hidden, F = x.num_mel_bins, NL = x.num_layers, sub = x.subsample;
    const int NS = x.per_layer_states ? NL : 1;
    const s3::FbankParams fp = decoar_fbank_params(x);
    if (fo.selection != S3ENC_SEL_HIDDEN)
        return fail("s3enc_forward: feature_selection is not defined for DeCoAR (the reference expert has one hidden_states list)");
    if (fo.featurize && !fo.w) return fail("s3enc_forward: featurize needs feat_w");
    if (!fo.featurize && fo.out_dtype != F32) return fail("s3enc_forward: out_dtype must be S3ENC_F32 for a DeCoAR handle");
    if (e->aux_codewords || e->aux_codeids) return fail("s3enc_forward_aux: codewords / codeids are outputs of a wav2vec handle with a vector quantizer");
    if (B > RNNB_B_MAX)
        return fail("s3enc_forward: a DeCoAR batch holds at most " + std::to_string(RNNB_B_MAX) + " utterances (the batch-shared recurrent kernel's limit)");
    long n_max;
    if (batch_n_max(wav_ptrs_host, lengths, B, n_max_in, n_max)) return 1;
    std::vector<int> frames(B);
    for (int b = 0; b < B; ++b) {
        if (s3::fbank_num_frames(lengths[b], fp) < 2)
            return fail("s3enc_forward: an utterance has fewer than 2 analysis windows (DeCoAR's front end normalises by the standard deviation over time: one frame has none)");
        frames[b] = (int)decoar_num_frames(e->cfg, x, lengths[b]);
    }
    const long T = decoar_num_frames(e->cfg, x, n_max);
    const long M = (long)B * T;
    if (M > 0x7fffffffL / 8) return fail("s3enc_forward: batch too large");
    if (check_out(out, fo, layer_stride, M * 2 * H)) return 1;
    DeviceGuard dg(e->device);
    if (!dg.ok) return fail("s3enc_forward: hipSetDevice failed");

    // ---- small device state: the frame counts ----
    const size_t tbl_bytes = (size_t)B * sizeof(int);
    HIP_TRY(e->small.ensure_on_stream(tbl_bytes + 1024, st));
    int* d_len = (int*)e->small.p;
    char* hp;
    if (stage_begin(e, tbl_bytes, st, hp)) return 1;
    memcpy(hp, frames.data(), tbl_bytes);
    if (stage_commit(e, hp, d_len, tbl_bytes, st)) return 1;

    // ---- workspace ----
    const bool feat_sum = fo.featurize;
    const size_t state = s3::rnnb_state_elems(B, H);
    float *feat, *xp, *pre, *yb[2], *hbuf, *cbuf;
    for (int pass = 0; pass < 2; ++pass) {
        Bump wb(pass ? e->ws.p : nullptr);
        feat = (float*)wb.take((size_t)M * sub * F * 4);
        xp = (float*)wb.take((size_t)M * H * 4);
        pre = (float*)wb.take((size_t)M * 8 * H * 4);
        for (int i = 0; i < 2; ++i) yb[i] = (float*)wb.take((size_t)M * 2 * H * 4);  // layer outputs that are no slab slot
        hbuf = (float*)wb.take(2 * state * 4);
        cbuf = (float*)wb.take(state * 4);
        if (!pass) HIP_TRY(e->ws.ensure_on_stream(wb.off + 4096, st));
    }
    e->taps.clear();

    // ---- where the states go ----
    Sink sink{e, st, feat_sum ? 2 : 0, out, (long)layer_stride, F32, M, 2 * H, fo.w, fo.feat_norm};
    HIP_TRY(sink.zero_without_terms(NS, M));

    // ---- front end: (B, sub * T, F), zeros behind every utterance's frames (pad_sequence) ----
    {
        Prof pr(e, st, "decoar_fbank", 0, 4.0 * ((double)B * n_max + (double)M * sub * F));
        HIP_TRY(hipMemsetAsync(feat, 0, (size_t)M * sub * F * 4, st));
        for (int b = 0; b < B; ++b) HIP_TRY(s3::launch_fbank(fp, wav_ptrs_host[b], lengths[b], feat + (size_t)b * T * sub * F, F, st));
    }

    // ---- post_extract_proj on every sub-th frame ----
    HIP_TRY(linear_f32(e, st, {"gemm:decoar_proj", feat, w.proj_w.p, w.proj_b.p, M, H, F, 0, nullptr, xp, nullptr, (long)sub * F}));

    // ---- the two LSTM stacks on packed sequences ----
    const int max_len = *std::max_element(frames.begin(), frames.end());
    const float* yin = nullptr;
    for (int l = 0; l < NL; ++l) {
        const int si = x.per_layer_states ? l : (l == NL - 1 ? 0 : -1);
        for (int d = 0; d < (l == 0 ? 1 : 2); ++d) {
            if (l == 0)  // both directions read the same rows: one (8 H, H) operand
                HIP_TRY(linear_f32(e, st, {"gemm:decoar_in", xp, w.w_ih0.p, w.b_pre0.p, M, 8 * H, H, 0, nullptr, pre}));
            else
                HIP_TRY(linear_f32(e, st, {"gemm:decoar_in", yin + (long)d * H, w.w_ih[d][l].p, w.b_pre[d][l].p, M, 4 * H, H, 0, nullptr,
                                           pre + (long)d * 4 * H, nullptr, 2L * H, 8L * H}));
        }
        float* yout = sink.slot32(si) ? sink.slot32(si) : yb[l & 1];
        s3::RnnbParams r{};
        r.pre_fwd = pre;
        r.pre_bwd = pre + 4L * H;
        r.w_fwd = (const float*)w.w_hh[0][l].p;
        r.w_bwd = (const float*)w.w_hh[1][l].p;
        r.len = d_len;
        r.B = B;
        r.T = (int)T;
        r.H = H;
        r.ld_pre = 8L * H;
        r.out = yout;
        r.ldo = 2L * H;
        r.max_len = max_len;
        r.hbuf = hbuf;
        r.cbuf = cbuf;
        if (const char* why = s3::rnnb_refusal(r)) return fail(std::string("s3enc_forward: the recurrent step refuses: ") + why);
        {
            Prof pr(e, st, "rnnb_lstm", 2.0 * 2 * M * 4 * H * H, 4.0 * (2.0 * max_len * 4 * H * H + (double)M * 8 * H + (double)M * 2 * H));
            HIP_TRY(s3::launch_rnnb(r, st));
        }
        if (sink.term(si)) {  // featurize: the state's term of the weighted sum
            Prof pr(e, st, "emit_state", 0, 4.0 * M * 2 * H * 2);
            HIP_TRY(sink.emit(si, yout));
        }
        HIP_TRY(sink.done(si));
        yin = yout;
    }
    return 0;
}


// valid: the utterance's own frame count (its packed length)
FamilyOps kDecoarFamily = {
    S3ENC_DECOAR, "decoar", "S3ENC_DECOAR", "s3enc_create_decoar", "the DeCoAR family needs its front-end / LSTM block",
    "DeCoAR (one hidden_states list)",
    [](const s3enc_config& c, const void* b) { return decoar_check_config(c, *(const s3enc_decoar_config*)b); },
    [](s3enc_encoder* e, const Ckpt& ck, const void* b) { e->decoar_cfg = *(const s3enc_decoar_config*)b; return decoar_create(e, ck); },
    decoar_forward,
    [](const s3enc_encoder* h, long n) { return decoar_num_frames(h->cfg, h->decoar_cfg, n); }};

}  // namespace s3e
