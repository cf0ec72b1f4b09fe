// apc.hip — APC / VQ-APC (upstream/apc/apc.py:101-169, audio.py:53-115, expert.py:18-59), exact fp32: a kaldi log-mel front end
// (hamming window, no deltas, CMVN over time) and 3 or 4 unidirectional GRU layers run on PACKED sequences — an utterance's
// recurrence stops at its own frame count, and pad_packed_sequence leaves zeros behind it.
//
// Schedule (all on the caller's stream, no host synchronisation):
//   front end: per utterance launch_fbank (fbank.hip: the folded DFT GEMM, mel + log, CMVN) into a zero-filled (B, T, F) buffer;
//   per layer: pre = x W_ih^T + b over the B * T rows (launch_gemm, K = F for layer 0; b = b_ih + the r and z parts of b_hh), then
//              launch_rnn_len (rnn.hip): one launch runs all steps, stops at every utterance's length, adds the layer's own input
//              for layers i > 0 when `residual`, and writes the zero tail — or, where it was measured to win (H = 512; tuning key
//              rnn_split), launch_rnn_step: the same recurrence bit for bit, one launch per step on a (S, B) grid.
// States — what the reference's three hooks return (expert.py:29-42): the input of rnn_layers[1], the input of rnn_layers[2] and the
// last layer's output after its residual; three states even for four layers, each (B, T, H), zero behind each length.
// VQ-APC: vq_layers.* and postnet.* feed only `predicted_BxLxM`, which the upstream discards (apc.py:143-169: the quantised
// tensor replaces the LAST layer's output only as the post-net's input) — no hooked state depends on them; not uploaded.
#include "engine_internal.h"

namespace s3e {

namespace {
s3::FbankParams apc_fbank_params(const s3enc_apc_config& x) {
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
}  // namespace

static int apc_check_config(const s3enc_config& c, const s3enc_apc_config& x) {
    static const char* dt[] = {"fp32", "bf16", "fp16", "fp32x3", "fp16x2"};
    if (c.compute_dtype < 0 || c.compute_dtype > 4) return fail("config: unknown compute_dtype");
    if (c.compute_dtype != S3ENC_F32)
        return fail(std::string("config: APC (log-mel front end + GRU) is built for compute dtype fp32 only; ") + dt[c.compute_dtype] +
                    " is not built");
    if (x.num_layers < 3)
        return fail("config: apc num_layers must be at least 3 (the reference's hooks read rnn_layers[1] and rnn_layers[2])");
    if (x.num_layers > 4) return fail("config: apc num_layers above 4 is not built");
    if (x.hidden < 64 || x.hidden % 64 || x.hidden > RNN_H_MAX)
        return fail("config: apc hidden_size must be a multiple of 64, at most " + std::to_string(RNN_H_MAX) + " (the recurrent kernel's limit)");
    if (x.window < 0 || x.window > 1) return fail("config: apc window must be 0 (povey) or 1 (hamming)");
    if (x.num_mel_bins < 4 || (x.num_mel_bins & 3) || x.num_mel_bins > 256)
        return fail("config: apc num_mel_bins must be a multiple of 4, at most 256");
    const int size = (int)(16000 * x.frame_length_ms * 0.001), shift = (int)(16000 * x.frame_shift_ms * 0.001);
    if (size < 4 || shift < 4 || (size & 3) || (shift & 3) || size > 4096)
        return fail("config: apc frame_length / frame_shift must be a multiple of 4 samples (the front end's GEMM reads 16-byte vectors)");
    if (c.n_conv != 1 || c.conv_kernel[0] != size || c.conv_stride[0] != shift)
        return fail("config: apc carries its frame geometry as n_conv = 1, conv_kernel[0] / conv_stride[0] = window / shift in samples");
    if (c.conv_dim != x.hidden || c.embed_dim != x.hidden || c.encoder_layers != 2)
        return fail("config: apc conv_dim / embed_dim must be hidden_size and encoder_layers 2 (three states)");
    return 0;
}

static int apc_create(s3enc_encoder* e, const Ckpt& ck) {
    const s3enc_apc_config& x = e->apc_cfg;
    e->apc.reset(new ApcW());
    for (int l = 0; l < x.num_layers; ++l)
        if (load_rnn_layer(ck, "rnn_layers." + std::to_string(l) + ".", "_l0", 3, x.hidden, l == 0 ? x.num_mel_bins : x.hidden, *e->apc)) return 1;
    return 0;
}

static int apc_forward(s3enc_handle e, const float* const* wav_ptrs_host, const int64_t* lengths, int32_t B, int64_t n_max_in,
                const FwdOpts& fo, void* out, int64_t layer_stride, hipStream_t st) {
    const s3enc_apc_config& x = e->apc_cfg;
    const ApcW& w = *e->apc;
    const int H = x.hidden, F = x.num_mel_bins, NL = x.num_layers;
    const s3::FbankParams fp = apc_fbank_params(x);
    if (fo.selection != S3ENC_SEL_HIDDEN)
        return fail("s3enc_forward: feature_selection is not defined for APC (the reference expert has one hidden_states list)");
    if (fo.featurize && !fo.w) return fail("s3enc_forward: featurize needs feat_w");
    if (!fo.featurize && fo.out_dtype != F32) return fail("s3enc_forward: out_dtype must be S3ENC_F32 for an APC handle");
    if (e->aux_codewords || e->aux_codeids) return fail("s3enc_forward_aux: codewords / codeids are outputs of a wav2vec handle with a vector quantizer");
    if (B > 65535) return fail("s3enc_forward: batch too large");
    long n_max;
    if (batch_n_max(wav_ptrs_host, lengths, B, n_max_in, n_max)) return 1;
    std::vector<int> frames(B);
    for (int b = 0; b < B; ++b) {
        const long tb = s3::fbank_num_frames(lengths[b], fp);
        if (tb < 1) return fail("s3enc_forward: an utterance is shorter than one analysis window (APC's front end keeps whole windows only)");
        frames[b] = (int)tb;
    }
    const long T = s3::fbank_num_frames(n_max, fp);
    const long M = (long)B * T;
    if (M > 0x7fffffffL) return fail("s3enc_forward: batch too large");
    if (check_out(out, fo, layer_stride, M * H)) return 1;
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
    const int split = rnn_split_pick(1, H, B);  // 0: one launch per layer; S: the step-split form (kernels.h)
    if (split && !rnn_split_ok(H, B, split))
        return fail("s3enc_forward: tuning rnn_split needs a power of two with hidden / S a multiple of 64 and S * B <= 256");
    float *feat, *pre, *hb[4], *hstep = nullptr;
    for (int pass = 0; pass < 2; ++pass) {
        Bump wb(pass ? e->ws.p : nullptr);
        feat = (float*)wb.take((size_t)M * F * 4);
        pre = (float*)wb.take((size_t)M * 3 * H * 4);
        for (int l = 0; l < 4; ++l) hb[l] = (l < NL && (feat_sum || (l >= 2 && l < NL - 1))) ? (float*)wb.take((size_t)M * H * 4) : nullptr;
        if (split) hstep = (float*)wb.take((size_t)2 * B * H * 4);
        if (!pass) HIP_TRY(e->ws.ensure_on_stream(wb.off + 4096, st));
    }
    e->taps.clear();

    // ---- where the states go ----
    Sink sink{e, st, feat_sum ? 2 : 0, out, (long)layer_stride, F32, M, H, fo.w, fo.feat_norm};
    HIP_TRY(sink.zero_without_terms(3, M));

    // ---- front end: (B, T, F), zeros behind every utterance's frames (pad_sequence) ----
    {
        Prof pr(e, st, "apc_fbank", 0, 4.0 * ((double)B * n_max + (double)M * F));
        HIP_TRY(hipMemsetAsync(feat, 0, (size_t)M * F * 4, st));
        for (int b = 0; b < B; ++b) HIP_TRY(s3::launch_fbank(fp, wav_ptrs_host[b], lengths[b], feat + (size_t)b * T * F, F, st));
    }

    // ---- GRU layers on packed sequences ----
    const float* xin = feat;
    int I = F;
    for (int l = 0; l < NL; ++l) {
        const int si = l < 2 ? l : (l == NL - 1 ? 2 : -1);  // the hooks: inputs of rnn_layers[1] and [2], the model's output
        HIP_TRY(linear_f32(e, st, {"gemm:apc_in", xin, w.w_ih[l].p, w.b_pre[l].p, M, 3 * H, I, 0, nullptr, pre}));
        float* hout = sink.slot32(si) ? sink.slot32(si) : hb[l];
        RnnLenParams r{};
        r.cell = 1;
        r.pre = pre;
        r.w = (const float*)w.w_hh[l].p;
        r.b_hn = (const float*)w.b_hn[l].p;
        r.B = B;
        r.T = (int)T;
        r.H = H;
        r.ld_pre = 3L * H;
        r.out = hout;
        r.ldo = H;
        r.len = d_len;
        r.res = (x.residual && l > 0) ? xin : nullptr;
        r.ld_res = H;
        {
            Prof pr(e, st, "rnn_gru_len", 2.0 * M * 3 * H * H, 4.0 * ((double)M * 3 * H + (double)M * H * (r.res ? 2 : 1)));
            if (split) {
                RnnStepParams q{};
                static_cast<RnnLenParams&>(q) = r;
                q.S = split;
                q.max_len = *std::max_element(frames.begin(), frames.end());
                q.hbuf = hstep;
                HIP_TRY(launch_rnn_step(q, st));
            } else {
                HIP_TRY(launch_rnn_len(r, st));
            }
        }
        if (sink.term(si)) {  // featurize: the state's term of the weighted sum
            Prof pr(e, st, "emit_state", 0, 4.0 * M * H * 2);
            HIP_TRY(sink.emit(si, hout));
        }
        HIP_TRY(sink.done(si));
        xin = hout;
        I = H;
    }
    return 0;
}


// frames, mask rule and rate are those of its one-layer "conv stack" (window, hop): valid_frames counts an utterance's own whole windows
FamilyOps kApcFamily = {
    S3ENC_APC, "apc", "S3ENC_APC", "s3enc_create_apc", "the APC family needs its front-end / GRU block",
    "APC (one hidden_states list of 3 states)",
    [](const s3enc_config& c, const void* b) { return apc_check_config(c, *(const s3enc_apc_config*)b); },
    [](s3enc_encoder* e, const Ckpt& ck, const void* b) { e->apc_cfg = *(const s3enc_apc_config*)b; return apc_create(e, ck); },
    apc_forward};

}  // namespace s3e
