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

int apc_check_config(const s3enc_config& c, const s3enc_apc_config& x) {
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

namespace {
struct ApcFetch {
    std::map<std::string, const s3enc_tensor*> m;
    int get(const std::string& name, long expect, std::vector<float>& out) const {
        auto it = m.find(name);
        if (it == m.end()) return fail("checkpoint is missing tensor '" + name + "'");
        long n = 1;
        for (int i = 0; i < it->second->ndim; ++i) n *= it->second->shape[i];
        if (n != expect)
            return fail("tensor '" + name + "' has " + std::to_string(n) + " elements, expected " + std::to_string(expect));
        out.assign(it->second->data, it->second->data + expect);
        return 0;
    }
};
}  // namespace

int apc_create(s3enc_encoder* e, const s3enc_tensor* tensors, int n_tensors) {
    const s3enc_apc_config& x = e->apc_cfg;
    const int H = x.hidden, F = x.num_mel_bins, NL = x.num_layers;
    ApcFetch ck;
    for (int i = 0; i < n_tensors; ++i)
        if (tensors[i].name && tensors[i].data) ck.m[tensors[i].name] = &tensors[i];
    e->apc.reset(new ApcW());
    ApcW& w = *e->apc;
    std::vector<float> t, t2, t3;
#define APC_GET(name, n, vec) \
    if (ck.get(name, n, vec)) return 1
#define APC_UP(buf, vec)                                                                       \
    do {                                                                                       \
        hipError_t _e = upload_f32(buf, vec);                                                  \
        if (_e != hipSuccess) return fail(std::string("weight upload failed: ") + hipGetErrorString(_e)); \
    } while (0)
    w.w_ih.resize(NL);
    w.b_pre.resize(NL);
    w.w_hh.resize(NL);
    w.b_hn.resize(NL);
    for (int l = 0; l < NL; ++l) {
        const std::string n = "rnn_layers." + std::to_string(l) + ".";
        const int I = l == 0 ? F : H;
        APC_GET(n + "weight_ih_l0", 3L * H * I, t);
        APC_UP(w.w_ih[l], t);
        APC_GET(n + "weight_hh_l0", 3L * H * H, t);
        pack_rnn_whh(t.data(), 3, H, t2);
        APC_UP(w.w_hh[l], t2);
        APC_GET(n + "bias_ih_l0", 3L * H, t);
        APC_GET(n + "bias_hh_l0", 3L * H, t2);
        for (int i = 0; i < 2 * H; ++i) t[i] += t2[i];  // b_hn stays inside r * (W_hn h + b_hn)
        APC_UP(w.b_pre[l], t);
        t3.assign(t2.begin() + 2 * H, t2.end());
        APC_UP(w.b_hn[l], t3);
    }
#undef APC_GET
#undef APC_UP
    return 0;
}

int apc_forward(s3enc_handle e, const float* const* wav_ptrs_host, const int64_t* lengths, int32_t B, int64_t n_max_in,
                const FwdOpts& fo, void* out, int64_t layer_stride, hipStream_t st) {
    const s3enc_apc_config& x = e->apc_cfg;
    const ApcW& w = *e->apc;
    const int H = x.hidden, F = x.num_mel_bins, NL = x.num_layers;
    const s3::FbankParams fp = apc_fbank_params(x);
    if (B <= 0) return fail("s3enc_forward: B must be positive");
    if (fo.selection != S3ENC_SEL_HIDDEN)
        return fail("s3enc_forward: feature_selection is not defined for APC (the reference expert has one hidden_states list)");
    if (fo.featurize && !fo.w) return fail("s3enc_forward: featurize needs feat_w");
    if (!fo.featurize && fo.out_dtype != F32) return fail("s3enc_forward: out_dtype must be S3ENC_F32 for an APC handle");
    if (e->aux_codewords || e->aux_codeids) return fail("s3enc_forward_aux: codewords / codeids are outputs of a wav2vec handle with a vector quantizer");
    if (B > 65535) return fail("s3enc_forward: batch too large");
    long n_max = 0;
    std::vector<int> frames(B);
    for (int b = 0; b < B; ++b) {
        if (lengths[b] <= 0) return fail("s3enc_forward: empty utterance");
        if (lengths[b] > n_max) n_max = lengths[b];
        if (!wav_ptrs_host[b]) return fail("s3enc_forward: null waveform pointer");
        const long tb = s3::fbank_num_frames(lengths[b], fp);
        if (tb < 1) return fail("s3enc_forward: an utterance is shorter than one analysis window (APC's front end keeps whole windows only)");
        frames[b] = (int)tb;
    }
    if (n_max_in > 0) {
        if (n_max_in < n_max) return fail("s3enc_forward: n_max is smaller than the longest utterance");
        n_max = n_max_in;
    }
    const long T = s3::fbank_num_frames(n_max, fp);
    const long M = (long)B * T;
    if (M > 0x7fffffffL) return fail("s3enc_forward: batch too large");
    if (!out) return fail("s3enc_forward: null output");
    if (!fo.featurize) {
        if (layer_stride < M * H) return fail("s3enc_forward: layer_stride < B*T*D");
        if (layer_stride & 3) return fail("s3enc_forward: layer_stride must be a multiple of 4 elements (vector stores)");
    }
    if ((uintptr_t)out & 15) return fail("s3enc_forward: out must be 16-byte aligned");
    DeviceGuard dg(e->device);
    if (!dg.ok) return fail("s3enc_forward: hipSetDevice failed");

    // ---- small device state: the frame counts ----
    const size_t tbl_bytes = (size_t)B * sizeof(int);
    HIP_TRY(e->small.ensure_on_stream(tbl_bytes + 1024, st));
    int* d_len = (int*)e->small.p;
    if (tbl_bytes > e->slot_bytes) {
        HIP_TRY(hipStreamSynchronize(st));
        if (e->pinned) HIP_TRY(hipHostFree(e->pinned));
        e->pinned = nullptr;
        e->slot_bytes = tbl_bytes * 4 + 4096;
        HIP_TRY(hipHostMalloc(&e->pinned, e->slot_bytes * s3enc_encoder::RING, hipHostMallocDefault));
    }
    {
        const int slot = e->slot_next;
        e->slot_next = (slot + 1) % s3enc_encoder::RING;
        HIP_TRY(hipEventSynchronize(e->slot_ev[slot]));
        char* hp = (char*)e->pinned + (size_t)slot * e->slot_bytes;
        memcpy(hp, frames.data(), tbl_bytes);
        HIP_TRY(hipMemcpyAsync(d_len, hp, tbl_bytes, hipMemcpyHostToDevice, st));
        HIP_TRY(hipEventRecord(e->slot_ev[slot], st));
    }

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
    bool first = true;
    if (feat_sum && fo.w[0] == 0.f && fo.w[1] == 0.f && fo.w[2] == 0.f) HIP_TRY(hipMemsetAsync(out, 0, (size_t)M * H * 4, st));
    auto emit = [&](int si, const float* state) -> hipError_t {  // featurize: the state's term of the weighted sum
        if (!feat_sum || fo.w[si] == 0.f) return hipSuccess;
        LnAcc a;
        a.acc = (float*)out;
        a.w = fo.w[si];
        a.mode = 1;
        a.norm = fo.feat_norm;
        a.init = first;
        first = false;
        Prof pr(e, st, "emit_state", 0, 4.0 * M * H * 2);
        return launch_emit_state(F32, state, M, H, nullptr, a, st);
    };
    auto done = [&](int si) -> hipError_t {
        if (feat_sum || e->layer_events.empty() || si >= (int)e->layer_events.size()) return hipSuccess;
        return hipEventRecord(e->layer_events[si], st);
    };

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
        GemmParams g{};
        g.A = xin;
        g.lda = I;
        g.W = w.w_ih[l].p;
        g.bias = (const float*)w.b_pre[l].p;
        g.M = (int)M;
        g.N = 3 * H;
        g.K = I;
        g.batches = 1;
        g.out32 = pre;
        g.ldo = 3L * H;
        {
            Prof pr(e, st, "gemm:apc_in", 2.0 * M * 3 * H * I, 4.0 * ((double)M * I + 3.0 * H * I + (double)M * 3 * H));
            HIP_TRY(launch_gemm(F32, g, st));
        }
        float* hout = (si >= 0 && !feat_sum) ? (float*)out + (long)si * layer_stride : hb[l];
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
        if (si >= 0) {
            HIP_TRY(emit(si, hout));
            HIP_TRY(done(si));
        }
        xin = hout;
        I = H;
    }
    return 0;
}

}  // namespace s3e
