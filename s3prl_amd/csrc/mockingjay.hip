// mockingjay.hip — Mockingjay / TERA / AudioALBERT (upstream/mockingjay/{expert,builder,model}.py), exact fp32: a spectrogram front
// end, the input representation Linear(input_dim, D) + sinusoid position row + LayerNorm, and num_hidden_layers post-LN BERT layers
// (AudioALBERT: one layer's weights run that many times, uploaded once).  Every LayerNorm is the TF-style one with the
// checkpoint's own layer_norm_eps (1e-12): the row kernel below takes eps as a parameter; the 1e-5 kernels of norm.hip are untouched.
//
// Schedule (all on the caller's stream, no host synchronisation):
//   front end   mel: launch_logmel (logmel.hip) for the whole batch; kaldi: launch_fbank per utterance (fbank.hip, its bits unchanged)
//               into a zero-filled feature buffer of Tp = n * Tc rows per utterance;
//   input repr  launch_gemm (K = input_dim, + bias) then layernorm_eps_kernel with the position row of t mod Tc;
//   per layer   q|k|v GEMM (q and its bias pre-scaled by 1 / 8 = head_dim^-0.5 at upload: a power of two, so the scores are the
//               reference's divided ones bit for bit in exact arithmetic), launch_attention over B * n sequences of Tc rows with
//               per-sequence key counts, out-proj GEMM + residual, LayerNorm(eps), fc1 GEMM + erf-GELU, fc2 GEMM + residual,
//               LayerNorm(eps) — which also writes the state's live-layout rows into the caller's slab.
// Chunking (builder.py:256-289): T > sequence_length > 0 splits time as torch.chunk(x, n0 = ceil(T / sequence_length), dim = 1) does:
// chunks of Tc = ceil(T / n0) rows, n = ceil(T / Tc) of them, the last one shorter.  Chunks run as extra batch entries: utterance b's
// rows live at [b * Tp, b * Tp + T) of buffers with Tp = n * Tc rows per utterance, sequence b * n + c is chunk c, positions restart
// with t mod Tc, and the key count of a sequence is the utterance's live frames inside that chunk.  The rows the padding adds
// ([T, Tp) of an utterance) are zero feature rows; they are computed like any padding row and never emitted.
// Padding rows (at or behind an utterance's frame count): the reference masks keys with -10000, which underflows to exactly 0 after
// the softmax wherever a chunk has a live key, so live rows agree with the -inf mask of launch_attention.  A chunk without a
// live key attends to its key 0 alone here (key count clamped to 1), where the reference attends uniformly: padding rows are
// finite, deterministic and inside the buffer, and they are not the reference's values.
#include "engine_internal.h"

namespace s3 {
namespace {

template <int NCH>
__global__ __launch_bounds__(256) void layernorm_eps_kernel(LnEpsParams p) {
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= p.rows) return;
    const int lane = threadIdx.x & 63;
    const int C = p.C, nch = C >> 2;
    const float* xr = p.x + row * C;
    const float* pr = p.pos ? p.pos + (row % p.Tc) * C : nullptr;
    float4 v[NCH];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
        const int ch = lane + 64 * i;
        v[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (ch < nch) {
            v[i] = *(const float4*)(xr + 4 * ch);
            if (pr) {
                const float4 q = *(const float4*)(pr + 4 * ch);
                v[i].x += q.x;
                v[i].y += q.y;
                v[i].z += q.z;
                v[i].w += q.w;
            }
        }
        s += (v[i].x + v[i].y) + (v[i].z + v[i].w);
    }
    const float invC = 1.f / (float)C;
    const float mu = wave_sum(s) * invC;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
        const int ch = lane + 64 * i;
        if (ch < nch) {
            const float a = v[i].x - mu, b = v[i].y - mu, c = v[i].z - mu, d = v[i].w - mu;
            q += (a * a + b * b) + (c * c + d * d);
        }
    }
    const float var = wave_sum(q) * invC;
    const float rs = 1.f / sqrtf(var + p.eps);
    float* o1 = p.out ? p.out + row * C : nullptr;
    float* o2 = nullptr;
    if (p.out2) {
        const long b = row / p.Tp, t = row - b * p.Tp;
        if (t < p.T) o2 = p.out2 + (b * p.T + t) * C;
    }
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
        const int ch = lane + 64 * i;
        if (ch >= nch) continue;
        const float4 g = *(const float4*)(p.gamma + 4 * ch), bt = *(const float4*)(p.beta + 4 * ch);
        float4 y;
        y.x = ln_affine(v[i].x, mu, rs, g.x, bt.x);
        y.y = ln_affine(v[i].y, mu, rs, g.y, bt.y);
        y.z = ln_affine(v[i].z, mu, rs, g.z, bt.z);
        y.w = ln_affine(v[i].w, mu, rs, g.w, bt.w);
        if (o1) *(float4*)(o1 + 4 * ch) = y;
        if (o2) *(float4*)(o2 + 4 * ch) = y;
    }
}

}  // namespace

hipError_t launch_layernorm_eps(const LnEpsParams& p, hipStream_t st) {
    if (p.rows <= 0) return hipSuccess;
    if ((p.C & 3) || p.C < 4 || p.C > 2048 || p.Tc < 1 || p.Tp < 1 || p.T < 1 || p.T > p.Tp || !(p.eps >= 0.f)) return hipErrorInvalidValue;
    if ((((uintptr_t)p.x | (uintptr_t)p.pos | (uintptr_t)p.gamma | (uintptr_t)p.beta | (uintptr_t)p.out | (uintptr_t)p.out2)) & 15)
        return hipErrorInvalidValue;
    if (p.out2 && p.rows % p.Tp) return hipErrorInvalidValue;
    if ((p.rows + 3) / 4 > 0x7fffffffL) return hipErrorInvalidValue;
    const int per_lane = ((p.C >> 2) + 63) / 64;
    dim3 grid((unsigned)((p.rows + 3) / 4)), block(256);
#define S3_LNE(N) hipLaunchKernelGGL((layernorm_eps_kernel<N>), grid, block, 0, st, p)
    if (per_lane <= 1) S3_LNE(1);
    else if (per_lane == 2) S3_LNE(2);
    else if (per_lane == 3) S3_LNE(3);
    else if (per_lane == 4) S3_LNE(4);
    else S3_LNE(8);
#undef S3_LNE
    return hipGetLastError();
}

}  // namespace s3

namespace s3e {

namespace {
s3::FbankParams mj_fbank_params(const s3enc_mockingjay_config& x) {
    s3::FbankParams f;
    f.sample_rate = 16000;
    f.num_mel_bins = x.fbank_num_mel_bins;
    f.frame_length_ms = x.fbank_frame_length_ms;
    f.frame_shift_ms = x.fbank_frame_shift_ms;
    f.preemph = x.fbank_preemphasis;
    f.delta_order = x.fbank_delta_order;
    f.delta_win = x.fbank_delta_win_length;
    f.use_cmvn = x.fbank_use_cmvn;
    f.cmvn_eps = x.fbank_cmvn_eps;
    f.window = 0;
    return f;
}
}  // namespace

// builder.py:469-481: pos / 10000^(2 (j / 2) / D), sin on even j, cos on odd j; float64, rounded once to fp32
void mj_position_rows(int rows, int D, std::vector<float>& out) {
    out.resize((size_t)rows * D);
    for (int t = 0; t < rows; ++t)
        for (int j = 0; j < D; ++j) {
            const double a = (double)t / std::pow(10000.0, 2.0 * (double)(j / 2) / (double)D);
            out[(size_t)t * D + j] = (float)((j & 1) ? std::cos(a) : std::sin(a));
        }
}

static long mj_num_frames(const s3enc_config& c, const s3enc_mockingjay_config& x, long n) {
    return x.frontend == 1 ? (n > 200 ? logmel_num_frames(n) : 0) : conv_len(c, n, c.n_conv);
}

static int mj_valid_frames(const s3enc_config& c, const s3enc_mockingjay_config& x, long length, long n_max) {
    const long T = mj_num_frames(c, x, n_max);
    if (T <= 0) return 0;
    long v;
    if (x.frontend == 1) v = x.cmvn ? logmel_frame_count(length, n_max) : T;  // without CMVN no feature row is zero: the reference sees T
    else v = conv_len(c, length, c.n_conv);
    return (int)std::max(0L, std::min(v, T));
}

static int mj_check_config(const s3enc_config& c, const s3enc_mockingjay_config& x) {
    static const char* dt[] = {"fp32", "bf16", "fp16", "fp32x3", "fp16x2"};
    if (c.compute_dtype < 0 || c.compute_dtype > 4) return fail("config: unknown compute_dtype");
    if (c.compute_dtype != S3ENC_F32)
        return fail(std::string("config: Mockingjay / TERA / AudioALBERT are built for compute dtype fp32 only; ") + dt[c.compute_dtype] +
                    " is not built");
    if (x.pre_layer_norm) return fail("config: mockingjay pre_layer_norm = True is not built (no released checkpoint uses it)");
    if (x.hidden_act != 0) return fail("config: mockingjay hidden_act other than gelu is not built");
    if (c.heads < 1 || c.embed_dim != c.heads * 64)
        return fail("config: mockingjay hidden_size / num_attention_heads must be 64 (the attention kernel's head width)");
    if (c.encoder_layers < 1 || c.encoder_layers > 64) return fail("config: mockingjay num_hidden_layers out of range");
    if (c.ffn_dim < 4 || (c.ffn_dim & 3)) return fail("config: mockingjay intermediate_size must be a multiple of 4");
    if (x.input_dim < 4 || (x.input_dim & 3) || x.input_dim > 4096) return fail("config: mockingjay input_dim must be a multiple of 4");
    if (!(x.layer_norm_eps >= 0.f) || x.layer_norm_eps > 1.f) return fail("config: mockingjay layer_norm_eps out of range");
    if (x.sequence_length < 0) return fail("config: mockingjay sequence_length must not be negative");
    if (c.n_conv != 1 || c.conv_stride[0] != 160 || c.conv_dim != c.embed_dim)
        return fail("config: mockingjay carries its frame geometry as n_conv = 1, conv_stride[0] = 160, conv_dim = embed_dim");
    if (x.frontend == 1) {
        if (c.conv_kernel[0] != 0) return fail("config: mockingjay mel front end: conv_kernel[0] must be 0 (centred frames)");
        if (x.n_mels != x.input_dim || x.n_mels > 256) return fail("config: mockingjay n_mels must equal input_dim, at most 256");
        if (!(x.target_level <= 0.f && x.target_level >= -200.f)) return fail("config: mockingjay target_level out of range");
    } else if (x.frontend == 0) {
        const s3::FbankParams f = mj_fbank_params(x);
        const int size = (int)(16000 * f.frame_length_ms * 0.001), shift = (int)(16000 * f.frame_shift_ms * 0.001);
        if (shift != 160 || size < 4 || (size & 3) || size > 4096 || c.conv_kernel[0] != size)
            return fail("config: mockingjay kaldi front end: a 10 ms shift and conv_kernel[0] = the analysis window in samples (a multiple of 4)");
        if (f.delta_order < 0 || f.delta_order > 2 || f.delta_win < 3 || !(f.delta_win & 1)) return fail("config: mockingjay unsupported delta configuration");
        if (f.num_mel_bins < 1 || f.num_mel_bins * (f.delta_order + 1) != x.input_dim)
            return fail("config: mockingjay input_dim must be num_mel_bins * (delta_order + 1)");
    } else {
        return fail("config: mockingjay frontend must be 0 (kaldi) or 1 (mel)");
    }
    return 0;
}

static int mj_create(s3enc_encoder* e, const Ckpt& ck) {
    const s3enc_mockingjay_config& x = e->mj_cfg;
    const s3enc_config& c = e->cfg;
    const int D = c.embed_dim, FF = c.ffn_dim, F = x.input_dim;
    e->mj.reset(new MjW());
    MjW& w = *e->mj;
    std::vector<float> t, t2;
    const std::string ir = "input_representations.";
    GET(ir + "spec_transform.weight", (long)D * F, t);
    UP(upload_f32(w.in_w, t));
    GET(ir + "spec_transform.bias", D, t);
    UP(upload_f32(w.in_b, t));
    GET(ir + "LayerNorm.weight", D, t);
    UP(upload_f32(w.in_g, t));
    GET(ir + "LayerNorm.bias", D, t);
    UP(upload_f32(w.in_beta, t));
    const int NW = x.share_layer ? 1 : c.encoder_layers;  // share_layer: the ModuleList holds ONE module (model.py:343-344)
    w.layers.resize(NW);
    for (int l = 0; l < NW; ++l)  // 1 / sqrt(64): exact
        if (load_layer(e, ck, "encoder.layer." + std::to_string(l) + ".", kBertLayer, 0.125f, false, w.layers[l])) return 1;
    w.pos_rows = x.sequence_length > 0 ? x.sequence_length : 3008;  // a chunk never has more rows than sequence_length
    mj_position_rows(w.pos_rows, D, t);
    UP(upload_f32(w.pos, t));
    return 0;
}

static int mj_forward(s3enc_handle e, const float* const* wav_ptrs_host, const int64_t* lengths, int32_t B, int64_t n_max_in,
               const FwdOpts& fo, void* out, int64_t layer_stride, hipStream_t st) {
    const s3enc_mockingjay_config& x = e->mj_cfg;
    const s3enc_config& c = e->cfg;
    MjW& w = *e->mj;
    const int D = c.embed_dim, FF = c.ffn_dim, F = x.input_dim, NL = c.encoder_layers, H = c.heads;
    const bool mel = x.frontend == 1;
    if (fo.selection != S3ENC_SEL_HIDDEN)
        return fail("s3enc_forward: feature_selection is not defined for Mockingjay / TERA / AudioALBERT (the reference expert has one hidden_states list)");
    if (fo.featurize && !fo.w) return fail("s3enc_forward: featurize needs feat_w");
    if (!fo.featurize && fo.out_dtype != F32) return fail("s3enc_forward: out_dtype must be S3ENC_F32 for a Mockingjay handle");
    if (e->aux_codewords || e->aux_codeids) return fail("s3enc_forward_aux: codewords / codeids are outputs of a wav2vec handle with a vector quantizer");
    if (B > 65535) return fail("s3enc_forward: batch too large");
    long n_max;
    if (batch_n_max(wav_ptrs_host, lengths, B, n_max_in, n_max)) return 1;
    for (int b = 0; mel && b < B; ++b)
        if (lengths[b] <= 200)
            return fail("s3enc_forward: an utterance of at most 200 samples has no reflect-padded centred frame (torch.stft refuses it)");
    const long T = mj_num_frames(c, x, n_max);
    if (T < 1) return fail("s3enc_forward: the batch is shorter than one analysis window");
    std::vector<int> frames(B);
    for (int b = 0; b < B; ++b) {
        frames[b] = mj_valid_frames(c, x, lengths[b], n_max);
        if (frames[b] < 1) return fail("s3enc_forward: an utterance is shorter than one analysis window");
        if (mel && x.cmvn && frames[b] < 2)
            return fail("s3enc_forward: an utterance with a single frame inside this batch has no standard deviation for the CMVN");
    }
    // torch.chunk(x, ceil(T / sequence_length), dim = 1): chunks of Tc rows, n of them
    long Tc = T, n = 1;
    if (x.sequence_length > 0 && T > x.sequence_length) {
        const long n0 = (T + x.sequence_length - 1) / x.sequence_length;
        Tc = (T + n0 - 1) / n0;
        n = (T + Tc - 1) / Tc;
    }
    const long Tp = n * Tc, M = (long)B * T, Mp = (long)B * Tp, NS = (long)B * n;
    if (Mp > 0x7fffffffL / 4 || NS > 0x7fffffffL) return fail("s3enc_forward: batch too large");
    if (check_out(out, fo, layer_stride, M * D)) return 1;
    DeviceGuard dg(e->device);
    if (!dg.ok) return fail("s3enc_forward: hipSetDevice failed");
    if (Tc > w.pos_rows) {  // only without a sequence_length: grow the position table (synchronising, once per new maximum)
        HIP_TRY(hipStreamSynchronize(st));
        std::vector<float> t;
        w.pos_rows = (int)(Tc + Tc / 4);
        mj_position_rows(w.pos_rows, D, t);
        HIP_TRY(upload_f32(w.pos, t));
    }

    // ---- small device state: waveform pointers, lengths, frame counts, per-sequence key counts ----
    const size_t o_ptr = 0, o_len = o_ptr + (size_t)B * 8, o_cnt = o_len + (size_t)B * 8, o_kv = o_cnt + (((size_t)B * 4 + 7) & ~(size_t)7);
    const size_t tbl_bytes = o_kv + (size_t)NS * 4;
    HIP_TRY(e->small.ensure_on_stream(tbl_bytes + 1024, st));
    char* dsm = (char*)e->small.p;
    char* hp;
    if (stage_begin(e, tbl_bytes, st, hp)) return 1;
    for (int b = 0; b < B; ++b) {
        ((const float**)(hp + o_ptr))[b] = wav_ptrs_host[b];
        ((long*)(hp + o_len))[b] = (long)lengths[b];
        ((int*)(hp + o_cnt))[b] = frames[b];
        for (long ch = 0; ch < n; ++ch) {
            const long rows = std::min(Tc, T - ch * Tc);  // the last chunk is shorter
            long kv = std::min(std::max((long)frames[b] - ch * Tc, 0L), rows);
            ((int*)(hp + o_kv))[b * n + ch] = (int)std::max(kv, 1L);  // a chunk without a live key: key 0 alone (finite rows)
        }
    }
    if (stage_commit(e, hp, dsm, tbl_bytes, st)) return 1;
    const float* const* d_ptr = (const float* const*)(dsm + o_ptr);
    const long* d_len = (const long*)(dsm + o_len);
    const int* d_cnt = (const int*)(dsm + o_cnt);
    const int* d_kv = (const int*)(dsm + o_kv);

    // ---- workspace ----
    const bool feat_sum = fo.featurize;
    float *feat, *xa, *xb, *tmp, *qkv, *ctx, *hbuf, *stc = nullptr, *sig = nullptr, *spec = nullptr, *scale = nullptr;
    for (int pass = 0; pass < 2; ++pass) {
        Bump wb(pass ? e->ws.p : nullptr);
        feat = (float*)wb.take((size_t)Mp * F * 4);
        xa = (float*)wb.take((size_t)Mp * D * 4);
        xb = (float*)wb.take((size_t)Mp * D * 4);
        tmp = (float*)wb.take((size_t)Mp * D * 4);
        qkv = (float*)wb.take((size_t)Mp * 3 * D * 4);
        ctx = (float*)wb.take((size_t)Mp * D * 4);
        hbuf = (float*)wb.take((size_t)Mp * FF * 4);
        if (feat_sum) stc = (float*)wb.take((size_t)M * D * 4);
        if (mel) {
            scale = (float*)wb.take((size_t)B * 4);
            sig = (float*)wb.take(logmel_sig_elems(B, n_max) * 4);
            spec = (float*)wb.take(logmel_spec_elems(B, n_max) * 4);
        }
        if (!pass) HIP_TRY(e->ws.ensure_on_stream(wb.off + 4096, st));
    }
    e->taps.clear();

    // ---- where the states go ----
    Sink sink{e, st, feat_sum ? 2 : 0, out, (long)layer_stride, F32, M, D, fo.w, fo.feat_norm};
    HIP_TRY(sink.zero_without_terms(NL + 1, M));
    // a state leaves its LayerNorm as compact (B, T, D) rows: into its slot of the slab, or into `stc` for its Featurizer term
    auto state_done = [&](int si) -> int {
        if (sink.term(si)) {
            Prof pr(e, st, "emit_state", 0, 4.0 * M * D * 2);
            HIP_TRY(sink.emit(si, stc));
        }
        HIP_TRY(sink.done(si));
        return 0;
    };
    auto ln = [&](const float* in, const float* pos, const DevBuf& g, const DevBuf& b, float* o, int si) -> hipError_t {
        LnEpsParams p;
        p.x = in;
        p.pos = pos;
        p.Tc = (int)Tc;
        p.gamma = (const float*)g.p;
        p.beta = (const float*)b.p;
        p.eps = x.layer_norm_eps;
        p.rows = Mp;
        p.C = D;
        p.out = o;
        p.out2 = si < 0 ? nullptr : (sink.slot32(si) ? sink.slot32(si) : stc);
        p.Tp = (int)Tp;
        p.T = (int)T;
        Prof pr(e, st, "layernorm_eps", 0, 4.0 * Mp * D * (si >= 0 ? 3 : 2));
        return launch_layernorm_eps(p, st);
    };

    // ---- front end: (B, Tp, F), zeros behind every utterance's frames and in the rows the chunk padding adds ----
    {
        Prof pr(e, st, mel ? "mj_logmel" : "mj_fbank", 0, 4.0 * ((double)B * n_max + (double)M * F));
        HIP_TRY(hipMemsetAsync(feat, 0, (size_t)Mp * F * 4, st));
        if (mel) {
            LogmelParams lp{};
            lp.wavs = d_ptr;
            lp.lens = d_len;
            lp.counts = d_cnt;
            lp.B = B;
            lp.max_len = n_max;
            lp.n_mels = x.n_mels;
            lp.target_level = x.target_level;
            lp.cmvn = x.cmvn;
            lp.scale = scale;
            lp.sig = sig;
            lp.spec = spec;
            lp.out = feat;
            lp.o_bs = Tp * F;
            HIP_TRY(launch_logmel(lp, st));
        } else {
            const s3::FbankParams fp = mj_fbank_params(x);
            for (int b = 0; b < B; ++b) HIP_TRY(s3::launch_fbank(fp, wav_ptrs_host[b], lengths[b], feat + (size_t)b * Tp * F, F, st));
        }
    }

    // ---- input representation: state 0 ----
    HIP_TRY(linear_f32(e, st, {"gemm:mj_in", feat, w.in_w.p, w.in_b.p, Mp, D, F, 0, nullptr, tmp}));
    HIP_TRY(ln(tmp, (const float*)w.pos.p, w.in_g, w.in_beta, xa, 0));
    if (state_done(0)) return 1;

    // ---- post-LN BERT layers over B * n sequences of Tc rows ----
    for (int l = 0; l < NL; ++l) {
        const LayerW& L = w.layers[x.share_layer ? 0 : l];
        HIP_TRY(linear_f32(e, st, {"gemm:qkv", xa, L.wqkv.p, L.bqkv.p, Mp, 3 * D, D, 0, nullptr, qkv}));
        {
            AttnParams a{};
            a.qkv = qkv;
            a.out = ctx;
            a.valid = d_kv;
            a.B = (int)NS;
            a.T = (int)Tc;
            a.H = H;
            Prof pr(e, st, "attention", 4.0 * NS * H * Tc * Tc * 64, 4.0 * Mp * D * 4);
            HIP_TRY(launch_attention(F32, a, st));
        }
        HIP_TRY(linear_f32(e, st, {"gemm:out_proj", ctx, L.wo.p, L.bo.p, Mp, D, D, 0, xa, tmp}));
        HIP_TRY(ln(tmp, nullptr, L.ln1g, L.ln1b, xb, -1));
        HIP_TRY(linear_f32(e, st, {"gemm:fc1", xb, L.w1.p, L.b1.p, Mp, FF, D, 1, nullptr, hbuf}));
        HIP_TRY(linear_f32(e, st, {"gemm:fc2", hbuf, L.w2.p, L.b2.p, Mp, D, FF, 0, xb, tmp}));
        HIP_TRY(ln(tmp, nullptr, L.ln2g, L.ln2b, xa, l + 1));
        if (state_done(l + 1)) return 1;
    }
    return 0;
}


// frames: the stand-alone count; inside a batch the mel front end's CMVN makes the valid count batch-dependent (mj_valid_frames)
FamilyOps kMockingjayFamily = {
    S3ENC_MOCKINGJAY, "mockingjay", "S3ENC_MOCKINGJAY", "s3enc_create_mockingjay",
    "the Mockingjay / TERA / AudioALBERT family needs its front-end block", "Mockingjay / TERA / AudioALBERT (one hidden_states list)",
    [](const s3enc_config& c, const void* b) { return mj_check_config(c, *(const s3enc_mockingjay_config*)b); },
    [](s3enc_encoder* e, const Ckpt& ck, const void* b) { e->mj_cfg = *(const s3enc_mockingjay_config*)b; return mj_create(e, ck); },
    mj_forward,
    [](const s3enc_encoder* h, long n) { return mj_num_frames(h->cfg, h->mj_cfg, n); },
    [](const s3enc_encoder* h, long length, long n_max) { return mj_valid_frames(h->cfg, h->mj_cfg, length, n_max); }};

}  // namespace s3e
