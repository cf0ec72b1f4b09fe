// engine.hip — the C ABI of libs3enc (include/s3enc.h): handle, weight packer, workspace, forward schedule.
//
// Forward schedule (all launches on the caller's stream, no host synchronisation inside):
//   table upload -> wav stats -> [GroupNorm lag sums] -> conv0 -> conv1..6 (implicit GEMM, GELU fused)
//   -> LayerNorm(C) -> post_extract_proj (+bias, padded frames zeroed) -> pos-conv (+GELU, +residual)
//   -> [post-LN: encoder.layer_norm] -> NL x { q|k|v GEMM, attention, out_proj(+residual), LN, fc1(+GELU),
//   fc2(+residual), LN }  with every hidden-state tap written straight into the caller's (NL+1, B, T, D) slab.
//   (multires-HuBERT continues in multires.hip after post_extract_proj; the single-kernel entry points are in ops.hip)
#include "engine_internal.h"
#include "spectral.h"

namespace s3e {

thread_local std::string g_err;

long conv_len(const s3enc_config& c, long n, int upto /*exclusive*/) {
    for (int i = 0; i < upto; ++i) n = n >= c.conv_kernel[i] ? (n - c.conv_kernel[i]) / c.conv_stride[i] + 1 : 0;
    if (c.family == S3ENC_DECOAR2 && upto >= c.n_conv) n = (n + 1) / 2;  // y[::2] behind the fbank frames (decoar2/audio.py:84)
    return n;
}

int valid_frames(const s3enc_config& c, long length, long n_max) {
    const long T = conv_len(c, n_max, c.n_conv);
    if (T <= 0) return 0;
    long v;
    if (c.family == S3ENC_WAV2VEC2 || c.family == S3ENC_DISTILLER || c.family == S3ENC_WAV2VEC || c.family == S3ENC_APC || c.family == S3ENC_NPC ||
        c.family == S3ENC_DECOAR2) {
        // wav2vec2_model.py:2652-2669; distiller/model.py:271-285; wav2vec has no mask: the frames an utterance's own samples reach;
        // APC: the utterance's own whole analysis windows (its packed length); DeCoAR 2.0: every second one of them (decoar2/expert.py:86-94)
        v = conv_len(c, length, c.n_conv);
    } else {
        const long chunk = n_max / T;  // hubert_model.py:454-464
        v = (length + chunk - 1) / chunk;
    }
    if (v > T) v = T;
    if (v < 0) v = 0;
    return (int)v;
}
int num_states(const s3enc_config& c, int selection) {
    if (c.family == S3ENC_MULTIRES) return c.encoder_layers + 2 * c.mr_pairs + 1;  // per block: layer inputs + its output
    if (selection == S3ENC_SEL_HIDDEN) return c.encoder_layers + 1 + (c.family == S3ENC_DISTILLER ? c.pred_heads : 0);
    return c.encoder_layers;
}

// ---- the plumbing every family shares (engine_internal.h) ----------------------------------------------------------------------------
int Ckpt::get(const std::string& name, long expect, std::vector<float>& out) const {
    auto it = m.find(name);
    if (it == m.end()) return fail("checkpoint is missing tensor '" + name + "'");
    long n = 1;
    for (int i = 0; i < it->second->ndim; ++i) n *= it->second->shape[i];
    if (n != expect) return fail("tensor '" + name + "' has " + std::to_string(n) + " elements, expected " + std::to_string(expect));
    out.assign(it->second->data, it->second->data + expect);
    return 0;
}

void tap_major(const std::vector<float>& t, int cout, int cin, int k, std::vector<float>& o) {
    o.resize(t.size());
    for (int co = 0; co < cout; ++co)
        for (int ci = 0; ci < cin; ++ci)
            for (int j = 0; j < k; ++j) o[((long)co * k + j) * cin + ci] = t[((long)co * cin + ci) * k + j];
}

void pack_conv_f22(const std::vector<float>& t, int C, std::vector<float>& w, std::vector<float>& wp) {
    tap_major(t, C, C, 3, w);
    wp.resize((size_t)C * C);
    for (int co = 0; co < C; ++co)
        for (int ci = 0; ci < C; ++ci) wp[(size_t)co * C + ci] = w[(long)co * 3 * C + ci] + w[(long)co * 3 * C + 2 * C + ci];
}

int load_rnn_layer(const Ckpt& ck, const std::string& prefix, const std::string& suffix, int G, int H, int I, RnnW& w) {
    std::vector<float> t, t2;
    w.w_ih.emplace_back();
    w.w_hh.emplace_back();
    w.b_pre.emplace_back();
    w.b_hn.emplace_back();
    GET(prefix + "weight_ih" + suffix, (long)G * H * I, t);
    UP(upload_f32(w.w_ih.back(), t));
    GET(prefix + "weight_hh" + suffix, (long)G * H * H, t);
    pack_rnn_whh(t.data(), G, H, t2);
    UP(upload_f32(w.w_hh.back(), t2));
    GET(prefix + "bias_ih" + suffix, (long)G * H, t);
    GET(prefix + "bias_hh" + suffix, (long)G * H, t2);
    // the input projection's bias: b_ih plus the part of b_hh outside a product — all of it for an LSTM, the r and z parts for
    // a GRU (b_hn stays inside r * (W_hn h + b_hn))
    const int fold = G == 4 ? G * H : 2 * H;
    for (int i = 0; i < fold; ++i) t[i] += t2[i];
    UP(upload_f32(w.b_pre.back(), t));
    if (G == 3) {
        t.assign(t2.begin() + 2 * H, t2.end());
        UP(upload_f32(w.b_hn.back(), t));
    }
    return 0;
}

int batch_n_max(const float* const* wav_ptrs_host, const int64_t* lengths, int32_t B, int64_t n_max_in, long& n_max) {
    if (B <= 0) return fail("s3enc_forward: B must be positive");
    n_max = 0;
    for (int b = 0; b < B; ++b) {
        if (lengths[b] <= 0) return fail("s3enc_forward: empty utterance");
        if (lengths[b] > n_max) n_max = lengths[b];
        if (!wav_ptrs_host[b]) return fail("s3enc_forward: null waveform pointer");
    }
    if (n_max_in > 0) {
        if (n_max_in < n_max) return fail("s3enc_forward: n_max is smaller than the longest utterance");
        n_max = n_max_in;
    }
    return 0;
}

int check_out(const void* out, const FwdOpts& fo, int64_t layer_stride, long min_stride) {
    if (!out) return fail("s3enc_forward: null output");
    if (!fo.featurize) {
        if (layer_stride < min_stride) return fail("s3enc_forward: layer_stride < B*T*D");
        if (layer_stride & 3) return fail("s3enc_forward: layer_stride must be a multiple of 4 elements (vector stores)");
    }
    if ((uintptr_t)out & 15) return fail("s3enc_forward: out must be 16-byte aligned");
    return 0;
}

int stage_begin(s3enc_encoder* e, size_t bytes, hipStream_t st, char*& hp) {
    if (bytes > e->slot_bytes) {
        HIP_TRY(hipStreamSynchronize(st));
        if (e->pinned) HIP_TRY(hipHostFree(e->pinned));
        e->pinned = nullptr;
        e->slot_bytes = bytes * 4 + 4096;
        HIP_TRY(hipHostMalloc(&e->pinned, e->slot_bytes * s3enc_encoder::RING, hipHostMallocDefault));
    }
    const int slot = e->slot_next;
    e->slot_next = (slot + 1) % s3enc_encoder::RING;
    HIP_TRY(hipEventSynchronize(e->slot_ev[slot]));
    hp = (char*)e->pinned + (size_t)slot * e->slot_bytes;
    return 0;
}
int stage_commit(s3enc_encoder* e, const char* hp, void* dst, size_t bytes, hipStream_t st) {
    HIP_TRY(hipMemcpyAsync(dst, hp, bytes, hipMemcpyHostToDevice, st));
    HIP_TRY(hipEventRecord(e->slot_ev[(hp - (const char*)e->pinned) / e->slot_bytes], st));
    return 0;
}
}  // namespace s3e

namespace {

// The families that come with a second configuration block (FamilyOps, engine_internal.h), in the order their entries were added:
// the one list of them the engine has.
const FamilyOps* const kFamilies[] = {&kWav2vecFamily, &kCpcFamily,    &kApcFamily,   &kMockingjayFamily, &kDecoarFamily,
                                      &kNpcFamily,     &kVggishFamily, &kByolAFamily, &kMaeAstFamily,     &kByolSFamily,
                                      &kSsastFamily};
// DeCoAR 2.0's front end, the family's own constants (decoar2/audio.py:8-9,70-76, kaldi.fbank's defaults; CMVN eps :16)
s3::FbankParams decoar2_fbank_params() {
    s3::FbankParams f;
    f.sample_rate = 16000;
    f.num_mel_bins = 80;
    f.frame_length_ms = 25.f;
    f.frame_shift_ms = 10.f;
    f.preemph = 0.97f;
    f.delta_order = 0;
    f.use_cmvn = 1;
    f.cmvn_eps = 1e-10f;
    f.window = 1;  // hamming: the reference's WINDOW_TYPE
    return f;
}

const FamilyOps* family_ops(int family) {  // null: a Transformer family
    for (const FamilyOps* f : kFamilies)
        if (f->family == family) return f;
    return nullptr;
}

// WavLM bucket table (wavlm/modules.py:418-462): table[h][rel + R] = E[bucket(rel)][h] for rel = key - query in [-R, R]
void build_rel_table(const s3enc_config& c, const std::vector<float>& emb, int R, std::vector<float>& table) {
    const int H = c.heads, nb = c.num_buckets / 2, max_exact = nb / 2;
    const int W = 2 * R + 1;
    table.resize((size_t)H * W);
    const float denom = (float)std::log((double)c.max_distance / (double)max_exact);
    for (int idx = 0; idx < W; ++idx) {
        const int rel = idx - R;
        int bucket = rel > 0 ? nb : 0;
        const int a = rel < 0 ? -rel : rel;
        if (a < max_exact) {
            bucket += a;
        } else {
            float v = std::log((float)a / (float)max_exact);
            v = v / denom;
            v = v * (float)(nb - max_exact);
            int large = max_exact + (int)v;
            if (large > nb - 1) large = nb - 1;
            bucket += large;
        }
        for (int h = 0; h < H; ++h) table[(size_t)h * W + idx] = emb[(size_t)bucket * H + h];
    }
}

int check_config(const s3enc_config& c) {
    if (c.family < 0 || c.family > S3ENC_SSAST || c.family == S3ENC_DECOAR2 + 1) return fail("config: unknown family");  // (17 is not assigned)
    if (family_ops(c.family)) return 0;  // its record's own check runs on both configuration blocks (create_impl)
    if (c.family == S3ENC_MULTIRES) {
        if (c.mr_pairs < 1 || c.mr_pairs > S3ENC_MAX_RES - 1) return fail("config: mr_pairs out of range");
        const int k = c.mr_kernel;
        if (k < 1 || k > 15 || !(k & 1)) return fail("config: mr_kernel must be odd and <= 15");
        int total = 0;
        for (int i = 0; i < 2 * c.mr_pairs + 1; ++i) {
            if (c.mr_layers[i] < 1) return fail("config: every multires block needs at least one layer");
            total += c.mr_layers[i];
        }
        if (total != c.encoder_layers) return fail("config: encoder_layers must equal the sum of mr_layers");
        for (int i = 0; i < 2 * c.mr_pairs; ++i) {
            const int r = c.mr_ratios[i];
            if (r < 1 || r > 4 || (k - 1) % r) return fail("config: every multires rate must divide mr_kernel - 1");
            if (c.mr_plain && !(i & 1) && r != 1) return fail("config: mr_plain needs rate pairs of the form (1, d)");
        }
        if (c.rel_pos || c.pred_heads || c.pos_conv_depth > 1 || c.no_feature_layer_norm)
            return fail("config: multires-HuBERT takes none of the WavLM / DistilHuBERT / data2vec options");
    }
    if (c.pred_heads < 0 || c.pred_heads > 16) return fail("config: pred_heads out of range");
    if (c.pred_heads && c.family != S3ENC_DISTILLER) return fail("config: pred_heads is a DistilHuBERT feature");
    const bool d2 = c.family == S3ENC_DECOAR2;  // no conv extractor: the kaldi front end's constants in the conv fields
    if (d2) {
        if (c.n_conv != 1 || c.conv_kernel[0] != 400 || c.conv_stride[0] != 160 || c.conv_dim != 80)
            return fail("config: DeCoAR 2.0 carries its front end as n_conv = 1, conv_kernel[0] / conv_stride[0] = 400 / 160 samples and conv_dim = 80 mel bins");
        if (c.layer_norm_first) return fail("config: DeCoAR 2.0 with layer_norm_first is not built");
        if (c.pos_conv_depth > 1) return fail("config: DeCoAR 2.0 with pos_conv_depth > 1 is not built");
        if (c.layer_type || c.rel_pos || c.pred_heads || c.no_feature_layer_norm)
            return fail("config: DeCoAR 2.0 takes none of the Conformer / WavLM / DistilHuBERT options");
        if (c.extractor_layer_norm || c.conv_bias || c.normalize)
            return fail("config: DeCoAR 2.0 has no conv extractor and no waveform normalisation (extractor_layer_norm, conv_bias and normalize must be 0)");
    }
    if (!d2 && (c.n_conv < 2 || c.n_conv > S3ENC_MAX_CONV)) return fail("config: n_conv out of range");
    if (!d2 && c.conv_kernel[0] != 10) return fail("config: the conv0 kernel is specialised for kernel width 10");
    if (!d2 && (c.conv_dim % 32 || c.conv_dim > 1024)) return fail("config: conv_dim must be a multiple of 32, <= 1024");
    if (c.heads <= 0 || c.embed_dim != c.heads * 64) return fail("config: head_dim must be 64");
    if (c.ffn_dim % 8) return fail("config: ffn_dim must be a multiple of 8");
    if (c.conv_pos_groups <= 0 || c.embed_dim % c.conv_pos_groups) return fail("config: embed_dim % conv_pos_groups != 0");
    const int dg = c.embed_dim / c.conv_pos_groups;
    if (dg != 24 && dg != 32 && dg != 40 && dg != 48 && dg != 64) return fail("config: embed_dim/conv_pos_groups must be 32, 48 or 64 (fp32: also 24 or 40)");
    if (c.conv_pos < 1 || c.conv_pos > 256) return fail("config: conv_pos out of range");
    if (c.compute_dtype < 0 || c.compute_dtype > 4) return fail("config: unknown compute_dtype");
    static const char* const kModes[] = {"fp32", "bf16", "fp16", "fp32x3", "fp16x2"};
    if ((dg == 24 || dg == 40) && c.compute_dtype != S3ENC_F32)
        return fail(std::string("config: the positional conv at group width ") + std::to_string(dg) + " is built for compute dtype fp32 only; " +
                    kModes[c.compute_dtype] + " is not built");
    if (c.family == S3ENC_LIGHTHUBERT) {
        if (c.compute_dtype != S3ENC_F32)
            return fail(std::string("config: LightHuBERT is built for compute dtype fp32 only; ") + kModes[c.compute_dtype] + " is not built");
        if (c.layer_norm_first) return fail("config: LightHuBERT with layer_norm_first is not built");
        if (c.pos_conv_depth > 1) return fail("config: LightHuBERT with pos_conv_depth > 1 is not built");
        if (c.layer_type || c.rel_pos || c.pred_heads || c.no_feature_layer_norm)
            return fail("config: LightHuBERT takes none of the Conformer / WavLM / DistilHuBERT options");
    }
    if (c.encoder_layers < 1) return fail("config: encoder_layers < 1");
    if (c.rel_pos && c.family != S3ENC_WAVLM) return fail("config: rel_pos is a WavLM feature");
    if (c.rel_pos && (c.num_buckets < 4 || c.max_distance <= c.num_buckets / 4))
        return fail("config: bad num_buckets / max_distance");
    if (c.rel_pos && c.max_distance > 8192) return fail("config: max_distance > 8192");
    if (c.pos_conv_depth < 0 || c.pos_conv_depth > 16) return fail("config: pos_conv_depth out of range");
    if (!(c.wav_norm_eps >= 0.f) || c.wav_norm_eps > 1.f) return fail("config: wav_norm_eps out of range");
    if (c.pos_conv_depth > 1 && c.family != S3ENC_WAV2VEC2) return fail("config: pos_conv_depth > 1 is the data2vec-audio encoder (wav2vec2 family)");
    if (c.layer_type < 0 || c.layer_type > 1) return fail("config: unknown layer_type (0 transformer, 1 conformer)");
    if (c.layer_type == 1) {
        if (c.family != S3ENC_WAV2VEC2 || c.pos_conv_depth > 1) return fail("config: conformer layers are a wav2vec2-family encoder");
        if (c.pos_enc_type != 1 && c.pos_enc_type != 2) return fail("config: conformer pos_enc_type must be 1 (rel_pos) or 2 (rope)");
        if (c.dw_kernel < 1 || c.dw_kernel > 63 || !(c.dw_kernel & 1)) return fail("config: conformer dw_kernel must be odd and <= 63");
        if (c.compute_dtype != S3ENC_F32)
            return fail(std::string("config: conformer layers (") + (c.pos_enc_type == 1 ? "rel_pos" : "rope") +
                        ") are built for compute dtype fp32 only; " +
                        (c.compute_dtype == 1 ? "bf16" : c.compute_dtype == 2 ? "fp16" : c.compute_dtype == 3 ? "fp32x3" : "fp16x2") +
                        " is not built");
    }
    return 0;
}
}  // namespace

// the handle's own device state behind the weights: staging-ring events and the status word of s3enc_forward_status
static int finish_create(std::unique_ptr<s3enc_encoder> e, s3enc_handle* out) {
    for (int i = 0; i < s3enc_encoder::RING; ++i)
        if (hipEventCreateWithFlags(&e->slot_ev[i], hipEventDisableTiming) != hipSuccess) return fail("hipEventCreate failed");
    // the status word of s3enc_forward_status: device int + pinned host copy + the event behind the copy
    bool st_ok = e->status_dev.ensure(64) == hipSuccess && hipMemset(e->status_dev.p, 0, 64) == hipSuccess &&
                 hipHostMalloc((void**)&e->status_host, s3enc_encoder::STATUS_RING * sizeof(int), hipHostMallocDefault) == hipSuccess;
    for (int i = 0; st_ok && i < s3enc_encoder::STATUS_RING; ++i)
        st_ok = hipEventCreateWithFlags(&e->status_ev[i], hipEventDisableTiming) == hipSuccess;
    if (!st_ok) return fail("s3enc_create: status word allocation failed");
    *out = e.release();
    return 0;
}

// Each family of kFamilies comes through the entry point that takes its block.  `own`: the family whose block the calling entry
// takes (-1: none).  An entry refuses the families whose entry was added after it by name (`entry` prefixes those refusals), and
// any other family than its own as not its block's.
static int wrong_entry(const char* entry, int own, int family) {
    if (family == own) return 0;
    for (const FamilyOps* f : kFamilies)
        if (f->family == family && family > own) return fail(std::string(entry) + ": " + f->needs + ": use " + f->entry);
    for (const FamilyOps* f : kFamilies)
        if (f->family == own) return fail(std::string(f->entry) + ": the " + f->block + " block belongs to family " + f->name + " only");
    return 0;
}

static int create_impl(const s3enc_config* cfg, int own, const void* block, const s3enc_tensor* tensors, int32_t n_tensors, int32_t device,
                       s3enc_handle* out);

// an entry whose block is required: s3enc_create_cpc and every later one
static int create_family(const FamilyOps& f, const s3enc_config* cfg, const void* block, const s3enc_tensor* tensors, int32_t n_tensors,
                         int32_t device, s3enc_handle* out) {
    if (!cfg || !block || !tensors || !out) return fail(std::string(f.entry) + ": null argument");
    *out = nullptr;
    if (wrong_entry(f.entry, f.family, cfg->family)) return 1;
    return create_impl(cfg, f.family, block, tensors, n_tensors, device, out);
}

extern "C" {

int s3enc_version(void) { return S3ENC_VERSION; }
const char* s3enc_last_error(void) { return g_err.c_str(); }

int s3enc_create(const s3enc_config* cfg, const s3enc_tensor* tensors, int32_t n_tensors, int32_t device, s3enc_handle* out) {
    return s3enc_create_ex(cfg, nullptr, tensors, n_tensors, device, out);
}

int s3enc_create_ex(const s3enc_config* cfg, const s3enc_wav2vec_config* w2v, const s3enc_tensor* tensors, int32_t n_tensors,
                    int32_t device, s3enc_handle* out) {
    if (cfg && cfg->family > S3ENC_WAV2VEC && wrong_entry("s3enc_create", -1, cfg->family)) {  // a later family: needs its own entry
        if (out) *out = nullptr;
        return 1;
    }
    return create_impl(cfg, w2v ? S3ENC_WAV2VEC : -1, w2v, tensors, n_tensors, device, out);
}

int s3enc_create_cpc(const s3enc_config* cfg, const s3enc_cpc_config* cpc, const s3enc_tensor* tensors, int32_t n_tensors,
                     int32_t device, s3enc_handle* out) {
    return create_family(kCpcFamily, cfg, cpc, tensors, n_tensors, device, out);
}
int s3enc_create_apc(const s3enc_config* cfg, const s3enc_apc_config* apc, const s3enc_tensor* tensors, int32_t n_tensors,
                     int32_t device, s3enc_handle* out) {
    return create_family(kApcFamily, cfg, apc, tensors, n_tensors, device, out);
}
int s3enc_create_mockingjay(const s3enc_config* cfg, const s3enc_mockingjay_config* mj, const s3enc_tensor* tensors, int32_t n_tensors,
                            int32_t device, s3enc_handle* out) {
    return create_family(kMockingjayFamily, cfg, mj, tensors, n_tensors, device, out);
}
int s3enc_create_decoar(const s3enc_config* cfg, const s3enc_decoar_config* decoar, const s3enc_tensor* tensors, int32_t n_tensors,
                        int32_t device, s3enc_handle* out) {
    return create_family(kDecoarFamily, cfg, decoar, tensors, n_tensors, device, out);
}
int s3enc_create_npc(const s3enc_config* cfg, const s3enc_npc_config* npc, const s3enc_tensor* tensors, int32_t n_tensors,
                     int32_t device, s3enc_handle* out) {
    return create_family(kNpcFamily, cfg, npc, tensors, n_tensors, device, out);
}
int s3enc_create_vggish(const s3enc_config* cfg, const s3enc_vggish_config* vggish, const s3enc_tensor* tensors, int32_t n_tensors,
                        int32_t device, s3enc_handle* out) {
    return create_family(kVggishFamily, cfg, vggish, tensors, n_tensors, device, out);
}
int s3enc_create_byol_a(const s3enc_config* cfg, const s3enc_byol_a_config* byol_a, const s3enc_tensor* tensors, int32_t n_tensors,
                        int32_t device, s3enc_handle* out) {
    return create_family(kByolAFamily, cfg, byol_a, tensors, n_tensors, device, out);
}
int s3enc_create_mae_ast(const s3enc_config* cfg, const s3enc_mae_ast_config* mae_ast, const s3enc_tensor* tensors, int32_t n_tensors,
                         int32_t device, s3enc_handle* out) {
    return create_family(kMaeAstFamily, cfg, mae_ast, tensors, n_tensors, device, out);
}
int s3enc_create_byol_s(const s3enc_config* cfg, const s3enc_byol_s_config* byol_s, const s3enc_tensor* tensors, int32_t n_tensors,
                        int32_t device, s3enc_handle* out) {
    return create_family(kByolSFamily, cfg, byol_s, tensors, n_tensors, device, out);
}
int s3enc_create_ssast(const s3enc_config* cfg, const s3enc_ssast_config* ssast, const s3enc_tensor* tensors, int32_t n_tensors,
                       int32_t device, s3enc_handle* out) {
    return create_family(kSsastFamily, cfg, ssast, tensors, n_tensors, device, out);
}

static int create_impl(const s3enc_config* cfg, int own, const void* block, const s3enc_tensor* tensors, int32_t n_tensors, int32_t device,
                       s3enc_handle* out) {
    if (!cfg || !tensors || !out) return fail("s3enc_create: null argument");
    *out = nullptr;
    if (check_config(*cfg)) return 1;
    // s3enc_create_ex: a wav2vec block with another family, the wav2vec family without its block (a later entry comes with own == family)
    if (wrong_entry("s3enc_create", own, cfg->family)) return 1;
    const FamilyOps* ops = family_ops(cfg->family);  // (non-null: the entry points have refused the family that came without its block)
    if (ops && ops->check(*cfg, block)) return 1;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail("s3enc_create: no HIP device visible — libs3enc has no CPU fallback");
    if (device < 0 || device >= ndev) return fail("s3enc_create: device index out of range");
    DeviceGuard dg(device);
    if (!dg.ok) return fail("s3enc_create: hipSetDevice failed");
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(std::string("s3enc_create: kernels are built for gfx950 only, device is ") + prop.gcnArchName);

    const Ckpt ck(tensors, n_tensors);
    std::unique_ptr<s3enc_encoder> e(new s3enc_encoder());  // (freed on every failing path below)
    e->cfg = *cfg;
    e->device = device;
    e->x3 = cfg->compute_dtype == 3;  // S3ENC_F32X3: the fp32 data flow, GEMMs through gemm_x3.hip
    e->x2 = cfg->compute_dtype == 4;  // S3ENC_F16X2: the fp16 data flow, GEMM weights split into two fp16 terms
    e->dtype = e->x3 ? (int)F32 : (e->x2 ? (int)F16 : cfg->compute_dtype);
    e->es = e->dtype == F32 ? 4 : 2;
    e->ops = ops;
    if (ops) return ops->create(e.get(), ck, block) ? 1 : finish_create(std::move(e), out);
    const s3enc_config& c = e->cfg;  // the Transformer families: their weights are packed here
    const int C = c.conv_dim, D = c.embed_dim, F = c.ffn_dim, H = c.heads;
    const bool multires = c.family == S3ENC_MULTIRES;
    const std::string enc0 = multires ? "encoders.0" : "encoder";  // only the first block keeps its positional conv
    std::vector<float> t, t2;

    // ---- conv feature extractor ----
    // (round 5: layer-norm extractors too — their conv outputs are LayerNorm'd + GELU'd, which renormalises the scale but not the
    // relative rounding noise: six stacked fp16 roundings are 6.0e-4 on HuBERT-large and, amplified by the bias-sharpened
    // attention of WavLM-large, 1.07e-3 alone on pretrained-like statistics — tools/fp16_error_budget.py, profiles/r05_fp16_cliff.md)
    if (e->x2 && !c.no_feature_layer_norm && c.n_conv >= 3) {
        bool ok = true;  // every conv from the second on must be a shape the three-term GEMM takes
        for (int i = 2; i < c.n_conv; ++i) ok = ok && x3_shape_ok(C, (long)c.conv_kernel[i] * C, (long)c.conv_stride[i] * C);
        if (ok) e->x2_conv_f32_from = 2;
        // round 6, tuning key fp16x2_conv1_f32 (read here): conv0 writes fp32 and conv1 — half of the conv stack's FLOPs — takes the
        // three-term GEMM as well.  What is left of the conv term after the hybrid above is conv0's own fp16 output (the largest single
        // site on the worst seed of the weight-seed sweep after the LayerNorm outputs: WavLM-large seed 1, 8.3e-4 -> 7.2e-4 emulated,
        // profiles/r06_parity_seeds.md); it costs conv1 at the three-term rate on fp32 rows — opt-in, the default stays inside 1e-3.
        if (ok && tuning().fp16x2_conv1_f32 && x3_shape_ok(C, (long)c.conv_kernel[1] * C, (long)c.conv_stride[1] * C)) e->x2_conv_f32_from = 1;
    }
    const bool d2 = c.family == S3ENC_DECOAR2;  // the kaldi front end has no weights
    e->conv.resize(c.n_conv);
    for (int i = 0; i < c.n_conv && !d2; ++i) {
        const std::string p = "feature_extractor.conv_layers." + std::to_string(i);
        const int cin = i == 0 ? 1 : C, k = c.conv_kernel[i];
        GET(p + ".0.weight", (long)C * cin * k, t);
        if (i == 0) {
            UP(upload_f32(e->conv[i].w, t));  // [C][k]
        } else {
            const bool f22 = e->dtype == F32 && !e->x3 && k == 3 && c.conv_stride[i] == 2;  // convf22.hip's WP = fl(W0 + W2)
            std::vector<float> wp;
            if (f22) pack_conv_f22(t, C, t2, wp);  // (cin = C from conv1 on; t2 is tap_major's image)
            else tap_major(t, C, cin, k, t2);  // W'[co][j*Cin + ci], the K order of the channel-last implicit GEMM
            if (e->x2_conv_f32_from && i >= e->x2_conv_f32_from) {
                UP(upload_gemm_w(e->conv[i].w, t2, C, (long)k * cin, e->dtype, e->x2));  // (read only if the three-term path declines)
            } else {
                UP(upload_gemm_w_mx(e.get(), e->conv[i].w, t2, C, (long)k * cin, 1));
            }
            if (e->x3 || (e->x2_conv_f32_from && i >= e->x2_conv_f32_from)) UP(upload_x3(e->conv[i].w3, t2, C, (long)k * cin));
            if (f22) UP(upload_f32(e->conv[i].wp, wp));
        }
        if (c.conv_bias) {
            GET(p + ".0.bias", C, t);
            UP(upload_f32(e->conv[i].bias, t));
            e->conv[i].has_bias = true;
        }
        if (c.extractor_layer_norm) {
            GET(p + ".2.1.weight", C, t);
            UP(upload_f32(e->conv[i].lng, t));
            GET(p + ".2.1.bias", C, t);
            UP(upload_f32(e->conv[i].lnb, t));
        } else if (i == 0) {
            GET(p + ".2.weight", C, t);
            UP(upload_f32(e->gn_g, t));
            GET(p + ".2.bias", C, t);
            UP(upload_f32(e->gn_b, t));
        }
    }
    if (!c.no_feature_layer_norm && !d2) {
        GET("layer_norm.weight", C, t);
        UP(upload_f32(e->fln_g, t));
        GET("layer_norm.bias", C, t);
        UP(upload_f32(e->fln_b, t));
    }
    GET("post_extract_proj.weight", (long)D * C, t);
    if (d2) {  // K = 80 on the CMVN's output, the model's input: exact fp32 in every operand mode
        UP(upload_f32(e->proj_w, t));
    } else {
        UP(upload_gemm_w(e->proj_w, t, D, C, e->dtype, e->x2));
        e->x2_proj_f32 = e->x2 && !c.no_feature_layer_norm && c.family != S3ENC_DISTILLER && x3_shape_ok(D, C, C);
        if (e->x3 || e->x2_proj_f32) UP(upload_x3(e->proj_w3, t, D, C));
    }
    GET("post_extract_proj.bias", D, t);
    UP(upload_f32(e->proj_b, t));

    // ---- positional conv: fold weight_norm(dim=2), then pack for the kernel of the compute dtype ----
    // (a Conformer encoder never calls its pos_conv, ConformerEncoder.extract_features: the checkpoint's weights are ignored)
    const bool conf = c.layer_type == 1;
    if (conf) {
    } else if (c.pos_conv_depth > 1) {
        // data2vec (wav2vec2_model.py:2995-3023): plain grouped convs of width max(3, conv_pos / depth), no weight_norm
        const int G = c.conv_pos_groups, Dg = D / G;
        int k = c.conv_pos / c.pos_conv_depth;
        k = k < 3 ? 3 : k;
        const bool k16 = e->dtype != F32 || e->x3;  // the implicit-GEMM kernel: even K with K * Dg a multiple of 128
        int kp = k;
        if (k16)
            while ((kp & 1) || ((long)kp * Dg) % 128) ++kp;
        e->pos_k = kp;
        e->pos_pad = k / 2;
        e->pos_ws.resize(c.pos_conv_depth);
        e->pos_bs.resize(c.pos_conv_depth);
        for (int i = 0; i < c.pos_conv_depth; ++i) {
            const std::string p = "encoder.pos_conv." + std::to_string(i) + ".0";
            std::vector<float> w, wp((size_t)D * Dg * kp, 0.f);
            GET(p + ".weight", (long)D * Dg * k, w);
            for (long r = 0; r < (long)D * Dg; ++r)
                for (int j = 0; j < k; ++j) wp[r * kp + j] = w[r * k + j];
            if (e->x3) {
                UP(upload_posconv_x3(e->pos_ws[i], wp, D, G, kp));
            } else {
                pack_posconv(wp, D, G, kp, e->dtype, t2);
                UP(upload_cvt(e->pos_ws[i], t2, e->dtype));
            }
            GET(p + ".bias", D, t);
            UP(upload_f32(e->pos_bs[i], t));
        }
        UP(upload_f32(e->ones, std::vector<float>(D, 1.f)));
        UP(upload_f32(e->zeros, std::vector<float>(D, 0.f)));
    } else {
        const int K = c.conv_pos, G = c.conv_pos_groups, Dg = D / G;
        std::vector<float> g, v;
        if (c.family == S3ENC_LIGHTHUBERT) {
            // the weight-norm runs over the UNSLICED supernet tensor (768 x 48 entries per tap), so only the binder can fold it:
            // the sliced, folded filters arrive as a plain conv weight (s3enc.h: S3ENC_LIGHTHUBERT)
            GET(enc0 + ".pos_conv.0.weight", (long)D * Dg * K, v);
        } else {
            GET(enc0 + ".pos_conv.0.weight_g", K, g);
            GET(enc0 + ".pos_conv.0.weight_v", (long)D * Dg * K, v);
            std::vector<double> nrm(K, 0.0);
            for (long i = 0; i < (long)D * Dg; ++i)
                for (int k = 0; k < K; ++k) nrm[k] += (double)v[i * K + k] * v[i * K + k];
            for (int k = 0; k < K; ++k) nrm[k] = (double)g[k] / std::sqrt(nrm[k]);
            for (long i = 0; i < (long)D * Dg; ++i)
                for (int k = 0; k < K; ++k) v[i * K + k] = (float)(v[i * K + k] * nrm[k]);
        }
        // the 16-bit / split-precision implicit GEMM wants an even tap count with K * Dg a multiple of 128: append zero
        // taps (the real kernel keeps its K / 2 left padding), as for the data2vec stack above
        int kp = K;
        if (e->dtype != F32 || e->x3)
            while ((kp & 1) || ((long)kp * Dg) % 128) ++kp;
        e->pos_k = kp;
        e->pos_pad = K / 2;
        if (kp != K) {
            std::vector<float> vp((size_t)D * Dg * kp, 0.f);
            for (long r = 0; r < (long)D * Dg; ++r)
                for (int j = 0; j < K; ++j) vp[r * kp + j] = v[r * K + j];
            v.swap(vp);
        }
        pack_posconv(v, D, G, kp, e->dtype, t2);
        UP(upload_cvt(e->pos_w, t2, e->dtype));
        if (e->x3) UP(upload_posconv_x3(e->pos_w3, v, D, G, kp));
        GET(enc0 + ".pos_conv.0.bias", D, t);
        UP(upload_f32(e->pos_b, t));
    }
    if (!multires) {
        GET("encoder.layer_norm.weight", D, t);
        UP(upload_f32(e->eln_g, t));
        GET("encoder.layer_norm.bias", D, t);
        UP(upload_f32(e->eln_b, t));
    }

    // ---- transformer layers ----
    // q *= head_dim^-0.5 is folded into W_q, b_q; the 16-bit attention kernels additionally want log2-domain scores
    // (attention.hip: softmax as exp2 with no per-score multiply), so those handles fold log2(e) in as well — one rounding
    // of the weight to the operand type either way.  The exact-fp32 and split-precision handles keep the power-of-two scale.
    const float qscale = (1.0f / std::sqrt((float)(D / H))) * (e->dtype != F32 ? 1.44269504088896340736f : 1.0f);
    e->x2_attn_f32 = e->x2 && !multires && x3_shape_ok(D, D, D);  // (the U-net keeps 16-bit)
    auto load = [&](const std::string& p, LayerW& L) { return load_layer(e.get(), ck, p, kFairseqLayer, qscale, c.rel_pos && c.gru_rel_pos, L); };
    // one ConformerEncoderLayer (wav2vec2_model.py:440-578) named `p`; returns non-zero after fail()
    auto load_conformer = [&](const std::string& p, ConformerLayerW& L) -> int {
        const int K = c.dw_kernel;
        auto ffn = [&](const std::string& f, DevBuf& lng, DevBuf& lnb, DevBuf& w1, DevBuf& b1, DevBuf& w2, DevBuf& b2) -> int {
            GET(f + ".layer_norm.weight", D, t);
            UP(upload_f32(lng, t));
            GET(f + ".layer_norm.bias", D, t);
            UP(upload_f32(lnb, t));
            GET(f + ".w_1.weight", (long)F * D, t);
            UP(upload_f32(w1, t));
            GET(f + ".w_1.bias", F, t);
            UP(upload_f32(b1, t));
            GET(f + ".w_2.weight", (long)D * F, t);
            for (auto& x : t) x *= 0.5f;  // x * 0.5 + residual: the half-step folded (exact)
            UP(upload_f32(w2, t));
            GET(f + ".w_2.bias", D, t);
            for (auto& x : t) x *= 0.5f;
            UP(upload_f32(b2, t));
            return 0;
        };
        if (ffn(p + ".ffn1", L.f1_lng, L.f1_lnb, L.f1_w1, L.f1_b1, L.f1_w2, L.f1_b2)) return 1;
        if (ffn(p + ".ffn2", L.f2_lng, L.f2_lnb, L.f2_w1, L.f2_b1, L.f2_w2, L.f2_b2)) return 1;
        GET(p + ".self_attn_layer_norm.weight", D, t);
        UP(upload_f32(L.at_lng, t));
        GET(p + ".self_attn_layer_norm.bias", D, t);
        UP(upload_f32(L.at_lnb, t));
        const bool relpos = c.pos_enc_type == 1;
        std::vector<float> pu, pv;
        if (relpos) {
            GET(p + ".self_attn.pos_bias_u", D, pu);
            GET(p + ".self_attn.pos_bias_v", D, pv);
        }
        const float qs = 1.0f / std::sqrt((float)(D / H));
        std::vector<float> w(3L * D * D), bb(3L * D);
        const char* names[3] = {"linear_q", "linear_k", "linear_v"};
        for (int s = 0; s < 3; ++s) {
            GET(p + ".self_attn." + names[s] + ".weight", (long)D * D, t);
            GET(p + ".self_attn." + names[s] + ".bias", D, t2);
            const float sc = s == 0 ? qs : 1.f;
            for (long i = 0; i < (long)D * D; ++i) w[(long)s * D * D + i] = t[i] * sc;
            for (int i = 0; i < D; ++i) bb[(long)s * D + i] = (s == 0 && relpos ? t2[i] + pu[i] : t2[i]) * sc;
        }
        UP(upload_f32(L.wqkv, w));
        UP(upload_f32(L.bqkv, bb));
        GET(p + ".self_attn.linear_out.weight", (long)D * D, t);
        UP(upload_f32(L.wo, t));
        GET(p + ".self_attn.linear_out.bias", D, t);
        UP(upload_f32(L.bo, t));
        if (relpos) {
            GET(p + ".self_attn.linear_pos.weight", (long)D * D, t);
            UP(upload_f32(L.wpos, t));
            for (int i = 0; i < D; ++i) t2[i] = (pv[i] - pu[i]) * qs;
            t2.resize(D);
            UP(upload_f32(L.qadd, t2));
        }
        GET(p + ".conv_module.layer_norm.weight", D, t);
        UP(upload_f32(L.cv_lng, t));
        GET(p + ".conv_module.layer_norm.bias", D, t);
        UP(upload_f32(L.cv_lnb, t));
        GET(p + ".conv_module.pointwise_conv1.weight", 2L * D * D, t);
        UP(upload_f32(L.pw1, t));
        GET(p + ".conv_module.pointwise_conv2.weight", (long)D * D, t);
        UP(upload_f32(L.pw2, t));
        std::vector<float> dw, g, bt, mu, var;
        GET(p + ".conv_module.depthwise_conv.weight", (long)D * K, dw);
        GET(p + ".conv_module.batch_norm.weight", D, g);
        GET(p + ".conv_module.batch_norm.bias", D, bt);
        GET(p + ".conv_module.batch_norm.running_mean", D, mu);
        GET(p + ".conv_module.batch_norm.running_var", D, var);
        std::vector<float> sh(D);
        for (int ch = 0; ch < D; ++ch) {  // BatchNorm1d eval (eps 1e-5): y = (x - mean) * gamma / sqrt(var + eps) + beta
            const double sc = (double)g[ch] / std::sqrt((double)var[ch] + 1e-5);
            for (int k = 0; k < K; ++k) dw[(long)ch * K + k] = (float)(dw[(long)ch * K + k] * sc);
            sh[ch] = (float)((double)bt[ch] - (double)mu[ch] * sc);
        }
        UP(upload_f32(L.taps, dw));
        UP(upload_f32(L.shift, sh));
        GET(p + ".final_layer_norm.weight", D, t);
        UP(upload_f32(L.fin_g, t));
        GET(p + ".final_layer_norm.bias", D, t);
        UP(upload_f32(L.fin_b, t));
        return 0;
    };
    if (conf) {
        e->cf_layers.resize(c.encoder_layers);
        for (int l = 0; l < c.encoder_layers; ++l)
            if (load_conformer("encoder.layers." + std::to_string(l), e->cf_layers[l])) return 1;
    } else if (!multires) {
        e->layers.resize(c.encoder_layers);
        for (int l = 0; l < c.encoder_layers; ++l)
            if (load("encoder.layers." + std::to_string(l) + ".", e->layers[l])) return 1;
    } else {
        // U-net blocks in execution order (hubert_model.py:399-507) and the conv adapters between them
        const int R = c.mr_pairs + 1, NB = 2 * R - 1, k = c.mr_kernel;
        e->mr_blocks.resize(NB);
        for (int bi = 0; bi < NB; ++bi) {
            const std::string bp = bi < R - 1 ? "encoders." + std::to_string(bi)
                                 : bi == R - 1 ? std::string("middle_encoder") : "decoders." + std::to_string(bi - R);
            BlockW& bw = e->mr_blocks[bi];
            GET(bp + ".layer_norm.weight", D, t);
            UP(upload_f32(bw.eln_g, t));
            GET(bp + ".layer_norm.bias", D, t);
            UP(upload_f32(bw.eln_b, t));
            bw.layers.resize(c.mr_layers[bi]);
            for (int l = 0; l < c.mr_layers[bi]; ++l)
                if (load(bp + ".layers." + std::to_string(l) + ".", bw.layers[l])) return 1;
        }
        // A conv over all D channels becomes a GEMM whose A rows are k_eff * D contiguous elements of a zero-bordered
        // frame buffer (kernels.h, PadCopyParams):
        //   Conv1d(D, D, k, stride s, padding (k-1)/2), weight (co, ci, j):  W'[co][j*D + ci], row t starts at frame t*s - pad
        //   ConvTranspose1d(D, D, k, stride s), weight (ci, co, j): s interleaved stride-1 convs of KT = ceil(k/s) taps —
        //     out[s*q + r] = sum_m x[q - m] . w[:, :, r + s*m]  ->  W'[r*D + co][j'*D + ci] = w[ci][co][r + s*(KT-1-j')]
        //     (0 where that tap is >= k), row q starts at frame q - (KT-1); the (Q, s*D) output IS the (s*Q, D) sequence
        auto load_conv = [&](const std::string& cp, bool transposed, int stride, AdapterConvW& cw) -> int {
            std::vector<float> w, pk;
            GET(cp + ".0.weight", (long)D * D * k, w);
            long N, K;
            if (!transposed) {
                N = D;
                K = (long)k * D;
                tap_major(w, D, D, k, pk);
            } else {
                const int KT = (k + stride - 1) / stride;
                N = (long)stride * D;
                K = (long)KT * D;
                pk.assign((size_t)N * K, 0.f);
                for (int r = 0; r < stride; ++r)
                    for (int jp = 0; jp < KT; ++jp) {
                        const int tap = r + stride * (KT - 1 - jp);
                        if (tap >= k) continue;
                        for (int co = 0; co < D; ++co)
                            for (int ci = 0; ci < D; ++ci)
                                pk[((long)r * D + co) * K + (long)jp * D + ci] = w[((long)ci * D + co) * k + tap];
                    }
            }
            UP(upload_gemm_w(cw.w, pk, N, K, e->dtype, e->x2));
            if (e->x3) UP(upload_x3(cw.w3, pk, N, K));
            GET(cp + ".2.weight", D, t);
            UP(upload_f32(cw.g, t));
            GET(cp + ".2.bias", D, t);
            UP(upload_f32(cw.b, t));
            return 0;
        };
        e->mr_adapters.resize(2 * (R - 1));
        for (int i = 0; i < R - 1; ++i) {
            const int u = c.mr_ratios[2 * i], d = c.mr_ratios[2 * i + 1];
            AdapterW& dn = e->mr_adapters[i];            // downsample_modules[i]: label_rate (u, d)
            AdapterW& upm = e->mr_adapters[R - 1 + i];   // upsample_modules[i]: the inverted pair (d, u) (:474-507)
            dn.kind = c.mr_plain ? 1 : 0;
            dn.up_rate = u;
            dn.down_rate = d;
            upm.kind = c.mr_plain ? 2 : 0;
            upm.up_rate = d;
            upm.down_rate = u;
            const std::string dp = "downsample_modules." + std::to_string(i), upp = "upsample_modules." + std::to_string(i);
            if (dn.kind != 1 && load_conv(dp + ".upsample_conv", true, dn.up_rate, dn.up)) return 1;
            if (load_conv(dp + ".downsample_conv", false, dn.down_rate, dn.down)) return 1;
            if (load_conv(upp + ".upsample_conv", true, upm.up_rate, upm.up)) return 1;
            if (upm.kind != 2 && load_conv(upp + ".downsample_conv", false, upm.down_rate, upm.down)) return 1;
        }
    }
    if (c.rel_pos) {
        // bucket(rel) (wavlm/modules.py:418-446) is constant for |rel| >= max_distance, so ONE (H, 2R+1) table with
        // R = max_distance serves every sequence length: nothing is rebuilt when T changes between batches
        std::vector<float> emb, table;
        GET("encoder.layers.0.self_attn.relative_attention_bias.weight", (long)c.num_buckets * H, emb);
        e->rel_R = c.max_distance;
        build_rel_table(c, emb, e->rel_R, table);
        UP(upload_f32(e->rel_table, table));
    }
    if (c.pred_heads) {
        // output_layer = Linear(D, N*D) -> GELU -> SplitLinear(D, N, D) (distiller/model.py:155-161): SplitLinear's
        // weight is (N, Din, Dout) (module.py:66-68); each head becomes an (out, in) row-major GEMM operand
        const int NH = c.pred_heads;
        GET("output_layer.0.weight", (long)NH * D * D, t);
        UP(upload_gemm_w(e->head_w1, t, (long)NH * D, D, e->dtype, e->x2));
        if (e->x3) UP(upload_x3(e->head_w13, t, (long)NH * D, D));
        GET("output_layer.0.bias", (long)NH * D, t);
        UP(upload_f32(e->head_b1, t));
        GET("output_layer.2.weight", (long)NH * D * D, t);
        t2.resize(t.size());
        for (int k = 0; k < NH; ++k)
            for (int i = 0; i < D; ++i)
                for (int n = 0; n < D; ++n) t2[((long)k * D + n) * D + i] = t[((long)k * D + i) * D + n];
        UP(upload_gemm_w(e->head_w2, t2, (long)NH * D, D, e->dtype, e->x2));
        if (e->x3) UP(upload_x3(e->head_w23, t2, (long)NH * D, D));
        GET("output_layer.2.bias", (long)NH * D, t);
        UP(upload_f32(e->head_b2, t));
    }
    return finish_create(std::move(e), out);
}

int s3enc_destroy(s3enc_handle h) {
    if (!h) return 0;
    DeviceGuard dg(h->device);
    (void)hipDeviceSynchronize();
    delete h;
    return 0;
}

// frames of an n-sample input; `output`: of the states a forward writes (multires-HuBERT cuts them to a common length)
static long frames_of(s3enc_handle h, long n_samples, bool output) {
    if (h->ops && h->ops->frames) return h->ops->frames(h, n_samples);
    return output ? output_frames(h->cfg, n_samples) : conv_len(h->cfg, n_samples, h->cfg.n_conv);
}
int s3enc_num_frames(s3enc_handle h, int64_t n_samples, int32_t* T) {
    if (!h || !T) return fail("s3enc_num_frames: null argument");
    *T = (int32_t)frames_of(h, n_samples, false);
    return 0;
}
int s3enc_num_output_frames(s3enc_handle h, int64_t n_samples, int32_t* T) {
    if (!h || !T) return fail("s3enc_num_output_frames: null argument");
    *T = (int32_t)frames_of(h, n_samples, true);
    return 0;
}
int s3enc_downsample_rate(s3enc_handle h, int32_t* rate) {
    if (!h || !rate) return fail("s3enc_downsample_rate: null argument");
    int r = 1;
    for (int i = 0; i < h->cfg.n_conv; ++i) r *= h->cfg.conv_stride[i];
    if (h->cfg.family == S3ENC_DECOAR2) r *= 2;  // every second frame: 320, what the reference's get_downsample_rates returns
    *rate = h->ops && h->ops->rate ? h->ops->rate(h) : r;
    return 0;
}
int s3enc_valid_frames(s3enc_handle h, int64_t length, int64_t n_max, int32_t* valid) {
    if (!h || !valid) return fail("s3enc_valid_frames: null argument");
    const FamilyOps* f = h->ops;
    if (f && f->valid) {
        *valid = f->valid(h, length, n_max);
    } else if (f && f->frames) {  // a family's own count and no mask rule: what the utterance's own samples reach, within the batch's
        *valid = (int32_t)std::max(0L, std::min(f->frames(h, length), f->frames(h, n_max)));
    } else {
        *valid = valid_frames(h->cfg, length, n_max);
    }
    return 0;
}

}  // extern "C"

namespace {

int forward_body(s3enc_handle e, const float* const* wav_ptrs_host, const int64_t* lengths, int32_t B, int64_t n_max_in,
                 const FwdOpts& fo, void* out, int64_t layer_stride, hipStream_t st);

// ---- Conformer position tables (host, the reference's fp32 formulas), grown to the largest T seen --------------------------------
// rope: inv_freq = 1 / 10000^(2i / 64), angle = t * inv_freq in fp32 (RotaryPositionalEmbedding, wav2vec2_model.py:40-71)
// rel_pos: div_term = exp(2i * -(ln 10000 / D)), pe[r] = {sin, cos}(p * div_term) of position p = (Tm - 1) - r (RelPositionalEncoding,
//   :1525-1588: flipped positive half, then the negative half without its 0).  A growth waits for the device (the old table may be in
//   use by forwards in flight): once per new longest batch.
int ensure_conformer_tables(s3enc_handle e, hipStream_t st, long T) {
    const s3enc_config& c = e->cfg;
    const int D = c.embed_dim;
    if (c.pos_enc_type == 2 && T > e->rope_T) {
        std::vector<float> tab((size_t)T * 64);
        float inv[32];
        for (int i = 0; i < 32; ++i) inv[i] = 1.0f / std::pow(10000.0f, (float)(2 * i) / 64.0f);
        for (long t = 0; t < T; ++t)
            for (int i = 0; i < 32; ++i) {
                const float a = (float)t * inv[i];
                tab[(size_t)t * 64 + i] = (float)std::cos((double)a);
                tab[(size_t)t * 64 + 32 + i] = (float)std::sin((double)a);
            }
        HIP_TRY(hipStreamSynchronize(st));
        HIP_TRY(upload_f32(e->rope_tab, tab));
        e->rope_T = (int)T;
    }
    if (c.pos_enc_type == 1 && T > e->pe_T) {
        const long R = 2 * T - 1;
        std::vector<float> pe((size_t)R * D);
        const float k = (float)(-(std::log(10000.0) / D));
        std::vector<float> div(D / 2);
        for (int i = 0; i < D / 2; ++i) div[i] = std::exp((float)(2 * i) * k);
        for (long r = 0; r < R; ++r) {
            const long pos = (T - 1) - r;  // the reference evaluates -1 * position * div_term for the negative half
            for (int i = 0; i < D / 2; ++i) {
                const float a = (float)(pos < 0 ? -pos : pos) * div[i];
                const float x = pos < 0 ? -a : a;
                pe[(size_t)r * D + 2 * i] = (float)std::sin((double)x);
                pe[(size_t)r * D + 2 * i + 1] = (float)std::cos((double)x);
            }
        }
        HIP_TRY(hipStreamSynchronize(st));
        HIP_TRY(upload_f32(e->pe_tab, pe));
        e->pe_T = (int)T;
    }
    return 0;
}

struct ConformerBufs {
    void *x32, *xpc, *xT, *qkv, *attn, *tmp1, *tmp2, *hbuf, *cbuf, *pbuf;
};

// The Conformer stack behind post_extract_proj (ConformerEncoder.extract_features, wav2vec2_model.py:3170-3211; layer :523-578),
// exact fp32.  xproj: (B, T, D) with padded frames zero.  States: the input of every layer and the encoder output.
int conformer_tail(s3enc_handle e, hipStream_t st, Sink& sink, int B, long T, const int* d_valid, float* xproj, const ConformerBufs& w) {
    const s3enc_config& c = e->cfg;
    const int D = c.embed_dim, F = c.ffn_dim, H = c.heads, NL = c.encoder_layers;
    const long M = (long)B * T;
    const double gM = (double)M;
    const bool prel = c.layer_norm_first != 0, relpos = c.pos_enc_type == 1;
    static const int dbg_stop = getenv("S3ENC_DEBUG_STOP") ? atoi(getenv("S3ENC_DEBUG_STOP")) : 0;
    if (ensure_conformer_tables(e, st, T)) return 1;
    float *xT = (float*)w.xT, *qkv = (float*)w.qkv, *attn = (float*)w.attn, *tmp1 = (float*)w.tmp1, *tmp2 = (float*)w.tmp2;
    float *hbuf = (float*)w.hbuf, *cbuf = (float*)w.cbuf, *pbuf = (float*)w.pbuf;
    auto other = [&](const float* busy) { return busy == (const float*)w.x32 ? (float*)w.xpc : (float*)w.x32; };
    auto ln = [&](const char* kind, const float* x, const DevBuf& g, const DevBuf& b, float* y, const LnAcc& fa) -> hipError_t {
        Prof pr(e, st, kind, 0, gM * D * 8);
        return launch_layernorm(F32, x, (const float*)g.p, (const float*)b.p, M, D, 0, y, nullptr, st, fa);
    };

    // hidden_states[0]: the layer-0 input — pre-LN: xproj itself (post_extract_proj wrote it into its slot), post-LN:
    // encoder.layer_norm(xproj) (applied before layer 0, wav2vec2_model.py:3182-3183)
    float* x_cur;
    if (prel) {
        x_cur = xproj;
    } else {
        x_cur = sink.slot32(0) ? sink.slot32(0) : other(xproj);
        HIP_TRY(ln("layernorm:enc", xproj, e->eln_g, e->eln_b, x_cur, sink.acc(0, 2)));
        HIP_TRY(sink.done(0));
    }
    for (int l = 0; l < NL; ++l) {
        const ConformerLayerW& L = e->cf_layers[l];
        if (dbg_stop == 40 + l) return 0;
        // x + 0.5 FFN1(x): swish in fc1's epilogue, the 0.5 in w_2 / b_2, the residual in fc2's epilogue
        HIP_TRY(ln("layernorm:ffn", x_cur, L.f1_lng, L.f1_lnb, xT, LnAcc()));
        HIP_TRY(linear_f32(e, st, {"gemm:ffn_w1", xT, L.f1_w1.p, L.f1_b1.p, M, F, D, 3, nullptr, hbuf}));
        HIP_TRY(linear_f32(e, st, {"gemm:ffn_w2", hbuf, L.f1_w2.p, L.f1_b2.p, M, D, F, 0, x_cur, tmp1}));
        if (l == 0) e->taps["ffn1_0"] = {tmp1, M * D, F32};
        // x + MHA(LN(x))
        HIP_TRY(ln("layernorm:attn", tmp1, L.at_lng, L.at_lnb, xT, LnAcc()));
        if (relpos) {
            HIP_TRY(linear_f32(e, st, {"gemm:qkv", xT, L.wqkv.p, L.bqkv.p, M, 3 * D, D, 0, nullptr, qkv}));
            // P = linear_pos(pe) for this T: the centre 2T - 1 rows of the table (depends on T and the layer only)
            GemmParams g{};
            g.A = (const float*)e->pe_tab.p + (long)(e->pe_T - T) * D;
            g.lda = D;
            g.W = L.wpos.p;
            g.M = (int)(2 * T - 1);
            g.N = D;
            g.K = D;
            g.batches = 1;
            g.out32 = pbuf;
            g.ldo = D;
            Prof pr(e, st, "gemm:linear_pos", 2.0 * g.M * D * D, ((double)g.M * D * 2 + (double)D * D) * 4);
            HIP_TRY(launch_gemm(F32, g, st));
        } else {
            // rope: q, k from rot(LN(x)), v from LN(x) (RotaryPositionMultiHeadedAttention, wav2vec2_model.py:275-310)
            {
                Prof pr(e, st, "rope", 0, gM * D * 8);
                HIP_TRY(launch_rope(xT, (const float*)e->rope_tab.p, M, (int)T, D, tmp2, st));
            }
            HIP_TRY(linear_f32(e, st, {"gemm:qk", tmp2, L.wqkv.p, L.bqkv.p, M, 2 * D, D, 0, nullptr, qkv, nullptr, 0, 3L * D}));
            GemmParams g{};
            g.A = xT;
            g.lda = D;
            g.W = (const float*)L.wqkv.p + 2L * D * D;
            g.bias = (const float*)L.bqkv.p + 2L * D;
            g.M = (int)M;
            g.N = D;
            g.K = D;
            g.batches = 1;
            g.out32 = qkv + 2L * D;
            g.ldo = 3L * D;
            Prof pr(e, st, "gemm:v", 2.0 * gM * D * D, (gM * D * 2 + (double)D * D) * 4);
            HIP_TRY(launch_gemm(F32, g, st));
        }
        {
            AttnParams a{};
            a.qkv = qkv;
            a.out = attn;
            a.valid = d_valid;
            a.B = B;
            a.T = (int)T;
            a.H = H;
            a.rel_P = relpos ? pbuf : nullptr;
            a.rel_qadd = relpos ? (const float*)L.qadd.p : nullptr;
            Prof pr(e, st, relpos ? "attention:relpos" : "attention", (relpos ? 6.0 : 4.0) * B * H * (double)T * T * 64, gM * 4 * D * 4);
            HIP_TRY(launch_attention(F32, a, st));
        }
        if (l == 0) e->taps["attn0"] = {attn, M * D, F32};
        HIP_TRY(linear_f32(e, st, {"gemm:out_proj", attn, L.wo.p, L.bo.p, M, D, D, 0, tmp1, tmp2}));
        // x + Conv(x): LN -> pointwise_conv1 -> [GLU, depthwise conv, BatchNorm, swish] -> pointwise_conv2 + residual
        HIP_TRY(ln("layernorm:conv", tmp2, L.cv_lng, L.cv_lnb, xT, LnAcc()));
        HIP_TRY(linear_f32(e, st, {"gemm:pw1", xT, L.pw1.p, nullptr, M, 2 * D, D, 0, nullptr, cbuf}));
        {
            ConformerConvParams p{};
            p.x = cbuf;
            p.taps = (const float*)L.taps.p;
            p.shift = (const float*)L.shift.p;
            p.out = attn;
            p.B = B;
            p.T = (int)T;
            p.D = D;
            p.K = c.dw_kernel;
            Prof pr(e, st, "conformer_conv", 2.0 * gM * D * c.dw_kernel, gM * D * 12);
            HIP_TRY(launch_conformer_conv(p, st));
        }
        if (l == 0) e->taps["conv0_mod"] = {attn, M * D, F32};
        HIP_TRY(linear_f32(e, st, {"gemm:pw2", attn, L.pw2.p, nullptr, M, D, D, 0, tmp2, tmp1}));
        // x + 0.5 FFN2(x), then final_layer_norm: the next layer's input (a state, except behind a pre-LN stack's last layer)
        HIP_TRY(ln("layernorm:ffn", tmp1, L.f2_lng, L.f2_lnb, xT, LnAcc()));
        HIP_TRY(linear_f32(e, st, {"gemm:ffn_w1", xT, L.f2_w1.p, L.f2_b1.p, M, F, D, 3, nullptr, hbuf}));
        HIP_TRY(linear_f32(e, st, {"gemm:ffn_w2", hbuf, L.f2_w2.p, L.f2_b2.p, M, D, F, 0, tmp1, tmp2}));
        if (l == 0) e->taps["ffn2_0"] = {tmp2, M * D, F32};
        const int si_next = (l + 1 < NL || !prel) ? l + 1 : -1;
        float* x_next = sink.slot32(si_next) ? sink.slot32(si_next) : other(x_cur);
        HIP_TRY(ln("layernorm:final", tmp2, L.fin_g, L.fin_b, x_next, sink.acc(si_next, 2)));
        HIP_TRY(sink.done(si_next));
        x_cur = x_next;
    }
    if (prel) {  // encoder.layer_norm on the output (TransformerEncoder.forward, wav2vec2_model.py:3046-3052)
        float* y = sink.slot32(NL) ? sink.slot32(NL) : other(x_cur);
        HIP_TRY(ln("layernorm:enc", x_cur, e->eln_g, e->eln_b, y, sink.acc(NL, 2)));
        HIP_TRY(sink.done(NL));
    }
    return 0;
}

// ---- forward chain: one event per device, re-recorded behind every forward; the next forward (any handle, any stream) waits for it on
// the device.  hipStreamWaitEvent captures the record that is current when it is called, so re-using one event is safe; a stream that
// waits for an event recorded on itself waits for nothing new.  Host cost: two runtime calls per forward under one mutex.
namespace {
struct ForwardChain {
    std::mutex mu;
    hipEvent_t ev[64] = {};
    bool recorded[64] = {};
};
ForwardChain& forward_chain() {
    static ForwardChain* c = new ForwardChain();  // (never destroyed: events must not outlive the runtime at process exit)
    return *c;
}
hipError_t forward_chain_wait(int dev, hipStream_t st) {
    if (dev < 0 || dev >= 64) return hipSuccess;
    ForwardChain& c = forward_chain();
    std::lock_guard<std::mutex> lock(c.mu);
    if (!c.recorded[dev]) return hipSuccess;
    return hipStreamWaitEvent(st, c.ev[dev], 0);
}
hipError_t forward_chain_record(int dev, hipStream_t st) {
    if (dev < 0 || dev >= 64) return hipSuccess;
    ForwardChain& c = forward_chain();
    std::lock_guard<std::mutex> lock(c.mu);
    if (!c.ev[dev]) {
        hipError_t e = hipEventCreateWithFlags(&c.ev[dev], hipEventDisableTiming);
        if (e != hipSuccess) return e;
    }
    hipError_t e = hipEventRecord(c.ev[dev], st);
    if (e == hipSuccess) c.recorded[dev] = true;
    return e;
}
}  // namespace

// The forward proper runs with the handle's tuning and status word current for this thread.  The word is cleared in front of
// it and copied to the next pinned slot behind it, with an event, so that s3enc_forward_status never has to touch the device.
int forward_impl(s3enc_handle e, const float* const* wav_ptrs_host, const int64_t* lengths, int32_t B, int64_t n_max_in,
                 const FwdOpts& fo, void* out, int64_t layer_stride, hipStream_t st) {
    TuningScope tuning_scope(e->has_tuning ? &e->tun : nullptr);
    StatusScope status_scope((int*)e->status_dev.p);
    // forward chain (tuning key forward_chain, kernels.h): this forward starts behind the previous forward of any handle on this device
    // (exact fp32 — the tile kernel waits vmcnt(0) for every buffer_load ... lds — stayed bit-stable in every concurrent run and is left free to overlap)
    const bool chain = tuning().forward_chain != 0 && (e->dtype != F32 || e->x3);
    if (chain) HIP_TRY(forward_chain_wait(e->device, st));
    HIP_TRY(hipMemsetAsync(e->status_dev.p, 0, sizeof(int), st));
    const int rc = forward_body(e, wav_ptrs_host, lengths, B, n_max_in, fo, out, layer_stride, st);
    if (chain) HIP_TRY(forward_chain_record(e->device, st));  // (also behind a failed forward: whatever it enqueued is in the stream)
    if (rc == 0) {
        const int slot = e->status_next;
        if (e->status_busy[slot]) {  // STATUS_RING forwards ago: finished long since unless the host ran far ahead
            HIP_TRY(hipEventSynchronize(e->status_ev[slot]));
            e->status_sticky |= ((volatile int*)e->status_host)[slot];
            e->status_busy[slot] = false;
        }
        HIP_TRY(hipMemcpyAsync(e->status_host + slot, e->status_dev.p, sizeof(int), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipEventRecord(e->status_ev[slot], st));
        e->status_busy[slot] = true;
        e->status_next = (slot + 1) % s3enc_encoder::STATUS_RING;
    }
    return rc;
}

int forward_body(s3enc_handle e, const float* const* wav_ptrs_host, const int64_t* lengths, int32_t B, int64_t n_max_in,
                 const FwdOpts& fo, void* out, int64_t layer_stride, hipStream_t st) {
    if (e->ops) return e->ops->forward(e, wav_ptrs_host, lengths, B, n_max_in, fo, out, layer_stride, st);
    const s3enc_config& c = e->cfg;
    const int C = c.conv_dim, D = c.embed_dim, F = c.ffn_dim, H = c.heads, NL = c.encoder_layers;
    const int dt = e->dtype, es = e->es;
    static const int dbg_stop = getenv("S3ENC_DEBUG_STOP") ? atoi(getenv("S3ENC_DEBUG_STOP")) : 0;
    const bool dist = c.family == S3ENC_DISTILLER;
    const bool mr = c.family == S3ENC_MULTIRES;
    const int NH = dist ? c.pred_heads : 0;
    if (fo.selection < 0 || fo.selection > 2) return fail("s3enc_forward: unknown selection");
    if ((dist || mr) && fo.selection != S3ENC_SEL_HIDDEN)
        return fail("s3enc_forward: DistilHuBERT / multires-HuBERT have one selection (their hidden_states list)");
    const bool lhb = c.family == S3ENC_LIGHTHUBERT;  // hidden_states[0] = post_extract_proj's output, then the layer outputs
    if (lhb && fo.selection != S3ENC_SEL_HIDDEN)
        return fail("s3enc_forward: feature_selection is not defined for LightHuBERT (its expert returns one hidden_states list)");
    const bool d2 = c.family == S3ENC_DECOAR2;  // the batch-wide kaldi front end in place of the conv extractor
    if (d2 && fo.selection != S3ENC_SEL_HIDDEN)
        return fail("s3enc_forward: feature_selection is not defined for DeCoAR 2.0 (its expert returns one hidden_states list)");
    const bool conf = c.layer_type == 1;
    if (conf && fo.selection != S3ENC_SEL_HIDDEN)
        return fail("s3enc_forward: feature_selection is not defined for a Conformer encoder (the reference's ConformerEncoder records "
                    "layer results only for a target layer and returns an empty list)");
    const int NS = num_states(c, fo.selection);
    if (fo.featurize && !fo.w) return fail("s3enc_forward: featurize needs feat_w");
    if (!fo.featurize && fo.out_dtype != F32 && (fo.out_dtype != dt || dt == F32))
        return fail("s3enc_forward: out_dtype must be S3ENC_F32 or the handle's own 16-bit compute dtype");
    long n_max;
    if (batch_n_max(wav_ptrs_host, lengths, B, n_max_in, n_max)) return 1;
    std::vector<long> L(std::max(c.n_conv, 2), 0L);
    for (int i = 0; i < c.n_conv; ++i) L[i] = conv_len(c, n_max, i + 1);
    const long T = L[c.n_conv - 1];
    if (T < 1) return fail("s3enc_forward: input shorter than the receptive field of the conv stack");
    // DeCoAR 2.0: the fbank frames of the padded batch and of every utterance; L[0] = T = ceil(d2_F / 2)
    const long d2_F = d2 ? s3::fbank_num_frames(n_max, decoar2_fbank_params()) : 0;
    const long d2_stride = (n_max + 3) & ~3L;  // row pitch of the staged PCM
    std::vector<int> d2_frames(d2 ? B : 0);
    for (int b = 0; d2 && b < B; ++b) {
        d2_frames[b] = (int)s3::fbank_num_frames(lengths[b], decoar2_fbank_params());
        if (d2_frames[b] < 2)
            return fail("s3enc_forward: an utterance has fewer than 2 analysis windows (DeCoAR 2.0's front end normalises by the standard deviation over time: one frame has none)");
    }
    if (d2 && d2_F > 0x7fffffffL / 1024) return fail("s3enc_forward: batch too large");
    const long M = (long)B * T;
    MrPlan plan;  // multires-HuBERT: the frame geometry of the U-net; the states are (B, plan.T_out, D)
    if (mr) mr_plan(c, T, plan);
    for (const auto& bp : plan.blocks)
        if (bp.T < 1 || plan.T_out < 1) return fail("s3enc_forward: input too short for the coarsest resolution of the U-net");
    const long out_rows = mr ? (long)B * plan.T_out : M;  // rows of every state the forward writes
    if (check_out(out, fo, layer_stride, out_rows * D)) return 1;
    if (c.rel_pos && T > 6000) return fail("s3enc_forward: WavLM relative-position window limited to 6000 frames (120 s) per batch");
    if (conf && T > 100000) return fail("s3enc_forward: Conformer position tables are limited to 100000 frames (max_source_positions)");
    std::vector<int> valid(B);
    for (int b = 0; b < B; ++b) {
        valid[b] = valid_frames(c, lengths[b], n_max);
        if (valid[b] < 1) return fail("s3enc_forward: an utterance is too short to produce a valid frame");
    }
    // multires-HuBERT: un-masked frames per block — the padding mask follows every adapter as
    // repeat_interleave(up)[::down][:T'] (hubert_model.py:1080-1084,1169-1172,1256-1258) and align_size_sum's cut (:777-783)
    std::vector<int> valid_blk;  // blocks 1.., B entries each (block 0 uses `valid`)
    if (mr) {
        std::vector<int> v = valid;
        for (size_t bi = 1; bi < plan.blocks.size(); ++bi) {
            const MrBlockPlan& bp = plan.blocks[bi];
            const AdapterW& aw = e->mr_adapters[bp.adapter];
            const long up = aw.kind == 1 ? 1 : aw.up_rate, down = aw.kind == 2 ? 1 : aw.down_rate;
            for (int b = 0; b < B; ++b) {
                long nv = ((long)v[b] * up + down - 1) / down;
                v[b] = (int)std::min(nv, bp.T);
            }
            valid_blk.insert(valid_blk.end(), v.begin(), v.end());
            for (int b = 0; b < B; ++b) v[b] = (int)std::min<long>(v[b], bp.T_sum);
        }
    }
    DeviceGuard dg(e->device);
    if (!dg.ok) return fail("s3enc_forward: hipSetDevice failed");

    // ---- small device state: tables + stats ----
    const size_t tbl_bytes = (size_t)B * (8 + 8 + 4) + (valid_blk.size() + d2_frames.size()) * 4;  // (never both: one tail)
    const size_t part_elems = stats_partial_elems(B, n_max);
    {
        Bump sb(nullptr);
        sb.take(tbl_bytes);
        sb.take((size_t)B * sizeof(float2));
        sb.take((size_t)B * C * sizeof(float2));
        sb.take(part_elems * 8);
        HIP_TRY(e->small.ensure_on_stream(sb.off + 1024, st));
    }
    Bump sb(e->small.p);
    char* d_tbl = (char*)sb.take(tbl_bytes);
    float2* d_norm = (float2*)sb.take((size_t)B * sizeof(float2));
    float2* d_gn = (float2*)sb.take((size_t)B * C * sizeof(float2));
    double* d_part = (double*)sb.take(part_elems * 8);
    const float* const* d_ptrs = (const float* const*)d_tbl;
    const long* d_lens = (const long*)(d_tbl + (size_t)B * 8);
    const int* d_valid = (const int*)(d_tbl + (size_t)B * 16);

    char* hp;
    if (stage_begin(e, tbl_bytes, st, hp)) return 1;
    memcpy(hp, wav_ptrs_host, (size_t)B * 8);
    for (int b = 0; b < B; ++b) ((long*)(hp + (size_t)B * 8))[b] = (long)lengths[b];
    memcpy(hp + (size_t)B * 16, valid.data(), (size_t)B * 4);
    if (!valid_blk.empty()) memcpy(hp + (size_t)B * 20, valid_blk.data(), valid_blk.size() * 4);
    if (d2) memcpy(hp + (size_t)B * 20, d2_frames.data(), (size_t)B * 4);
    const int* d_frames = (const int*)(d_tbl + (size_t)B * 20);  // DeCoAR 2.0: every utterance's fbank frames
    if (stage_commit(e, hp, d_tbl, tbl_bytes, st)) return 1;

    // ---- workspace ----
    const bool lnmode = c.extractor_layer_norm != 0;
    const bool prel = c.layer_norm_first != 0;
    const bool gated = c.rel_pos && c.gru_rel_pos;
    const bool featln = !c.no_feature_layer_norm && !d2;
    const bool ffn_tap = fo.selection == S3ENC_SEL_FFN_OUT;
    const long HW = std::max<long>(F, (long)NH * D);  // widest row of the FFN / prediction-head intermediate
    void *actA, *actB, *tmp32, *feat32, *featT, *x32, *xpc, *xT, *qkv, *attn, *tmp1, *tmp2, *hbuf, *gate, *ffnbuf, *lnst, *cbuf, *pbuf;
    float *d2_pcm = nullptr, *d2_feat = nullptr, *d2_spec = nullptr;  // DeCoAR 2.0: staged PCM rows, (B, d2_F, 80) log-mels, spectra
    const size_t d2_spec_bytes = d2 ? s3::fbank_batch_workspace(decoar2_fbank_params(), B, d2_F, 0) : 0;
    for (int pass = 0; pass < 2; ++pass) {
        Bump wb(pass ? e->ws.p : nullptr);
        if (d2) {
            d2_pcm = (float*)wb.take((size_t)B * d2_stride * 4);
            d2_feat = (float*)wb.take((size_t)B * d2_F * C * 4);
            d2_spec = (float*)wb.take(d2_spec_bytes);
        }
        // conv0's output in the compute dtype; in the fp16x2 hybrid conv2, conv4, ... write fp32 rows back here: L[2] <= L[0] / 2
        // only when conv1 * conv2 stride >= 2, which no config validation promises
        actA = wb.take(std::max((size_t)B * L[0] * C * (e->x2_conv_f32_from == 1 ? 4 : es),
                                (e->x2_conv_f32_from && c.n_conv > 2) ? (size_t)B * L[2] * C * 4 : (size_t)0));
        actB = wb.take((size_t)B * L[1] * C * (e->x2_conv_f32_from ? 4 : es));  // (fp32 activations between the later convs)
        tmp32 = lnmode ? wb.take((size_t)B * L[1] * C * 4) : nullptr;
        feat32 = featln ? wb.take((size_t)M * C * 4) : nullptr;
        featT = wb.take((size_t)M * C * (e->x2_proj_f32 ? 4 : es));
        x32 = wb.take((size_t)M * D * 4);
        xpc = wb.take((size_t)M * D * 4);
        xT = wb.take((size_t)M * D * es);
        qkv = wb.take((size_t)M * 3 * D * es);
        attn = wb.take((size_t)M * D * (e->x2_attn_f32 ? 4 : es));
        tmp1 = wb.take((size_t)M * D * 4);
        tmp2 = wb.take((size_t)M * D * 4);
        lnst = wb.take((size_t)M * sizeof(float2));  // (mean, rstd) per row: LayerNorm 1 -> fc2's epilogue (ln1_fold)
        hbuf = wb.take((size_t)M * HW * es);
        gate = gated ? wb.take((size_t)B * H * T * 4) : nullptr;
        ffnbuf = (ffn_tap && (fo.featurize || fo.out_dtype != F32)) ? wb.take((size_t)M * D * 4) : nullptr;
        cbuf = conf ? wb.take((size_t)M * 2 * D * 4) : nullptr;                                   // Conformer: pointwise_conv1 output
        pbuf = (conf && c.pos_enc_type == 1) ? wb.take((size_t)(2 * T - 1) * D * 4) : nullptr;    // rel_pos: linear_pos(pe) of this T
        if (!pass) HIP_TRY(e->ws.ensure_on_stream(wb.off + 4096, st));
        // (diagnostic, profiles/r06d_concurrent_forwards_exclusions.md: S3ENC_DEBUG_POISON=1 fills the workspace with NaN patterns in front of
        //  every forward — every buffer is written before it is read, so a correct forward does not change; a read that overtakes its
        //  producer shows as NaN rows instead of plausible numbers)
        static const int dbg_poison = getenv("S3ENC_DEBUG_POISON") ? atoi(getenv("S3ENC_DEBUG_POISON")) : 0;
        if (pass && dbg_poison) HIP_TRY(hipMemsetAsync(e->ws.p, 0xFF, wb.off, st));
    }
    e->taps.clear();

    Sink sink{e, st, fo.featurize ? 2 : (fo.out_dtype != F32 ? 1 : 0), out, (long)layer_stride, dt, M, D, fo.w, fo.feat_norm};
    HIP_TRY(sink.zero_without_terms(NS, out_rows));
    // state index of each tensor of the forward under this selection (-1: not a state)
    const bool hid = fo.selection == S3ENC_SEL_HIDDEN && !dist;
    const bool lay = fo.selection == S3ENC_SEL_LAYER_OUT;
    auto si_hidden = [&](int l) { return hid && !(lhb && l == 0) ? l : -1; };         // input of layer l / encoder output
    auto si_layer_out = [&](int l) { return lay ? l : (dist ? 1 + l : -1); };         // output of layer l
    auto si_stream = [&](int l) {  // the tensor "residual stream after layer l" as the next layer's input
        const int a = (l + 1 < NL || !prel) ? si_hidden(l + 1) : -1;  // pre-LN: the encoder output is the normed stream
        return a >= 0 ? a : si_layer_out(l);
    };
    auto other = [&](const float* busy) { return busy == (const float*)x32 ? (float*)xpc : (float*)x32; };

    WavTable wt{d_ptrs, d_lens, B, n_max};
    // (diagnostic: S3ENC_DEBUG_KEEP=1 copies conv0 and the early conv outputs aside behind their kernel, so that a FULL forward keeps them as
    //  taps — the workspace reuses their buffers; the copies are never freed: a debugging process)
    static const int dbg_keep = getenv("S3ENC_DEBUG_KEEP") ? atoi(getenv("S3ENC_DEBUG_KEEP")) : 0;
    auto keep_tap = [&](const char* name, int idx, const void* src, long elems, int tdt) -> hipError_t {
        if (!dbg_keep) return hipSuccess;
        static std::map<std::pair<const void*, int>, std::pair<void*, size_t>> kept;
        static std::mutex kept_mu;
        const size_t bytes = (size_t)elems * (tdt == F32 ? 4 : 2);
        void* kp = nullptr;
        {
            std::lock_guard<std::mutex> lk(kept_mu);
            auto& slot = kept[{(const void*)e, idx}];
            if (slot.second < bytes) {
                hipError_t er = hipMalloc(&slot.first, bytes);
                if (er != hipSuccess) return er;
                slot.second = bytes;
            }
            kp = slot.first;
        }
        hipError_t er = hipMemcpyAsync(kp, src, bytes, hipMemcpyDeviceToDevice, st);
        if (er != hipSuccess) return er;
        e->taps[name] = {kp, elems, tdt};
        return hipSuccess;
    };
    if (d2) {
        // every utterance's samples into one (B, d2_stride) slab, zeros behind them: the batched GEMM wants one row pitch
        {
            Prof pr(e, st, "decoar2_stage", 0, 8.0 * B * n_max);
            hipLaunchKernelGGL((s3::reflect_pad_kernel<long>), dim3((unsigned)((d2_stride + 255) / 256), B), dim3(256), 0, st, d_ptrs, d_lens,
                               (const float*)nullptr, n_max, 0, d2_stride, d2_pcm);
        }
        Prof pr(e, st, "decoar2_fbank", 2.0 * B * d2_F * 514 * 400, 4.0 * ((double)B * n_max + (double)B * d2_F * (2 * 514 + 2 * C)));
        HIP_TRY(s3::launch_fbank_batch(decoar2_fbank_params(), d2_pcm, d2_stride, d_frames, B, d2_F, d2_feat, C, d2_spec, d2_spec_bytes, 0, st));
        e->taps["fbank"] = {d2_feat, (long)B * d2_F * C, F32};
    }
    if (!d2) {
        Prof pr(e, st, "wav_stats", 0, 4.0 * B * n_max);
        HIP_TRY(launch_wav_norm_stats(wt, c.normalize, d_part, d_norm, st, c.wav_norm_eps));
    }
    if (!lnmode && !d2) {
        Prof pr(e, st, "gn_stats", 0, 4.0 * B * n_max);
        HIP_TRY(launch_gn_stats(wt, d_norm, (const float*)e->conv[0].w.p, (const float*)e->gn_g.p, (const float*)e->gn_b.p, C,
                                c.conv_kernel[0], c.conv_stride[0], L[0], d_part, nullptr, d_gn, st));
    }
    if (!d2) {
        Conv0Params p{};
        p.wav = wt;
        p.norm = d_norm;
        p.w0 = (const float*)e->conv[0].w.p;
        p.bias = e->conv[0].has_bias ? (const float*)e->conv[0].bias.p : nullptr;
        p.gn = lnmode ? nullptr : d_gn;
        p.ln_g = lnmode ? (const float*)e->conv[0].lng.p : nullptr;
        p.ln_b = lnmode ? (const float*)e->conv[0].lnb.p : nullptr;
        p.C = C;
        p.k0 = c.conv_kernel[0];
        p.s0 = c.conv_stride[0];
        p.L0 = L[0];
        p.out = actA;
        const bool c0f32 = e->x2_conv_f32_from == 1;  // (fp16x2_conv1_f32: conv1 reads fp32 rows)
        p.fast = e->x3 || c0f32;
        p.nt = tuning().conv0_nt;
        Prof pr(e, st, "conv0", 2.0 * B * L[0] * C * p.k0, 4.0 * B * n_max + (double)B * L[0] * C * (c0f32 ? 4 : es));
        HIP_TRY(launch_conv0(c0f32 ? (int)F32 : dt, p, st));
        // (diagnostic, tools/two_stream_probe.py --taps: S3ENC_DEBUG_STOP = k ends the forward behind conv(k - 1) and keeps its output as a tap)
        if (dbg_stop) e->taps["conv0"] = {actA, (long)B * L[0] * C, c0f32 ? (int)F32 : dt};
        else HIP_TRY(keep_tap("conv0", 0, actA, (long)B * L[0] * C, c0f32 ? (int)F32 : dt));
        if (dbg_stop == 1) return 0;
    }
    // conv1..: implicit GEMM on channel-last activations.  The last one feeds LayerNorm(C) in fp32, or — without that
    // norm (DistilHuBERT) — post_extract_proj directly, in the compute dtype.
    void* cur = actA;
    for (int i = 1; i < c.n_conv; ++i) {
        const bool last = i == c.n_conv - 1;
        // S3ENC_F16X2, GroupNorm extractor: conv `x2_conv_f32_from`.. read fp32 activations through the three-term GEMM
        const bool x3in = e->x2_conv_f32_from && i >= e->x2_conv_f32_from;
        const bool x3next = e->x2_conv_f32_from && i + 1 >= e->x2_conv_f32_from && !last;
        const bool f32out = dt == F32 || (last && featln) || x3next;
        void* dst = last ? (featln ? feat32 : featT) : (cur == actA ? actB : actA);
        GemmParams g{};
        g.A = cur;
        g.lda = (long)c.conv_stride[i] * C;
        g.a_bs = L[i - 1] * C;
        g.W = e->conv[i].w.p;
        g.W_x3 = e->conv[i].w3.p;
        g.bias = e->conv[i].has_bias ? (const float*)e->conv[i].bias.p : nullptr;
        g.M = (int)L[i];
        g.N = C;
        g.K = c.conv_kernel[i] * C;
        g.batches = B;
        g.ldo = C;
        g.o_bs = L[i] * C;
        const double fl = 2.0 * B * L[i] * C * g.K;
        const double by = ((double)B * L[i - 1] * C + (double)C * g.K) * (x3in ? 4 : es) + (double)B * L[i] * C * (f32out ? 4 : es);
        char kind[32];
        snprintf(kind, sizeof(kind), "gemm:conv%d", i);
        // S3ENC_F32, k = 3, stride 2: the two-output form (convf22.hip); eligibility depends on C and the buffers, never on B or L
        ConvF22Params f22{};
        bool use_f22 = false;
        if (dt == F32 && !e->x3 && !x3in && c.conv_kernel[i] == 3 && c.conv_stride[i] == 2 && e->conv[i].wp.p) {
            f22.x = (const float*)cur;
            f22.x_bs = L[i - 1] * C;
            f22.W = (const float*)e->conv[i].w.p;
            f22.WP = (const float*)e->conv[i].wp.p;
            f22.bias = g.bias;
            f22.M = (int)L[i];
            f22.C = C;
            f22.batches = B;
            f22.act = lnmode ? 0 : 1;
            f22.out = (float*)(lnmode ? tmp32 : dst);
            f22.o_bs = L[i] * C;
            use_f22 = conv_f22_eligible(f22);
        }
        if (!lnmode) {
            g.act = 1;
            if (f32out) g.out32 = (float*)dst; else g.out16 = dst;
            Prof pr(e, st, kind, fl, by);
            if (use_f22) {
                HIP_TRY(launch_conv_f22(f22, st));
            } else if (x3in) {
                if (!gemm_x3_eligible(g)) return fail("conv layer is not a shape of the three-term GEMM (internal)");
                HIP_TRY(launch_gemm(F32, g, st));
            } else {
                HIP_TRY(launch_gemm(dt, wsplit_of(e, g), st));
            }
        } else {
            g.act = 0;
            g.out32 = (float*)tmp32;
            {
                Prof pr(e, st, kind, fl, by);
                if (use_f22) {
                    HIP_TRY(launch_conv_f22(f22, st));
                } else if (x3in) {  // fp32 LayerNorm output of the previous conv -> three-term GEMM (S3ENC_F16X2, see x2_conv_f32_from)
                    if (!gemm_x3_eligible(g)) return fail("conv layer is not a shape of the three-term GEMM (internal)");
                    HIP_TRY(launch_gemm(F32, g, st));
                } else {
                    HIP_TRY(launch_gemm(dt, wsplit_of(e, g), st));
                }
            }
            Prof pr(e, st, "layernorm:conv", 0, (double)B * L[i] * C * (4 + (f32out ? 4 : es)));
            HIP_TRY(launch_layernorm(dt, (const float*)tmp32, (const float*)e->conv[i].lng.p, (const float*)e->conv[i].lnb.p,
                                     (long)B * L[i], C, e->x3 ? 2 : 1, f32out ? (float*)dst : nullptr, f32out ? nullptr : dst, st));
        }
        char tn[16];
        snprintf(tn, sizeof(tn), "conv%d", i);
        if (i >= c.n_conv - 3 || dbg_stop) e->taps[tn] = {dst, (long)B * L[i] * C, f32out ? (int)F32 : dt};  // earlier ones get overwritten
        else HIP_TRY(keep_tap(tn, i, dst, (long)B * L[i] * C, f32out ? (int)F32 : dt));
        if (dbg_stop == 1 + i) return 0;
        cur = dst;
    }
    // LayerNorm(C) -> post_extract_proj (+ zero padded frames)
    const bool proj32 = dt == F32 || (e->x2_proj_f32 && featln);  // the projection's operand stays fp32
    if (featln) {
        Prof pr(e, st, "layernorm:feat", 0, (double)M * C * (4 + (proj32 ? 4 : es)));
        HIP_TRY(launch_layernorm(dt, (const float*)feat32, (const float*)e->fln_g.p, (const float*)e->fln_b.p, M, C, 0,
                                 proj32 ? (float*)featT : nullptr, proj32 ? nullptr : featT, st));
        e->taps["feat_ln"] = {featT, M * C, proj32 ? (int)F32 : dt};
        if (dbg_stop == 20) return 0;
    }
    // DistilHuBERT: hidden_states[0] = feat_final, padded frames zeroed in place; a pre-LN Conformer's hidden_states[0] is the same
    // tensor (ConformerEncoder has no positional conv and zeroes the padded frames, wav2vec2_model.py:3170-3175); LightHuBERT's too
    const int si_proj = (dist || lhb || (conf && c.layer_norm_first)) ? 0 : -1;
    float* xproj = sink.slot32(si_proj) ? sink.slot32(si_proj) : (float*)x32;
    {
        GemmParams g{};
        g.A = d2 ? (const void*)d2_feat : featT;
        g.lda = d2 ? 2L * C : C;  // DeCoAR 2.0: every second fbank row costs nothing, the rows are read at twice the pitch
        g.a_bs = d2 ? d2_F * C : T * C;
        g.W = e->proj_w.p;
        g.W_x3 = e->proj_w3.p;
        g.bias = (const float*)e->proj_b.p;
        g.M = (int)T;
        g.N = D;
        g.K = C;
        g.batches = B;
        g.row_limit = d_valid;
        g.out32 = xproj;
        g.out16 = sink.slot16(si_proj);
        g.ldo = D;
        g.o_bs = T * D;
        {
            Prof pr(e, st, "gemm:proj", 2.0 * M * D * C, ((double)M * C + (double)D * C) * es + (double)M * D * 4);
            if (d2) {  // fp32 operands in every mode (e->proj_w is an fp32 image, W_x3 is null)
                HIP_TRY(launch_gemm(F32, g, st));
            } else if (proj32 && dt != F32) {
                if (!gemm_x3_eligible(g)) return fail("post_extract_proj is not a shape of the three-term GEMM (internal)");
                HIP_TRY(launch_gemm(F32, g, st));
            } else {
                HIP_TRY(launch_gemm(dt, wsplit_of(e, g), st));
            }
        }
        e->taps["proj"] = {xproj, M * D, F32};
        if (dbg_stop == 21) return 0;
        HIP_TRY(sink.emit(si_proj, xproj, false));
        HIP_TRY(sink.done(si_proj));
    }
    if (mr) {
        std::vector<const int*> dv(plan.blocks.size(), d_valid);
        for (size_t bi = 1; bi < plan.blocks.size(); ++bi) dv[bi] = (const int*)(d_tbl + (size_t)B * 20) + (bi - 1) * (size_t)B;
        return multires_tail(e, st, B, plan, dv, xproj, out, (long)layer_stride, fo) ? 1 : 0;
    }
    if (conf) {
        ConformerBufs cb{x32, xpc, xT, qkv, attn, tmp1, tmp2, hbuf, cbuf, pbuf};
        return conformer_tail(e, st, sink, B, T, d_valid, xproj, cb);
    }
    // positional conv + residual; hidden_states[0]
    float* x_cur;          // the fp32 residual stream entering the layer loop
    void* a16_cur = nullptr;  // post-LN 16-bit modes: its 16-bit copy (the q|k|v operand)
    {
        const int si0 = si_hidden(0);
        float* pc_out = prel ? (sink.slot32(si0) ? sink.slot32(si0) : other(xproj)) : other(xproj);
        PosConvParams p{};
        p.x = xproj;
        p.w = e->pos_w.p;
        p.bias = (const float*)e->pos_b.p;
        p.out = pc_out;
        p.B = B;
        p.T = (int)T;
        p.D = D;
        p.G = c.conv_pos_groups;
        p.K = e->pos_k;  // conv_pos, or conv_pos + zero taps in the 16-bit / fp32x3 modes
        p.pad = e->pos_pad;
        auto run_conv = [&](PosConvParams& q) -> hipError_t {
            if (e->x3) return launch_posconv16(3, q, st);
            return dt == F32 ? launch_posconv(q, st) : launch_posconv16(dt, q, st);
        };
        if (c.pos_conv_depth > 1) {
            // data2vec: x + block_n(...block_1(x)), block = conv -> LayerNorm(no affine) -> GELU (wav2vec2_model.py:2999-3017)
            const float* cur_in = xproj;
            const int gelu_act = (dt != F32 || e->x3) ? 2 : 1;
            for (int i = 0; i < c.pos_conv_depth; ++i) {
                p.x = cur_in;
                p.w = e->pos_ws[i].p;
                p.bias = (const float*)e->pos_bs[i].p;
                p.out = (float*)tmp1;
                p.K = e->pos_k;
                p.pad = e->pos_pad;
                p.plain = 1;
                {
                    Prof pr(e, st, "posconv", 2.0 * M * D * (D / p.G) * (2 * e->pos_pad + 1), (double)M * D * 8);
                    HIP_TRY(run_conv(p));
                }
                Prof pr(e, st, "layernorm:posconv", 0, (double)M * D * 8);
                HIP_TRY(launch_layernorm(F32, (const float*)tmp1, (const float*)e->ones.p, (const float*)e->zeros.p, M, D, gelu_act,
                                         (float*)tmp2, nullptr, st));
                cur_in = (const float*)tmp2;
            }
            Prof pr(e, st, "residual_add", 0, (double)M * D * 12);
            HIP_TRY(launch_add(xproj, (const float*)tmp2, pc_out, M * D, st));
            p.out = pc_out;
        } else {
            Prof pr(e, st, "posconv", 2.0 * M * D * (D / p.G) * c.conv_pos, (double)M * D * 8 + (double)D * (D / p.G) * c.conv_pos * 4);
            if (e->x3) p.w = e->pos_w3.p;
            HIP_TRY(run_conv(p));
        }
        e->taps["posconv"] = {p.out, M * D, F32};
        if (dbg_stop == 22) return 0;
        if (prel) {
            x_cur = pc_out;
            if (sink.mode == 1) HIP_TRY(sink.emit(si0, pc_out));  // featurize: ln1 of layer 0 adds this state's term
            HIP_TRY(sink.done(si0));
        } else {
            float* h0 = sink.slot32(si0) ? sink.slot32(si0) : other(pc_out);
            void* h16 = dt == F32 ? nullptr : (sink.slot16(si0) ? sink.slot16(si0) : xT);
            Prof pr(e, st, "layernorm:enc", 0, (double)M * D * (8 + (dt == F32 ? 0 : es)));
            LnGate g0;  // post-LN WavLM: the gate of layer 0 reads this LayerNorm's output
            if (gated) {
                g0.gw = (const float*)e->layers[0].grep_w.p;
                g0.gb = (const float*)e->layers[0].grep_b.p;
                g0.ga = (const float*)e->layers[0].grep_a.p;
                g0.gate = (float*)gate;
                g0.T = (int)T;
                g0.H = H;
            }
            HIP_TRY(launch_layernorm(dt, pc_out, (const float*)e->eln_g.p, (const float*)e->eln_b.p, M, D, 0, h0, h16, st,
                                     sink.acc(si0, 2), g0));
            x_cur = h0;
            a16_cur = h16;
            HIP_TRY(sink.done(si0));
        }
    }
    const float* d_table = c.rel_pos ? (const float*)e->rel_table.p : nullptr;
    // WavLM gate of layer l's attention, computed by the LayerNorm that produces that attention's input
    auto gate_of = [&](int l) {
        LnGate g;
        if (gated && l < NL) {
            const LayerW& w = e->layers[l];
            g.gw = (const float*)w.grep_w.p;
            g.gb = (const float*)w.grep_b.p;
            g.ga = (const float*)w.grep_a.p;
            g.gate = (float*)gate;
            g.T = (int)T;
            g.H = H;
        }
        return g;
    };

    const double gM = (double)M;
    int si_cur = si_hidden(0);  // state index of x_cur (pre-LN featurize: its term is added by the LayerNorm that reads it)
    LayerRun run{B, T, d_valid, prel};
    run.xT = xT;
    run.qkv = qkv;
    run.attn = attn;
    run.hbuf = hbuf;
    run.tmp1 = (float*)tmp1;
    run.tmp2 = (float*)tmp2;
    run.lnst = (float2*)lnst;
    run.bias_table = d_table;
    run.table_R = e->rel_R;
    run.gate = gated ? (const float*)gate : nullptr;
    run.allow_ln1_fold = !ffn_tap && tuning().ln1_fold;
    run.ln1_inplace = tuning().ws_inplace;
    int l = 0;
    if (ffn_tap)  // "fairseq_layers_before_residual": state l is fc2(x) + bias, final behind the GEMM that exports it
        run.ffn_exported = [&]() -> int {
            HIP_TRY(sink.emit(l, run.ffn_out32, false));
            HIP_TRY(sink.done(l));
            return 0;
        };
    for (; l < NL; ++l) {
        if (dbg_stop == 40 + l) return 0;  // (before layer l)
        // pre-LN: fc2's result IS the residual stream after the layer (a state for l < NL-1, and for the fairseq_layers /
        // DistilHuBERT selections); post-LN: the state is final_layer_norm's output
        const int si_next = si_stream(l);
        void* s16 = sink.slot16(si_next);
        run.x = x_cur;
        run.x16 = a16_cur;
        // (the last pre-LN layer's raw stream goes to tmp2 when it is not a state, which keeps the "proj" debug tap in x32
        // alive through a default forward)
        run.x_next = sink.slot32(si_next) ? sink.slot32(si_next) : ((prel && l == NL - 1) ? (float*)tmp2 : other(x_cur));
        run.x16_next = (prel || dt == F32 || s16) ? s16 : xT;
        // the WavLM gate of a layer's attention is computed by the LayerNorm that produces that attention's input
        run.gate_here = gate_of(l);
        run.gate_next = gate_of(l + 1);
        run.acc_in = prel ? sink.acc(si_cur, 1) : LnAcc();
        run.acc_out = prel ? LnAcc() : sink.acc(si_next, 2);
        if (ffn_tap) {
            run.ffn_out32 = sink.slot32(l) ? sink.slot32(l) : (float*)ffnbuf;
            run.ffn_out16 = sink.slot16(l);
        }
        run.taps = l == 0;
        run.stop_after = l == 0 ? dbg_stop : 0;
        if (const int rc = encoder_layer(e, st, e->layers[l], run)) return rc == LAYER_STOPPED ? 0 : 1;
        HIP_TRY(sink.done(si_next));
        if (!prel) a16_cur = run.x16_next;
        x_cur = run.x_next;
        si_cur = si_next;
    }
    const float* enc_out = x_cur;  // what the DistilHuBERT heads read
    const void* enc_out16 = a16_cur;
    if (prel) {
        // encoder.layer_norm on the last residual stream (wav2vec2_model.py:3049-3050): the encoder output
        const int si_fin = si_hidden(NL);
        float* y = sink.slot32(si_fin) ? sink.slot32(si_fin) : other(x_cur);
        void* y16 = dt == F32 ? nullptr : (sink.slot16(si_fin) ? sink.slot16(si_fin) : xT);
        // featurize: this LayerNorm adds the term of its output (hidden list) or of its input (fairseq_layers / distiller)
        LnAcc fa = sink.wanted(si_fin) ? sink.acc(si_fin, 2) : sink.acc(si_cur, 1);
        Prof pr(e, st, "layernorm:enc", 0, gM * D * 8);
        HIP_TRY(launch_layernorm(dt, x_cur, (const float*)e->eln_g.p, (const float*)e->eln_b.p, M, D, 0, y, y16, st, fa));
        HIP_TRY(sink.done(si_fin));
        enc_out = y;
        enc_out16 = y16;
    }
    if (NH) {
        // DistilHuBERT prediction heads (distiller/model.py:155-161,245-258): Linear(D, NH*D) + GELU, then per head k
        // the (D x D) slice of SplitLinear on columns [k*D, (k+1)*D) of the intermediate
        {
            Linear q{"gemm:head1", dt == F32 ? (const void*)enc_out : enc_out16, e->head_w1.p, e->head_b1.p, M, NH * D, D, 1};
            q.W_x3 = e->head_w13.p;
            if (dt == F32) q.out32 = (float*)hbuf; else q.out16 = hbuf;
            if (linear(e, st, q)) return 1;
        }
        for (int k = 0; k < NH; ++k) {
            const int si = 1 + NL + k;
            float* dst = sink.slot32(si) ? sink.slot32(si) : (float*)tmp1;
            // (x2: W rows are [hi | lo])
            Linear q{"gemm:head2", (const char*)hbuf + (size_t)k * D * es, (const char*)e->head_w2.p + (size_t)k * D * D * es * (e->x2 ? 2 : 1),
                     (const float*)e->head_b2.p + (long)k * D, M, D, D};
            q.W_x3 = e->head_w23.p ? (const char*)e->head_w23.p + (size_t)k * D * D * 4 : nullptr;
            q.lda = (long)NH * D;
            q.out32 = dst;
            q.out16 = sink.slot16(si);
            if (linear(e, st, q)) return 1;
            HIP_TRY(sink.emit(si, dst, false));
            HIP_TRY(sink.done(si));
        }
    }
    return 0;
}
}  // namespace

extern "C" {

static int parse_opts(s3enc_handle h, const s3enc_forward_opts* o, FwdOpts& fo) {
    if (!o) return 0;
    fo.selection = o->selection;
    fo.out_dtype = o->out_dtype;
    fo.featurize = o->featurize != 0;
    fo.feat_norm = o->feat_normalize != 0;
    fo.w = o->feat_w;
    if (fo.out_dtype < 0 || fo.out_dtype > 2) return fail("s3enc_forward_ex: out_dtype must be S3ENC_F32 / BF16 / F16");
    return 0;
}

int s3enc_forward(s3enc_handle h, const float* const* wavs, const int64_t* lengths, int32_t B, int64_t n_max, float* out,
                  int64_t layer_stride, void* stream) {
    if (!h || !wavs || !lengths) return fail("s3enc_forward: null argument");
    return forward_impl(h, wavs, lengths, B, n_max, FwdOpts(), out, layer_stride, (hipStream_t)stream);
}

int s3enc_forward_ex(s3enc_handle h, const float* const* wavs, const int64_t* lengths, int32_t B, int64_t n_max,
                     const s3enc_forward_opts* opts, void* out, int64_t layer_stride, void* stream) {
    if (!h || !wavs || !lengths) return fail("s3enc_forward_ex: null argument");
    FwdOpts fo;
    if (parse_opts(h, opts, fo)) return 1;
    return forward_impl(h, wavs, lengths, B, n_max, fo, out, layer_stride, (hipStream_t)stream);
}

int s3enc_forward_aux(s3enc_handle h, const float* const* wavs, const int64_t* lengths, int32_t B, int64_t n_max,
                      const s3enc_forward_opts* opts, void* out, int64_t layer_stride, float* codewords, int64_t* codeids, void* stream) {
    if (!h || !wavs || !lengths) return fail("s3enc_forward_aux: null argument");
    if ((codewords || codeids) && h->cfg.family != S3ENC_WAV2VEC)
        return fail("s3enc_forward_aux: codewords / codeids are outputs of a wav2vec handle with a vector quantizer");
    h->aux_codewords = codewords;
    h->aux_codeids = (long long*)codeids;
    const int rc = s3enc_forward_ex(h, wavs, lengths, B, n_max, opts, out, layer_stride, stream);
    h->aux_codewords = nullptr;
    h->aux_codeids = nullptr;
    return rc;
}

int s3enc_forward_status(s3enc_handle h, int32_t wait, int32_t* status) {
    if (!h || !status) return fail("s3enc_forward_status: null argument");
    DeviceGuard dg(h->device);
    const int running = h->status_collect(wait != 0);
    *status = h->status_sticky | (running ? S3ENC_STATUS_PENDING : 0);
    h->status_sticky = 0;
    return 0;
}

int s3enc_num_states(s3enc_handle h, int32_t selection, int32_t* n) {
    if (!h || !n) return fail("s3enc_num_states: null argument");
    if (selection < 0 || selection > 2) return fail("s3enc_num_states: unknown selection");
    if (h->cfg.family == S3ENC_LIGHTHUBERT && selection != S3ENC_SEL_HIDDEN)
        return fail("s3enc_num_states: feature_selection is not defined for LightHuBERT (its expert returns one hidden_states list)");
    if (h->cfg.family == S3ENC_DECOAR2 && selection != S3ENC_SEL_HIDDEN)
        return fail("s3enc_num_states: feature_selection is not defined for DeCoAR 2.0 (its expert returns one hidden_states list)");
    if ((h->cfg.family == S3ENC_DISTILLER || h->cfg.family == S3ENC_MULTIRES) && selection != S3ENC_SEL_HIDDEN)
        return fail("s3enc_num_states: DistilHuBERT / multires-HuBERT have one selection (their hidden_states list)");
    if (h->cfg.layer_type == 1 && selection != S3ENC_SEL_HIDDEN)
        return fail("s3enc_num_states: feature_selection is not defined for a Conformer encoder");
    if (h->ops && h->ops->one_list && selection != S3ENC_SEL_HIDDEN)
        return fail(std::string("s3enc_num_states: feature_selection is not defined for ") + h->ops->one_list);
    *n = h->ops && h->ops->states ? h->ops->states(h) : num_states(h->cfg, selection);
    return 0;
}

int s3enc_forward_padded(s3enc_handle h, const float* pcm, int64_t row_stride, const int64_t* lengths, int32_t B, int64_t n_max,
                         float* out, int64_t layer_stride, void* stream) {
    if (!h || !pcm || !lengths) return fail("s3enc_forward_padded: null argument");
    if (B <= 0) return fail("s3enc_forward_padded: B must be positive");
    std::vector<const float*> ptrs(B);
    for (int b = 0; b < B; ++b) {
        if (lengths[b] > row_stride) return fail("s3enc_forward_padded: length exceeds row_stride");
        ptrs[b] = pcm + (long)b * row_stride;
    }
    return forward_impl(h, ptrs.data(), lengths, B, n_max, FwdOpts(), out, layer_stride, (hipStream_t)stream);
}

int s3enc_set_layer_events(s3enc_handle h, void* const* events, int32_t n) {
    if (!h) return fail("null handle");
    if (n == 0) {
        h->layer_events.clear();
        return 0;
    }
    if (!events || n < h->cfg.encoder_layers || n > num_states(h->cfg, S3ENC_SEL_HIDDEN))
        return fail("s3enc_set_layer_events: pass one event per state of the selection the forwards will use");
    h->layer_events.assign((hipEvent_t const*)events, (hipEvent_t const*)events + n);
    return 0;
}

int s3enc_profile_enable(s3enc_handle h, int32_t on) {
    if (!h) return fail("null handle");
    h->prof = on == 2 ? 2 : (on != 0);
    return 0;
}
int s3enc_profile_reset(s3enc_handle h) {
    if (!h) return fail("null handle");
    DeviceGuard dg(h->device);
    HIP_TRY(hipDeviceSynchronize());
    for (auto& r : h->recs) {
        h->ev_pool.push_back(r.a);
        h->ev_pool.push_back(r.b);
    }
    h->recs.clear();
    h->kinds.clear();
    h->kflops.clear();
    h->kbytes.clear();
    h->klaunches.clear();
    return 0;
}
int s3enc_profile_read(s3enc_handle h, s3enc_profile_entry* entries, int32_t max_entries, int32_t* n_entries) {
    if (!h || !entries || !n_entries) return fail("s3enc_profile_read: null argument");
    DeviceGuard dg(h->device);
    HIP_TRY(hipDeviceSynchronize());
    std::vector<double> ms(h->kinds.size(), 0.0);
    for (auto& r : h->recs) {
        float t = 0.f;
        HIP_TRY(hipEventElapsedTime(&t, r.a, r.b));
        ms[r.kind] += t;
    }
    int n = 0;
    for (size_t k = 0; k < h->kinds.size() && n < max_entries; ++k, ++n) {
        memset(&entries[n], 0, sizeof(entries[n]));
        strncpy(entries[n].name, h->kinds[k].c_str(), sizeof(entries[n].name) - 1);
        entries[n].launches = h->klaunches[k];
        entries[n].ms = ms[k];
        entries[n].flops = h->kflops[k];
        entries[n].bytes = h->kbytes[k];
    }
    *n_entries = n;
    return 0;
}

int s3enc_debug_tap(s3enc_handle h, const char* name, float* host_out, int64_t max_elems, int64_t* n_elems) {
    if (!h || !name || !n_elems) return fail("s3enc_debug_tap: null argument");
    auto it = h->taps.find(name);
    if (it == h->taps.end()) return fail(std::string("s3enc_debug_tap: unknown tap '") + name + "'");
    *n_elems = it->second.elems;
    if (!host_out) return 0;
    if (max_elems < it->second.elems) return fail("s3enc_debug_tap: buffer too small");
    DeviceGuard dg(h->device);
    HIP_TRY(hipDeviceSynchronize());
    if (it->second.dtype == F32) {
        HIP_TRY(hipMemcpy(host_out, it->second.p, (size_t)it->second.elems * 4, hipMemcpyDeviceToHost));
    } else {
        std::vector<uint16_t> tmp((size_t)it->second.elems);
        HIP_TRY(hipMemcpy(tmp.data(), it->second.p, tmp.size() * 2, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < tmp.size(); ++i) host_out[i] = h_from16(tmp[i], it->second.dtype);
    }
    return 0;
}
}  // extern "C"
