// vggish.hip — VGGish (upstream/vggish/audio.py:30-84,256-294, vggish.py:18-133, expert.py:16-40), exact fp32: the un-padded
// log-mel front end cut into examples of `example_frames` frames, a stack of 3 x 3 Conv2d + ReLU (+ 2 x 2 max-pool) layers, three
// Linear + ReLU layers and the PCA / clamp / 8-bit quantiser.  The reference runs its utterances one by one and pad_sequences the
// (E_b, D) results; here the examples of ALL utterances are one batch of sum E_b images.
//
// Schedule (all on the caller's stream, no host synchronisation):
//   front end: fbank.hip's fold — the periodic Hann window and the zero-padded n_fft-point real DFT as ONE (2 nbin) x window matrix,
//              built in float64 at create — so the spectrum of an utterance's E_b * example_frames frames is a GEMM whose A rows
//              overlap in the caller's PCM (lda = shift); frames of an incomplete last example are not computed;
//              spectral.h's mel_rows_kernel: |X| -> the mel matrix (float64 on the host, rounded once) -> log(. + offset), written into the
//              first layer's operand, the BORDERED single-channel image (E, frames + 2, bands + 2) indexed by example, frame, band;
//   layer 0:   conv2d.hip's VALU kernel (C = 1), layers 1..: its MFMA kernel; bias -> ReLU -> max-pool in the epilogue, each into
//              the interior of the next layer's bordered (H + 2, W + 2, C) operand.  The last layer writes a plain contiguous
//              (E, H, W, C) buffer: channel-last IS the reference's flatten order (frames, bands, channels), so that buffer is the
//              first Linear's A operand;
//   Linears:   the fp32 tile GEMM with M = examples, then launch_relu (the GEMM's epilogues have no ReLU);
//   vggish_post_kernel: the PCA product in the reference's order (P (y - m), y - m rounded first), clamp, rintf (half to even),
//              scattered into (B, E_max, D) with exact zero rows behind every utterance's own examples; without postprocess the
//              same scatter of the embedding itself.
// Every layer's bordered operand is cleared with one memset per forward (the workspace is shared by forwards of every shape, so a
// border zeroed for one batch is not where the next batch's border lies); the convolutions write interiors only.
#include <cmath>

#include "engine_internal.h"
#include "spectral.h"

namespace s3e {

namespace {

// one workgroup per (utterance, example slot) row of the (B, E_max, D) state; off[b] = the first example of utterance b in `emb`
__global__ __launch_bounds__(256) void vggish_post_kernel(const float* emb, const int* off, const int* cnt, int E_max, int D,
                                                          const float* P, const float* mean, int post, float qmin, float qmax,
                                                          float qscale, float* out) {
    extern __shared__ float d[];
    const int b = blockIdx.x / E_max, slot = blockIdx.x - b * E_max;
    float* o = out + (long)blockIdx.x * D;
    if (slot >= cnt[b]) {
        for (int j = threadIdx.x; j < D; j += blockDim.x) o[j] = 0.f;
        return;
    }
    const float* y = emb + (long)(off[b] + slot) * D;
    if (!post) {
        for (int j = threadIdx.x; j < D; j += blockDim.x) o[j] = y[j];
        return;
    }
    for (int j = threadIdx.x; j < D; j += blockDim.x) d[j] = y[j] - mean[j];
    __syncthreads();
    for (int j = threadIdx.x; j < D; j += blockDim.x) {
        const float* p = P + (long)j * D;
        float acc = 0.f;
        for (int k = 0; k < D; ++k) acc = fmaf(p[k], d[k], acc);
        const float c = fminf(fmaxf(acc, qmin), qmax);  // a NaN would come out as qmin; the embedding is finite for finite PCM
        o[j] = rintf((c - qmin) * qscale);
    }
}

int vggish_pools(const s3enc_vggish_config& x) {
    int p = 0;
    for (int i = 0; i < x.n_layers; ++i) p += x.pool_after[i] ? 1 : 0;
    return p;
}

// index of layer i's Conv2d in the reference's nn.Sequential: a conv and its ReLU count two, a pool one
int vggish_seq_index(const s3enc_vggish_config& x, int i) {
    int k = 0;
    for (int j = 0; j < i; ++j) k += 2 + (x.pool_after[j] ? 1 : 0);
    return k;
}

}  // namespace

// E of an n-sample utterance, 0 when it holds no example
static long vggish_num_examples(const s3enc_vggish_config& x, long n_samples) {
    if (n_samples < x.window) return 0;
    const long F = 1 + (n_samples - x.window) / x.shift;
    return F < x.example_frames ? 0 : 1 + (F - x.example_frames) / x.example_hop;
}

static int vggish_check_config(const s3enc_config& c, const s3enc_vggish_config& x) {
    static const char* dt[] = {"fp32", "bf16", "fp16", "fp32x3", "fp16x2"};
    if (c.compute_dtype < 0 || c.compute_dtype > 4) return fail("config: unknown compute_dtype");
    if (c.compute_dtype != S3ENC_F32)
        return fail(std::string("config: VGGish (log-mel examples + 3 x 3 convolutions + Linears) is built for compute dtype fp32 only; ") +
                    dt[c.compute_dtype] + " is not built");
    if (x.n_layers < 1 || x.n_layers > S3ENC_VGGISH_MAX_LAYERS) return fail("config: vggish n_layers must be 1..8");
    for (int i = 0; i < x.n_layers; ++i)
        if (x.channels[i] < 16 || (x.channels[i] & 15) || x.channels[i] > 4096)
            return fail("config: vggish channels of layer " + std::to_string(i) + " must be a multiple of 16, at most 4096 (got " +
                        std::to_string(x.channels[i]) + "): a tap is a whole number of 64-byte K steps");
    const int div = 1 << vggish_pools(x);
    if (x.example_frames < 1 || x.example_frames > 4096 || x.example_frames % div)
        return fail("config: vggish example_frames " + std::to_string(x.example_frames) + " is not divisible by 2^pools = " + std::to_string(div));
    if (x.num_mel_bins < 1 || x.num_mel_bins > 1024 || x.num_mel_bins % div)
        return fail("config: vggish num_mel_bins " + std::to_string(x.num_mel_bins) + " is not divisible by 2^pools = " + std::to_string(div));
    if (x.example_hop != x.example_frames)
        return fail("config: vggish example_hop " + std::to_string(x.example_hop) + " is not built: only example_hop = example_frames (" +
                    std::to_string(x.example_frames) + "), examples that do not overlap");
    if (x.window < 4 || x.shift < 4 || (x.window & 3) || (x.shift & 3) || x.window > 4096)
        return fail("config: vggish window / shift must be a multiple of 4 samples (the front end's GEMM reads 16-byte vectors)");
    int nfft = 1;
    while (nfft < x.window) nfft <<= 1;
    if (x.n_fft != nfft) return fail("config: vggish n_fft must be the power of two at or above window (" + std::to_string(nfft) + ")");
    if (!(x.mel_min_hz >= 0.f) || !(x.mel_min_hz < x.mel_max_hz) || !(x.mel_max_hz <= 8000.f))
        return fail("config: vggish mel edges must satisfy 0 <= mel_min_hz < mel_max_hz <= 8000");
    if (!(x.log_offset > 0.f)) return fail("config: vggish log_offset must be positive");
    for (int i = 0; i < 3; ++i)
        if (x.fc[i] < 4 || (x.fc[i] & 3) || x.fc[i] > 16384) return fail("config: vggish Linear widths must be multiples of 4, at most 16384");
    if (x.postprocess < 0 || x.postprocess > 1) return fail("config: vggish postprocess must be 0 or 1");
    if (x.postprocess && !(x.quant_min < x.quant_max)) return fail("config: vggish quantiser range must satisfy quant_min < quant_max");
    if (c.n_conv != 1 || c.conv_kernel[0] != x.window || c.conv_stride[0] != x.shift)
        return fail("config: vggish carries its frame geometry as n_conv = 1, conv_kernel[0] / conv_stride[0] = window / shift in samples");
    if (c.conv_dim != x.fc[2] || c.embed_dim != x.fc[2] || c.encoder_layers != 0)
        return fail("config: vggish conv_dim / embed_dim must be the last Linear's width and encoder_layers 0 (one state)");
    return 0;
}

static int vggish_create(s3enc_encoder* e, const Ckpt& ck) {
    const s3enc_vggish_config& x = e->vggish_cfg;
    e->vggish.reset(new VggishW());
    VggishW& w = *e->vggish;
    std::vector<float> t, packed;
    int cin = 1, H = x.example_frames, W = x.num_mel_bins;
    for (int i = 0; i < x.n_layers; ++i) {
        const std::string nm = "features." + std::to_string(vggish_seq_index(x, i));
        const int N = x.channels[i];
        w.cw.emplace_back();
        w.cb.emplace_back();
        GET(nm + ".weight", (long)N * cin * 9, t);
        s3::pack_conv2d3x3(t.data(), N, cin, packed);
        UP(upload_f32(w.cw.back(), packed));
        GET(nm + ".bias", N, t);
        UP(upload_f32(w.cb.back(), t));
        cin = N;
        if (x.pool_after[i]) {
            H >>= 1;
            W >>= 1;
        }
    }
    long K = (long)H * W * cin;
    for (int i = 0; i < 3; ++i) {
        const std::string nm = "embeddings." + std::to_string(2 * i);
        GET(nm + ".weight", (long)x.fc[i] * K, t);
        UP(upload_f32(w.fw[i], t));
        GET(nm + ".bias", x.fc[i], t);
        UP(upload_f32(w.fb[i], t));
        K = x.fc[i];
    }
    if (x.postprocess) {
        const long D = x.fc[2];
        GET("pca_eigen_vectors", D * D, t);
        UP(upload_f32(w.pca, t));
        GET("pca_means", D, t);
        UP(upload_f32(w.pca_mean, t));
    }
    // the front end's constants, float64 on the host and rounded once
    const int N = x.window, nb = x.n_fft / 2 + 1, nmel = x.num_mel_bins;
    UP(upload_f32(w.dft, s3::fold_dft(s3::hann_periodic(N).data(), N, x.n_fft)));
    std::vector<int> bands;
    s3::sparsify(s3::vggish_bank(nb, nmel, x.mel_min_hz, x.mel_max_hz), nb, nmel, bands, t);
    UP(upload_f32(w.wts, t));
    UP(w.bands.ensure(bands.size() * sizeof(int)));
    UP(hipMemcpy(w.bands.p, bands.data(), bands.size() * sizeof(int), hipMemcpyHostToDevice));
    return 0;
}

static int vggish_forward(s3enc_handle e, const float* const* wav_ptrs_host, const int64_t* lengths, int32_t B, int64_t n_max_in,
                   const FwdOpts& fo, void* out, int64_t layer_stride, hipStream_t st) {
    const s3enc_vggish_config& x = e->vggish_cfg;
    const VggishW& w = *e->vggish;
    const int D = x.fc[2], NL = x.n_layers, FR = x.example_frames, NM = x.num_mel_bins, nb = x.n_fft / 2 + 1, N2 = 2 * nb;
    if (fo.selection != S3ENC_SEL_HIDDEN)
        return fail("s3enc_forward: feature_selection is not defined for VGGish (the reference expert has one hidden_states list)");
    if (fo.featurize && !fo.w) return fail("s3enc_forward: featurize needs feat_w");
    if (!fo.featurize && fo.out_dtype != F32) return fail("s3enc_forward: out_dtype must be S3ENC_F32 for a VGGish handle");
    if (e->aux_codewords || e->aux_codeids) return fail("s3enc_forward_aux: codewords / codeids are outputs of a wav2vec handle with a vector quantizer");
    if (B > 65535) return fail("s3enc_forward: batch too large");
    long n_max;
    if (batch_n_max(wav_ptrs_host, lengths, B, n_max_in, n_max)) return 1;
    const long shortest = x.window + (long)(FR - 1) * x.shift;
    std::vector<int> tbl(2 * (size_t)B);  // first example, examples
    long Etot = 0;
    for (int b = 0; b < B; ++b) {
        const long E = vggish_num_examples(x, lengths[b]);
        if (E < 1)
            return fail("s3enc_forward: utterance " + std::to_string(b) + " has " + std::to_string((long)lengths[b]) +
                        " samples, fewer than one VGGish example of " + std::to_string(shortest) + " samples (" + std::to_string(FR) +
                        " frames; the reference raises on it)");
        if (((uintptr_t)wav_ptrs_host[b]) & 3) return fail("s3enc_forward: utterance " + std::to_string(b) + " is not 4-byte aligned");
        tbl[b] = (int)Etot;
        tbl[B + b] = (int)E;
        Etot += E;
    }
    const long E_max = vggish_num_examples(x, n_max);
    const long M = (long)B * E_max;
    if (M > 0x7fffffffL / 8 || Etot > (1L << 20)) return fail("s3enc_forward: batch too large");
    if (check_out(out, fo, layer_stride, M * D)) return 1;
    DeviceGuard dg(e->device);
    if (!dg.ok) return fail("s3enc_forward: hipSetDevice failed");

    // ---- layer geometry ----
    struct Geo {
        int H, W, C, Ho, Wo, pad;  // input map and channels, output map, border of the output buffer
        size_t out_elems;
    };
    std::vector<Geo> geo(NL);
    {
        int H = FR, W = NM, C = 1;
        for (int i = 0; i < NL; ++i) {
            Geo& g = geo[i];
            g.H = H;
            g.W = W;
            g.C = C;
            g.Ho = x.pool_after[i] ? H / 2 : H;
            g.Wo = x.pool_after[i] ? W / 2 : W;
            g.pad = i == NL - 1 ? 0 : 1;
            g.out_elems = (size_t)Etot * (g.Ho + 2 * g.pad) * (g.Wo + 2 * g.pad) * x.channels[i];
            if (g.out_elems * 4 >= (1ul << 32) - 64)
                return fail("s3enc_forward: batch too large (" + std::to_string(Etot) + " examples: layer " + std::to_string(i) +
                            "'s activation is not addressable with 32-bit offsets)");
            H = g.Ho;
            W = g.Wo;
            C = x.channels[i];
        }
    }
    const long Kflat = (long)geo[NL - 1].Ho * geo[NL - 1].Wo * x.channels[NL - 1];
    const long rows = Etot * FR;  // spectrum rows
    if (rows * N2 * 4 >= (1L << 32)) return fail("s3enc_forward: batch too large");

    // ---- small device state: first example / examples per utterance ----
    const size_t tbl_bytes = tbl.size() * sizeof(int);
    HIP_TRY(e->small.ensure_on_stream(tbl_bytes + 1024, st));
    int* d_tbl = (int*)e->small.p;
    char* hp;
    if (stage_begin(e, tbl_bytes, st, hp)) return 1;
    memcpy(hp, tbl.data(), tbl_bytes);
    if (stage_commit(e, hp, d_tbl, tbl_bytes, st)) return 1;

    // ---- workspace ----
    bool misaligned = false;
    for (int b = 0; b < B; ++b) misaligned |= (((uintptr_t)wav_ptrs_host[b]) & 15) != 0;
    float *spec, *img, *fcb[2], *post = nullptr, *stage = nullptr;
    std::vector<float*> act(NL);
    const int fcw = std::max(x.fc[0], std::max(x.fc[1], x.fc[2]));
    for (int pass = 0; pass < 2; ++pass) {
        Bump wb(pass ? e->ws.p : nullptr);
        spec = (float*)wb.take((size_t)rows * N2 * 4);
        img = (float*)wb.take((size_t)Etot * (FR + 2) * (NM + 2) * 4);
        for (int i = 0; i < NL; ++i) act[i] = (float*)wb.take(geo[i].out_elems * 4);
        for (int i = 0; i < 2; ++i) fcb[i] = (float*)wb.take((size_t)Etot * fcw * 4);
        if (fo.featurize) post = (float*)wb.take((size_t)M * D * 4);
        if (misaligned) stage = (float*)wb.take((size_t)n_max * 4 + 64);
        if (!pass) HIP_TRY(e->ws.ensure_on_stream(wb.off + 4096, st));
    }
    e->taps.clear();

    Sink sink{e, st, fo.featurize ? 2 : 0, out, (long)layer_stride, F32, M, D, fo.w, fo.feat_norm};
    HIP_TRY(sink.zero_without_terms(1, M));

    // ---- front end ----
    {
        Prof pr(e, st, "vggish_frontend", 2.0 * rows * N2 * x.window + 2.0 * rows * nb * NM,
                4.0 * ((double)B * n_max + 2.0 * rows * N2 + (double)Etot * (FR + 2) * (NM + 2)));
        HIP_TRY(hipMemsetAsync(img, 0, (size_t)Etot * (FR + 2) * (NM + 2) * 4, st));
        for (int b = 0; b < B; ++b) {
            const long Eb = tbl[B + b], nuse = x.window + (Eb * FR - 1) * x.shift;  // the samples its complete examples read
            const float* a = wav_ptrs_host[b];
            if (((uintptr_t)a) & 15) {  // the GEMM loads 16-byte vectors: stage a misaligned waveform (stream-ordered re-use)
                HIP_TRY(hipMemcpyAsync(stage, a, (size_t)nuse * 4, hipMemcpyDeviceToDevice, st));
                a = stage;
            }
            GemmParams g{};
            g.A = a;
            g.lda = x.shift;  // overlapping rows: frame t starts at sample t * shift
            g.W = w.dft.p;
            g.M = (int)(Eb * FR);
            g.N = N2;
            g.K = x.window;
            g.batches = 1;
            g.out32 = spec + (size_t)tbl[b] * FR * N2;
            g.ldo = N2;
            HIP_TRY(launch_gemm(F32, g, st));
        }
        // row r of `spec` is frame r % FR of example r / FR: into the interior of the bordered image
        hipLaunchKernelGGL((s3::mel_rows_kernel<s3::MAGNITUDE, s3::LogAdd>), dim3((unsigned)rows), dim3(128), nb * sizeof(float), st, spec, nb, FR,
                           (const int*)w.bands.p, (const float*)w.wts.p, NM, s3::LogAdd{x.log_offset}, img + (NM + 2) + 1,
                           (long)(FR + 2) * (NM + 2), (long)(NM + 2), (float*)nullptr);
        HIP_TRY(hipGetLastError());
    }

    // ---- the convolution stack ----
    for (int i = 0; i < NL; ++i) {
        const Geo& g = geo[i];
        const int N = x.channels[i];
        s3::Conv2dParams q{};
        q.src = i == 0 ? img : act[i - 1];
        q.src_bs = (long)(g.H + 2) * (g.W + 2) * g.C;
        q.C = g.C;
        q.Wt = (const float*)w.cw[i].p;
        q.bias = (const float*)w.cb[i].p;
        q.H = g.H;
        q.W = g.W;
        q.N = N;
        q.B = (int)Etot;
        q.act = 1;
        q.pool = x.pool_after[i] ? 1 : 0;
        q.dst = act[i];
        q.dst_pad = g.pad;
        q.ld_dst = N;
        q.dst_bs = (long)(g.Ho + 2 * g.pad) * (g.Wo + 2 * g.pad) * N;
        if (const char* why = s3::conv2d3x3_refusal(q))
            return fail(std::string("s3enc_forward: the 3 x 3 convolution of layer ") + std::to_string(i) + " refuses: " + why);
        const double px = (double)Etot * g.H * g.W;
        const std::string kind = i == 0 ? std::string("conv2d3x3:first") : "conv2d3x3:L" + std::to_string(i);
        Prof pr(e, st, kind.c_str(), 2.0 * px * N * 9 * g.C,
                4.0 * ((double)Etot * q.src_bs + 9.0 * N * g.C + (g.pad ? 2.0 : 1.0) * (double)g.out_elems));
        if (g.pad) HIP_TRY(hipMemsetAsync(act[i], 0, g.out_elems * 4, st));
        HIP_TRY(s3::launch_conv2d3x3(q, st));
    }

    // ---- the Linears ----
    const float* a = act[NL - 1];
    long K = Kflat;
    for (int i = 0; i < 3; ++i) {
        const std::string kind = "gemm:vggish_fc" + std::to_string(i);
        HIP_TRY(linear_f32(e, st, {kind.c_str(), a, w.fw[i].p, w.fb[i].p, Etot, x.fc[i], (int)K, 0, nullptr, fcb[i & 1]}));
        {
            Prof pr(e, st, "relu", 0, 8.0 * Etot * x.fc[i]);
            HIP_TRY(launch_relu(fcb[i & 1], Etot * x.fc[i], st));
        }
        a = fcb[i & 1];
        K = x.fc[i];
    }

    e->taps["logmel"] = {img, Etot * (FR + 2) * (NM + 2), F32};  // the bordered examples, (sum E, frames + 2, bands + 2)
    e->taps["emb"] = {(void*)a, Etot * D, F32};                  // the embeddings, (sum E, D), before the post-processor

    // ---- PCA + quantiser + scatter (zero rows behind every utterance's own examples) ----
    float* dst = fo.featurize ? post : sink.slot32(0);
    {
        Prof pr(e, st, "vggish_post", x.postprocess ? 2.0 * Etot * D * D : 0.0, 4.0 * ((double)Etot * D + (double)M * D + (double)D * D));
        hipLaunchKernelGGL(vggish_post_kernel, dim3((unsigned)M), dim3(256), D * sizeof(float), st, a, d_tbl, d_tbl + B, (int)E_max, D,
                           (const float*)w.pca.p, (const float*)w.pca_mean.p, x.postprocess, x.quant_min, x.quant_max,
                           (float)(255.0 / ((double)x.quant_max - (double)x.quant_min)), dst);
        HIP_TRY(hipGetLastError());
    }
    if (sink.term(0)) {
        Prof pr(e, st, "emit_state", 0, 4.0 * M * D * 2);
        HIP_TRY(sink.emit(0, dst));
    }
    HIP_TRY(sink.done(0));
    return 0;
}


// frames: examples; valid: the utterance's own examples (the rows behind them are exact zeros); rate: vggish/expert.py:21-22 (the
// examples are 15360 samples apart; the reference says 16000)
FamilyOps kVggishFamily = {
    S3ENC_VGGISH, "vggish", "S3ENC_VGGISH", "s3enc_create_vggish", "the VGGish family needs its front-end / layer block",
    "VGGish (one hidden_states list)",
    [](const s3enc_config& c, const void* b) { return vggish_check_config(c, *(const s3enc_vggish_config*)b); },
    [](s3enc_encoder* e, const Ckpt& ck, const void* b) { e->vggish_cfg = *(const s3enc_vggish_config*)b; return vggish_create(e, ck); },
    vggish_forward,
    [](const s3enc_encoder* h, long n) { return vggish_num_examples(h->vggish_cfg, n); },
    nullptr,
    [](const s3enc_encoder*) { return 16000; }};

}  // namespace s3e
