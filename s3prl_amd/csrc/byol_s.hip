// byol_s.hip — BYOL-S (upstream/byol_s/expert.py:12-36, serab_byols/serab.py:106-170, serab_byols/utils.py:31-106,
// byol_a/models/resnetish.py, byol_a/models/audio_ntt.py), exact fp32.
//
// Windows (utils.py:51-106, frame_audio): the batch is zero-padded to n_max, every row gets window / 2 zeros in front and window -
// window / 2 behind, and window k is padded[k * step : k * step + window], k = 0 .. n_max / step: S = n_max / step + 1.  Window (b, k)
// therefore starts at sample k * step - window / 2 of utterance b: its samples in front of the utterance (`lead`) and at or behind the
// utterance's own length are zeros.  The state is (B, S, 2048) and NOTHING is masked — BYOL-A's convention.
//
// Front end (serab.py:136-160): melspec.hip with the hann(400)-in-1024 window table, un-normalised: log(mel + FLT_EPSILON) as
// (window, frame, mel), all N = B S windows at once.
//
// Statistics (utils.py:31-48, compute_timestamp_stats) over every element of the N x T x 64 log-mel tensor: mean = x.mean() / N, std =
// x.std() / N (unbiased) — both divided by the number of windows, the reference's own arithmetic, kept.  Two passes (the mean, then the
// squared deviations from it), each a two-stage reduction in float64: stats_partial_kernel gives every one of NPART workgroups its own
// contiguous slice (a thread strides its slice, the workgroup folds a fixed tree in LDS), stats_combine_kernel folds the NPART
// partials in one workgroup in a fixed order.  No atomics: the bits depend on the element count only.  The two results are rounded
// once to fp32 and divided by N in fp32 on the device; nothing is read back.  normalise_kernel then writes (x - mean) / std into the
// interior of the network's bordered single-channel operand.
//
// Networks, on the TRANSPOSED image (H = time, W = mel; every tap is transposed at pack time, as byol_a.hip does):
//   default    AudioNTT2020: byol_a.hip's network as it is (three conv + BatchNorm + ReLU + floor-pool layers, two Linears, max + mean);
//   resnetish  stem.hip (7 x 7 conv + BatchNorm + ReLU + MaxPool2d(3, 2, 1)), then BasicBlocks on conv2d.hip's general form:
//              t = relu(bn1(conv3x3_s(x))), y = relu(bn2(conv3x3(t)) + id), id = x or bn(conv1x1_s(x)) (the first block of layers 2-4, s
//              = 2).  Every BatchNorm is the epilogue's per-channel scale / shift (float64 on the host, rounded once), the residual is
//              added behind it and before the ReLU.  The last map is written without a border as (window, T', 4, 512): row t of a
//              window is the reference's permute(0, 3, 2, 1).reshape order d * 512 + c, and byol_a.hip's tail kernel gives max_t +
//              mean_t (its ReLU is the identity on a map that is behind one).
// The network runs over the windows in chunks of tuning().byol_s_chunk: the workspace is bounded by the chunk, and since conv2d.hip's
// and the GEMM's K order is fixed and their M axis only enumerates windows, a window's bits do not depend on the chunk size.
// Everything runs on the caller's stream without host synchronisation.
#include <cmath>

#include "engine_internal.h"

namespace s3e {

namespace {

constexpr int NPART = 1024;

// pass 0: part[p] = sum of slice p; pass 1: sum of (x - mean)^2 of slice p
__global__ __launch_bounds__(256) void stats_partial_kernel(const float* x, long n, long per, int pass, const double* mean, double* part) {
    __shared__ double red[256];
    const int tid = threadIdx.x;
    const long lo = (long)blockIdx.x * per, hi = lo + per < n ? lo + per : n;
    const double m = pass ? *mean : 0.0;
    double acc = 0.0;
    for (long i = lo + tid; i < hi; i += 256) {
        const double v = (double)x[i] - m;
        acc += pass ? v * v : v;
    }
    red[tid] = acc;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    if (tid == 0) part[blockIdx.x] = red[0];
}

// pass 0: mean (kept in float64 for pass 1) and stats[0] = fp32(mean) / N; pass 1: stats[1] = fp32(sqrt(sum / (n - 1))) / N
__global__ __launch_bounds__(256) void stats_combine_kernel(const double* part, long n, long N, int pass, double* mean, float* stats) {
    __shared__ double red[256];
    const int tid = threadIdx.x;
    double acc = 0.0;
    for (int i = tid; i < NPART; i += 256) acc += part[i];
    red[tid] = acc;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    if (tid != 0) return;
    if (pass == 0) {
        const double m = red[0] / (double)n;
        *mean = m;
        stats[0] = (float)m / (float)N;
    } else {
        stats[1] = (float)sqrt(red[0] / (double)(n - 1)) / (float)N;
    }
}

// (window, frame, mel) -> the interior of bordered (T + 2 bd) x (64 + 2 bd) images: PrecomputedNorm, (x - mean) / std in fp32
__global__ __launch_bounds__(256) void normalise_kernel(const float* x, const float* stats, long n, int T, int bd, float* out, long o_bs) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= n) return;
    const int m = (int)(idx & 63);
    const long r = idx >> 6;
    const long w = r / T;
    const int t = (int)(r - w * T);
    out[w * o_bs + (long)(t + bd) * (64 + 2 * bd) + m + bd] = (x[idx] - stats[0]) / stats[1];
}

const char* kNetworks[] = {"default", "resnetish", "cvt", "clstm"};

// an eval-mode BatchNorm2d behind a bias-free convolution as the epilogue's (scale, shift)
int fold_bn(const Ckpt& ck, const std::string& bn, int C, float eps, DevBuf& scale, DevBuf& shift) {
    std::vector<float> g, b, rm, rv, sc(C), sh(C);
    GET(bn + ".weight", C, g);
    GET(bn + ".bias", C, b);
    GET(bn + ".running_mean", C, rm);
    GET(bn + ".running_var", C, rv);
    for (int n = 0; n < C; ++n) {
        const double var = (double)rv[n] + (double)eps;
        if (!(var > 0.0)) return fail("checkpoint: " + bn + ".running_var[" + std::to_string(n) + "] + eps is not positive");
        const double s = (double)g[n] / std::sqrt(var);
        sc[n] = (float)s;
        sh[n] = (float)((double)b[n] - (double)rm[n] * s);
    }
    UP(upload_f32(scale, sc));
    UP(upload_f32(shift, sh));
    return 0;
}

// nn.Conv2d's (N, C, k, k) with its taps transposed (the image is time x mel), as conv2d.hip's image
int load_conv(const Ckpt& ck, const std::string& name, int N, int C, int k, DevBuf& dst) {
    std::vector<float> t, tt, packed;
    GET(name, (long)N * C * k * k, t);
    if (k == 1) {
        UP(upload_f32(dst, t));
        return 0;
    }
    tt.resize(t.size());
    for (long nc = 0; nc < (long)N * C; ++nc)
        for (int ky = 0; ky < 3; ++ky)
            for (int kx = 0; kx < 3; ++kx) tt[nc * 9 + kx * 3 + ky] = t[nc * 9 + ky * 3 + kx];
    s3::pack_conv2d3x3(tt.data(), N, C, packed);
    UP(upload_f32(dst, packed));
    return 0;
}

}  // namespace

static long byol_s_num_windows(const s3enc_byol_s_config& x, long n_samples) { return n_samples < 0 ? 0 : n_samples / x.step + 1; }

static int byol_s_check_config(const s3enc_config& c, const s3enc_byol_s_config& x) {
    static const char* dt[] = {"fp32", "bf16", "fp16", "fp32x3", "fp16x2"};
    if (c.compute_dtype < 0 || c.compute_dtype > 4) return fail("config: unknown compute_dtype");
    if (c.compute_dtype != S3ENC_F32)
        return fail(std::string("config: BYOL-S (FFT log-mel windows + whole-batch statistics + a ResNet of 3 x 3 convolutions) is built for "
                                "compute dtype fp32 only; ") + dt[c.compute_dtype] + " is not built");
    if (x.network == S3ENC_BYOL_S_CVT || x.network == S3ENC_BYOL_S_CLSTM)
        return fail(std::string("config: byol_s network ") + kNetworks[x.network] + " is not built (default and resnetish are)");
    if (x.network != S3ENC_BYOL_S_DEFAULT && x.network != S3ENC_BYOL_S_RESNETISH) return fail("config: unknown byol_s network");
    if (x.network == S3ENC_BYOL_S_RESNETISH) {
        if (x.bottleneck) return fail("config: byol_s Bottleneck blocks (resnetish50) are not built: BasicBlock layers only");
        for (int i = 0; i < 4; ++i)
            if (x.blocks[i] < 1 || x.blocks[i] > 64)
                return fail("config: byol_s layer" + std::to_string(i + 1) + " needs 1..64 BasicBlocks (got " + std::to_string(x.blocks[i]) + ")");
    }
    if (x.window <= 512)
        return fail("config: byol_s window of " + std::to_string(x.window) + " samples is too short: a window of at most 512 samples cannot be "
                    "reflect-padded by 512 (n_fft / 2)");
    if (x.network == S3ENC_BYOL_S_DEFAULT && x.window < 1120)
        return fail("config: byol_s window of " + std::to_string(x.window) + " samples is too short for the default network: fewer than 8 frames "
                    "(1120 samples), nothing survives three 2 x 2 pools");
    if (x.window > (1 << 22)) return fail("config: byol_s window is too long");
    if (x.step < 1) return fail("config: byol_s step must be at least one sample");
    if (!(x.bn_eps > 0.f)) return fail("config: byol_s bn_eps must be positive");
    if (c.n_conv != 1 || c.conv_kernel[0] != x.window || c.conv_stride[0] != x.step)
        return fail("config: byol_s carries its window geometry as n_conv = 1, conv_kernel[0] / conv_stride[0] = window / step in samples");
    if (c.conv_dim != 2048 || c.embed_dim != 2048 || c.encoder_layers != 0)
        return fail("config: byol_s conv_dim / embed_dim must be 2048 and encoder_layers 0 (one state)");
    return 0;
}

static int byol_s_create(s3enc_encoder* e, const Ckpt& ck) {
    const s3enc_byol_s_config& x = e->byol_s_cfg;
    e->byol_s.reset(new ByolSW());
    ByolSW& w = *e->byol_s;
    if (x.network == S3ENC_BYOL_S_DEFAULT) return byol_a_load(w.ntt, ck, 2048, x.bn_eps);
    {
        std::vector<float> t, tt(64 * 49), packed;
        GET("conv1.weight", 64L * 49, t);
        for (int n = 0; n < 64; ++n)  // tap (time, mel) here is the reference's (mel, time)
            for (int ky = 0; ky < 7; ++ky)
                for (int kx = 0; kx < 7; ++kx) tt[n * 49 + ky * 7 + kx] = t[n * 49 + kx * 7 + ky];
        s3::pack_stem7x7(tt.data(), packed);
        UP(upload_f32(w.stem_w, packed));
        if (fold_bn(ck, "bn1", 64, x.bn_eps, w.stem_s, w.stem_t)) return 1;
    }
    int cin = 64;
    for (int L = 0; L < 4; ++L) {
        const int planes = 64 << L;
        for (int b = 0; b < x.blocks[L]; ++b) {
            const std::string pre = "layer" + std::to_string(L + 1) + "." + std::to_string(b) + ".";
            w.blocks.emplace_back();
            ByolSBlockW& k = w.blocks.back();
            k.cin = cin;
            k.cout = planes;
            k.stride = (L > 0 && b == 0) ? 2 : 1;
            k.down = k.stride != 1 || cin != planes;
            if (load_conv(ck, pre + "conv1.weight", planes, cin, 3, k.w1) || fold_bn(ck, pre + "bn1", planes, x.bn_eps, k.s1, k.t1)) return 1;
            if (load_conv(ck, pre + "conv2.weight", planes, planes, 3, k.w2) || fold_bn(ck, pre + "bn2", planes, x.bn_eps, k.s2, k.t2)) return 1;
            if (k.down && (load_conv(ck, pre + "downsample.0.weight", planes, cin, 1, k.wd) ||
                           fold_bn(ck, pre + "downsample.1", planes, x.bn_eps, k.sd, k.td)))
                return 1;
            cin = planes;
        }
    }
    return 0;
}

namespace {

// one launch of conv2d.hip's general form inside the ResNet
struct ConvCall {
    const float* src;
    int H, W, C, N, k, stride, act;
    const DevBuf *wt, *scale, *shift;
    const float* res;
    int res_pad;
    float* dst;
    int dst_pad;
};
int run_conv(s3enc_encoder* e, hipStream_t st, int nb, const ConvCall& c) {
    const int Ho = s3::conv2d_out(c.H, c.k, c.stride), Wo = s3::conv2d_out(c.W, c.k, c.stride);
    s3::Conv2dParams q{};
    q.src = c.src;
    q.src_bs = (long)(c.H + 2) * (c.W + 2) * c.C;
    q.C = c.C;
    q.Wt = (const float*)c.wt->p;
    q.scale = (const float*)c.scale->p;
    q.shift = (const float*)c.shift->p;
    q.H = c.H;
    q.W = c.W;
    q.N = c.N;
    q.B = nb;
    q.act = c.act;
    q.n64 = 1;
    q.gen = 1;
    q.k = c.k;
    q.stride = c.stride;
    q.res = c.res;
    q.res_pad = c.res_pad;
    q.ld_res = c.N;
    q.res_bs = (long)(Ho + 2 * c.res_pad) * (Wo + 2 * c.res_pad) * c.N;
    q.dst = c.dst;
    q.dst_pad = c.dst_pad;
    q.ld_dst = c.N;
    q.dst_bs = (long)(Ho + 2 * c.dst_pad) * (Wo + 2 * c.dst_pad) * c.N;
    if (const char* why = s3::conv2d3x3_refusal(q)) return fail(std::string("s3enc_forward: a convolution of the BYOL-S ResNet refuses: ") + why);
    const std::string kind = "conv2d:k" + std::to_string(c.k) + "s" + std::to_string(c.stride) + ":" + std::to_string(c.C) + ">" +
                             std::to_string(c.N) + "@" + std::to_string(Ho) + "x" + std::to_string(Wo) + (c.res ? "+res" : "");
    const double px = (double)nb * Ho * Wo;
    Prof pr(e, st, kind.c_str(), 2.0 * px * c.N * c.k * c.k * c.C,
            4.0 * ((double)nb * q.src_bs + (double)c.N * c.k * c.k * c.C + px * c.N * (c.res ? 2.0 : 1.0)));
    HIP_TRY(s3::launch_conv2d3x3(q, st));
    return 0;
}

}  // namespace

static int byol_s_forward(s3enc_handle e, const float* const* wav_ptrs_host, const int64_t* lengths, int32_t B, int64_t n_max_in,
                          const FwdOpts& fo, void* out, int64_t layer_stride, hipStream_t st) {
    const s3enc_byol_s_config& x = e->byol_s_cfg;
    const ByolSW& w = *e->byol_s;
    const int D = 2048, L = x.window;
    const bool resnet = x.network == S3ENC_BYOL_S_RESNETISH;
    if (fo.selection != S3ENC_SEL_HIDDEN)
        return fail("s3enc_forward: feature_selection is not defined for BYOL-S (the reference expert has one hidden_states list)");
    if (fo.featurize && !fo.w) return fail("s3enc_forward: featurize needs feat_w");
    if (!fo.featurize && fo.out_dtype != F32) return fail("s3enc_forward: out_dtype must be S3ENC_F32 for a BYOL-S handle");
    if (e->aux_codewords || e->aux_codeids) return fail("s3enc_forward_aux: codewords / codeids are outputs of a wav2vec handle with a vector quantizer");
    if (B > 65535) return fail("s3enc_forward: batch too large");
    long n_max;
    if (batch_n_max(wav_ptrs_host, lengths, B, n_max_in, n_max)) return 1;
    const long S = byol_s_num_windows(x, n_max);
    const long N = (long)B * S;
    const int T = (int)s3::melspec_num_frames(L);
    const long n_lm = N * T * 64;  // log-mel elements
    if (N > (1L << 20) || n_lm > 0x7fffffffL) return fail("s3enc_forward: batch too large");
    for (int b = 0; b < B; ++b)
        if (((uintptr_t)wav_ptrs_host[b]) & 3) return fail("s3enc_forward: utterance " + std::to_string(b) + " is not 4-byte aligned");
    if (check_out(out, fo, layer_stride, N * D)) return 1;
    DeviceGuard dg(e->device);
    if (!dg.ok) return fail("s3enc_forward: hipSetDevice failed");
    const long CH = std::min<long>(N, s3::tuning().byol_s_chunk);  // windows per pass of the network

    // ---- the window table: first sample, readable samples and leading zeros of window b * S + k ----
    const size_t ptr_bytes = (size_t)N * sizeof(const float*), tbl_bytes = ptr_bytes + 2 * (size_t)N * sizeof(int);
    HIP_TRY(e->small.ensure_on_stream(tbl_bytes + 1024, st));
    char* hp;
    if (stage_begin(e, tbl_bytes, st, hp)) return 1;
    {
        uintptr_t* hptr = (uintptr_t*)hp;
        int* hval = (int*)(hp + ptr_bytes);
        int* hlead = hval + N;
        for (int b = 0; b < B; ++b)
            for (long k = 0; k < S; ++k) {
                const long start = k * x.step - L / 2, left = (long)lengths[b] - start;  // (start < 0: the window begins in the front padding)
                const long i = b * S + k;
                const bool any = left > 0 && start + L > 0;
                hptr[i] = any ? (uintptr_t)wav_ptrs_host[b] + (uintptr_t)(start * 4) : (uintptr_t)wav_ptrs_host[b];
                hval[i] = any ? (int)(left > L ? L : left) : 0;
                hlead[i] = any && start < 0 ? (int)-start : 0;
            }
    }
    if (stage_commit(e, hp, e->small.p, tbl_bytes, st)) return 1;
    const float* const* d_ptr = (const float* const*)e->small.p;
    const int* d_val = (const int*)((char*)e->small.p + ptr_bytes);
    const int* d_lead = d_val + N;

    // ---- layer geometry of the ResNet: H = time, W = mel ----
    struct Stage {
        int H, W, C;        // the stage's output map
        float *t, *y[2], *ds;
        size_t elems;       // one bordered buffer of the chunk
    };
    Stage stg[4];
    const int Hs = (T - 1) / 2 + 1;  // behind the stem's pool; W is 32
    {
        int H = Hs, W = 32;
        for (int l = 0; l < 4; ++l) {
            if (l) {
                H = s3::conv2d_out(H, 3, 2);
                W = s3::conv2d_out(W, 3, 2);
            }
            stg[l].H = H;
            stg[l].W = W;
            stg[l].C = 64 << l;
            stg[l].elems = (size_t)CH * (H + 2) * (W + 2) * stg[l].C;
        }
    }
    const int bd = resnet ? 4 : 1;
    const size_t img_elems = (size_t)CH * (T + 2 * bd) * (64 + 2 * bd);
    const size_t map_elems = (size_t)CH * (T + 2) * 66 * 64, s0_elems = (size_t)CH * (Hs + 2) * 34 * 64;
    const size_t fin_elems = (size_t)CH * stg[3].H * stg[3].W * 512;
    const int fused = s3::tuning().stem_fused;
    if (resnet && std::max(s0_elems, fused ? s0_elems : map_elems) * 4 >= (1ul << 32) - 64)
        return fail("s3enc_forward: byol_s_chunk of " + std::to_string(CH) + " windows is too large: the stem's activation is not addressable with "
                    "32-bit offsets");

    // ---- workspace ----
    float *lm, *img, *post = nullptr, *map = nullptr, *s0 = nullptr, *fin = nullptr, *stats;
    double *part, *mean;
    ByolANet nb{};
    size_t zero_from = 0, zero_to = 0;  // the bordered buffers, zeroed once per forward: the kernels write interiors only
    for (int pass = 0; pass < 2; ++pass) {
        Bump wb(pass ? e->ws.p : nullptr);
        lm = (float*)wb.take((size_t)n_lm * 4);
        part = (double*)wb.take(NPART * sizeof(double));
        mean = (double*)wb.take(sizeof(double));
        stats = (float*)wb.take(2 * sizeof(float));
        if (fo.featurize) post = (float*)wb.take((size_t)N * D * 4);
        zero_from = wb.off;
        img = (float*)wb.take(img_elems * 4);
        if (resnet) {
            if (!fused) map = (float*)wb.take(map_elems * 4);
            s0 = (float*)wb.take(s0_elems * 4);
            for (int l = 0; l < 4; ++l) {
                stg[l].t = (float*)wb.take(stg[l].elems * 4);
                stg[l].y[0] = (float*)wb.take(stg[l].elems * 4);
                stg[l].y[1] = (float*)wb.take(stg[l].elems * 4);
            }
            zero_to = wb.off;
            for (int l = 0; l < 4; ++l) stg[l].ds = (float*)wb.take(stg[l].elems * 4);
            fin = (float*)wb.take(fin_elems * 4);
        } else {
            zero_to = wb.off;
            if (byol_a_net_plan(CH, T, D, wb, nb)) return 1;
        }
        if (!pass) HIP_TRY(e->ws.ensure_on_stream(wb.off + 4096, st));
    }
    e->taps.clear();

    Sink sink{e, st, fo.featurize ? 2 : 0, out, (long)layer_stride, F32, N, D, fo.w, fo.feat_norm};
    HIP_TRY(sink.zero_without_terms(1, N));
    HIP_TRY(hipMemsetAsync((char*)e->ws.p + zero_from, 0, zero_to - zero_from, st));

    // ---- front end: every window of the batch ----
    {
        Prof pr(e, st, "melspec:fft400", (double)N * T * 5e4, 4.0 * ((double)N * L + (double)n_lm));
        s3::MelspecParams m{};
        m.ptrs = d_ptr;
        m.valid = d_val;
        m.lead = d_lead;
        m.nseg = (int)N;
        m.L = L;
        m.mean = 0.f;
        m.std_ = 1.f;
        m.win400 = 1;
        m.out = lm;
        m.o_bs = (long)T * 64;
        m.o_row = 64;
        m.fft = 1;
        if (const char* why = s3::melspec_refusal(m)) return fail(std::string("s3enc_forward: the BYOL-S front end refuses: ") + why);
        HIP_TRY(s3::launch_melspec(m, st));
    }
    // ---- the statistics of the whole batch ----
    {
        Prof pr(e, st, "byol_s_stats", 4.0 * n_lm, 8.0 * n_lm);
        const long per = (n_lm + NPART - 1) / NPART;
        for (int pass = 0; pass < 2; ++pass) {
            hipLaunchKernelGGL(stats_partial_kernel, dim3(NPART), dim3(256), 0, st, lm, n_lm, per, pass, mean, part);
            hipLaunchKernelGGL(stats_combine_kernel, dim3(1), dim3(256), 0, st, part, n_lm, N, pass, mean, stats);
        }
        HIP_TRY(hipGetLastError());
    }
    e->taps["logmel"] = {lm, n_lm, F32};  // (B S, frames, 64), un-normalised
    e->taps["stats"] = {stats, 2, F32};   // mean / (B S), std / (B S)

    float* dst = fo.featurize ? post : sink.slot32(0);
    for (long c0 = 0; c0 < N; c0 += CH) {
        const int nbw = (int)std::min<long>(CH, N - c0);
        {
            const long n = (long)nbw * T * 64;
            Prof pr(e, st, "byol_s_normalise", 2.0 * n, 8.0 * n);
            hipLaunchKernelGGL(normalise_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, lm + c0 * T * 64, stats, n, T, bd, img,
                               (long)(T + 2 * bd) * (64 + 2 * bd));
            HIP_TRY(hipGetLastError());
        }
        if (!resnet) {
            if (byol_a_net_run(e, w.ntt, D, img, nbw, T, nb, dst + c0 * D, st)) return 1;
            continue;
        }
        {
            s3::StemParams q{};
            q.src = img;
            q.src_bs = (long)(T + 8) * 72;
            q.H = T;
            q.B = nbw;
            q.Wt = (const float*)w.stem_w.p;
            q.scale = (const float*)w.stem_s.p;
            q.shift = (const float*)w.stem_t.p;
            q.dst = s0;
            q.dst_bs = (long)(Hs + 2) * 34 * 64;
            q.fused = fused;
            q.map = map;
            q.map_bs = (long)(T + 2) * 66 * 64;
            if (const char* why = s3::stem_refusal(q)) return fail(std::string("s3enc_forward: the BYOL-S stem refuses: ") + why);
            const double px = (double)nbw * T * 64;
            Prof pr(e, st, fused ? "stem:fused" : "stem:split", 2.0 * px * 64 * 49 * (fused ? 2.25 : 1.0),
                    4.0 * (px + (fused ? 0.0 : 2.0 * px * 64) + (double)nbw * Hs * 32 * 64));
            HIP_TRY(s3::launch_stem(q, st));
        }
        const float* cur = s0;
        int H = Hs, W = 32, l = 0, in_layer = 0, flip = 0;
        for (size_t bi = 0; bi < w.blocks.size(); ++bi) {
            const ByolSBlockW& k = w.blocks[bi];
            if (in_layer == x.blocks[l]) {
                ++l;
                in_layer = 0;
                flip = 0;
            }
            const Stage& sg = stg[l];
            const bool last = bi + 1 == w.blocks.size();
            if (run_conv(e, st, nbw, {cur, H, W, k.cin, k.cout, 3, k.stride, 1, &k.w1, &k.s1, &k.t1, nullptr, 0, sg.t, 1})) return 1;
            if (k.down && run_conv(e, st, nbw, {cur, H, W, k.cin, k.cout, 1, k.stride, 0, &k.wd, &k.sd, &k.td, nullptr, 0, sg.ds, 0})) return 1;
            float* y = last ? fin : sg.y[flip];
            if (run_conv(e, st, nbw, {sg.t, sg.H, sg.W, k.cout, k.cout, 3, 1, 1, &k.w2, &k.s2, &k.t2, k.down ? sg.ds : cur, k.down ? 0 : 1, y, last ? 0 : 1}))
                return 1;
            cur = y;
            H = sg.H;
            W = sg.W;
            flip ^= 1;
            ++in_layer;
        }
        Prof pr(e, st, "byol_a_tail", 2.0 * nbw * H * D, 4.0 * ((double)nbw * H * D + (double)nbw * D));
        HIP_TRY(launch_byol_tail(fin, H, W * 512, nbw, dst + c0 * D, st));
    }
    if (sink.term(0)) {
        Prof pr(e, st, "emit_state", 0, 4.0 * N * D * 2);
        HIP_TRY(sink.emit(0, dst));
    }
    HIP_TRY(sink.done(0));
    return 0;
}

// frames: windows; valid: the utterance's own windows (the rows behind them are the reference's values, not zeros); rate:
// byol_s/expert.py:27-28, int(hop_size / 1000 * 16000)
FamilyOps kByolSFamily = {
    S3ENC_BYOL_S, "byol_s", "S3ENC_BYOL_S", "s3enc_create_byol_s", "the BYOL-S family needs its window / network block",
    "BYOL-S (one hidden_states list)",
    [](const s3enc_config& c, const void* b) { return byol_s_check_config(c, *(const s3enc_byol_s_config*)b); },
    [](s3enc_encoder* e, const Ckpt& ck, const void* b) { e->byol_s_cfg = *(const s3enc_byol_s_config*)b; return byol_s_create(e, ck); },
    byol_s_forward,
    [](const s3enc_encoder* h, long n) { return byol_s_num_windows(h->byol_s_cfg, n); },
    nullptr,
    [](const s3enc_encoder* h) { return (int)h->byol_s_cfg.step; }};

}  // namespace s3e
