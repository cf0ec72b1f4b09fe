// ops.hip — the library-level entry points that are not tied to a handle: tuning keys, the single-kernel entry points the
// op-level tests and micro-benchmarks call (s3enc_op_*), the Featurizer's weighted sum and the fbank upstream.
#include "engine_internal.h"

namespace s3 {
Tuning g_tuning;
thread_local const Tuning* t_tuning = nullptr;
thread_local int* t_status = nullptr;

int tuning_set(Tuning& t, const char* key, int value, const char** err) {
    struct Key {
        const char* name;
        int Tuning::*field;
        int lo, hi;
    };
    static const Key keys[] = {
        {"gemm_variant", &Tuning::gemm_variant, 0, 63},      {"gemm_lds_pad", &Tuning::gemm_lds_pad, 0, 120 * 1024},
        {"gemm32_big", &Tuning::gemm32_big, 0, 5},           {"gemm_x3_tile", &Tuning::gemm_x3_tile, 0, 5},
        {"gemm16_big", &Tuning::gemm16_big, 0, 10},          {"gemm16_rows", &Tuning::gemm16_rows, 0, 1},
        {"attn_lds_pad", &Tuning::attn_lds_pad, 0, 48 * 1024}, {"conv0_nt", &Tuning::conv0_nt, 0, 1},
        {"ws_inplace", &Tuning::ws_inplace, 0, 1},           {"gemm16_pp", &Tuning::gemm16_pp, 0, 3},
        {"gemm16_mx", &Tuning::gemm16_mx, 0, 31},            {"reserve_cus", &Tuning::reserve_cus, 0, 128},
        {"x3_pack_cache", &Tuning::x3_pack_cache, 0, 1},     {"gelu32", &Tuning::gelu32, 0, 1},
        {"comm_self_p2p", &Tuning::comm_self_p2p, 0, 1},     {"attn_persist", &Tuning::attn_persist, 0, 1},
        {"fp16x2_conv1_f32", &Tuning::fp16x2_conv1_f32, 0, 1}, {"gn_lag_one_block", &Tuning::gn_lag_one_block, 0, 1},
        {"ln_rows", &Tuning::ln_rows, 1, 2},                 {"ln1_fold", &Tuning::ln1_fold, 0, 1},
        {"ln_preload", &Tuning::ln_preload, 0, 1},           {"forward_chain", &Tuning::forward_chain, 0, 1},
        {"conv0_fast", &Tuning::conv0_fast, 0, 1},           {"conv_f22", &Tuning::conv_f22, 0, 1},
        {"rnn_split", &Tuning::rnn_split, -1, 8},           {"npc_skip_taps", &Tuning::npc_skip_taps, 0, 1},
        {"conv2d_n64", &Tuning::conv2d_n64, 0, 1},           {"melspec_fft", &Tuning::melspec_fft, 0, 1},
        {"patch_embed_fused", &Tuning::patch_embed_fused, 0, 1},
        {"patch_strided_fused", &Tuning::patch_strided_fused, 0, 1}, {"ssast_chunk", &Tuning::ssast_chunk, 1, 1 << 22},
        {"stem_fused", &Tuning::stem_fused, 0, 1},           {"byol_s_chunk", &Tuning::byol_s_chunk, 1, 4096},
        {"gemm32_tail", &Tuning::gemm32_tail, 0, 2},         {"gemm32_tail_units", &Tuning::gemm32_tail_units, 0, 1 << 20},
    };
    static thread_local char msg[160];
    if (!key) {
        *err = "s3enc_set_tuning: null key";
        return 1;
    }
    for (const Key& k : keys)
        if (!strcmp(key, k.name)) {
            if (value < k.lo || value > k.hi) {
                snprintf(msg, sizeof(msg), "%s must be %d..%d", k.name, k.lo, k.hi);
                *err = msg;
                return 1;
            }
            t.*(k.field) = value;
            return 0;
        }
    snprintf(msg, sizeof(msg), "s3enc_set_tuning: unknown key '%s'", key);
    *err = msg;
    return 1;
}
}  // namespace s3

extern "C" {

int s3enc_set_tuning(const char* key, int32_t value) {
    const char* err = nullptr;
    if (tuning_set(g_tuning, key, value, &err)) return fail(err);
    return 0;
}
int s3enc_set_handle_tuning(s3enc_handle h, const char* key, int32_t value) {
    if (!h) return fail("null handle");
    if (!h->has_tuning) {
        h->tun = g_tuning;  // start from the process defaults as they are now
        h->has_tuning = true;
    }
    const char* err = nullptr;
    if (tuning_set(h->tun, key, value, &err)) return fail(err);
    return 0;
}

// ---- single-kernel entry points -------------------------------------------------------------------------------
int s3enc_op_gemm(int32_t dtype, const void* A, int64_t lda, int64_t a_batch_stride, const void* W, const float* bias, int32_t M,
                  int32_t N, int32_t K, int32_t batches, int32_t act, const float* residual, const int32_t* row_limit,
                  float* out32, void* out16, int64_t ldo, int64_t o_batch_stride, void* stream) {
    GemmParams g{};
    g.A = A;
    g.lda = lda;
    g.a_bs = a_batch_stride;
    g.W = W;
    g.bias = bias;
    g.M = M;
    g.N = N;
    g.K = K;
    g.batches = batches;
    g.act = act;
    g.residual = residual;
    g.row_limit = row_limit;
    g.out32 = out32;
    g.out16 = out16;
    g.ldo = ldo;
    g.o_bs = o_batch_stride;
    if (dtype == 4) {  // S3ENC_F16X2: fp16 A, W given as (N, 2K) fp16 rows [hi(K) | lo(K)] — the contraction runs over both
        g.wsplit = 1;
        HIP_TRY(launch_gemm(F16, g, (hipStream_t)stream));
        return 0;
    }
    if (dtype == 5) {  // S3ENC_F16X2 with the lo term on the MX pipe (test / lab entry): fp16 A, W given as FP32 (N, K) on the device;
                       // the [hi | lo] rows and the MX-fp4 image are packed here exactly as s3enc_create packs them
        std::vector<float> hw((size_t)N * K);
        HIP_TRY(hipMemcpy(hw.data(), W, hw.size() * 4, hipMemcpyDeviceToHost));
        DevBuf w2;
        MxImage img;
        HIP_TRY(upload_gemm_w(w2, hw, N, K, F16, true));
        HIP_TRY(upload_mx4_lo(img, hw, N, K));
        g.W = w2.p;
        g.wsplit = 1;
        g.W4 = img.data.p;
        g.W4s = img.scales.p;
        g.mxw = 1;
        Tuning forced = tuning();
        forced.gemm16_mx = 31;  // every shape the kernel can take (the engine's default also weighs the tile rounds)
        TuningScope force(&forced);
        if (!gemm16_mx_eligible(F16, g)) return fail("s3enc_op_gemm: shape / alignment not eligible for the MX second-term kernel (K % 128, N >= 128, 16-byte rows)");
        HIP_TRY(launch_gemm(F16, g, (hipStream_t)stream));
        HIP_TRY(hipStreamSynchronize((hipStream_t)stream));  // the packed images are freed on return
        return 0;
    }
    if (dtype == 3) {  // S3ENC_F32X3: fp32 operands; W is split into its pair-packed bf16 hi / lo image here
        if (K % 32) return fail("s3enc_op_gemm: S3ENC_F32X3 needs K % 32 == 0");
        // tuning key "x3_pack_cache" (micro-benchmarks only): keep the packed image of the last (W, N, K) and skip the
        // host round trip + synchronisation when the same weight pointer comes back
        static DevBuf cached;
        static const void* cached_w = nullptr;
        static long cached_n = 0, cached_k = 0;
        if (tuning().x3_pack_cache && cached_w == W && cached_n == N && cached_k == K) {
            g.W_x3 = cached.p;
            if (!gemm_x3_eligible(g)) return fail("s3enc_op_gemm: shape / alignment not eligible for the S3ENC_F32X3 kernel");
            HIP_TRY(launch_gemm(F32, g, (hipStream_t)stream));
            return 0;
        }
        std::vector<float> hw((size_t)N * K);
        HIP_TRY(hipMemcpy(hw.data(), W, hw.size() * 4, hipMemcpyDeviceToHost));
        DevBuf w3;
        HIP_TRY(upload_x3(w3, hw, N, K));
        g.W_x3 = w3.p;
        if (!gemm_x3_eligible(g)) return fail("s3enc_op_gemm: shape / alignment not eligible for the S3ENC_F32X3 kernel");
        HIP_TRY(launch_gemm(F32, g, (hipStream_t)stream));
        HIP_TRY(hipStreamSynchronize((hipStream_t)stream));  // w3 is freed on return (or kept as the cache)
        if (tuning().x3_pack_cache) {
            HIP_TRY(hipDeviceSynchronize());
            std::swap(cached.p, w3.p);
            std::swap(cached.bytes, w3.bytes);
            cached_w = W;
            cached_n = N;
            cached_k = K;
        }
        return 0;
    }
    HIP_TRY(launch_gemm(dtype, g, (hipStream_t)stream));
    return 0;
}

// Measurement hook: `workgroups` workgroups of `threads` threads that do nothing but hold their CU slots for `milliseconds` on `stream`
// — a stand-in for the channel kernels of a collective running beside the encoder (bench.py --steal-cus; there is one GPU per box on
// this pool, so the real RCCL exchange cannot be timed against the compute it overlaps)
namespace {
__global__ void occupy_kernel(long long ticks) {
    const long long t0 = wall_clock64();
    while (wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(32);
}
}  // namespace
int s3enc_debug_occupy_cus(int32_t workgroups, int32_t threads, double milliseconds, void* stream) {
    // (the hold is bounded: a typo in `milliseconds` must not be able to hang the GPU for an arbitrary time)
    if (workgroups <= 0 || threads <= 0 || threads > 1024 || !(milliseconds >= 0) || milliseconds > 10000.0)
        return fail("s3enc_debug_occupy_cus: bad argument (workgroups > 0, 0 < threads <= 1024, 0 <= milliseconds <= 10000)");
    int dev = 0, khz = 0;
    HIP_TRY(hipGetDevice(&dev));
    if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, dev) != hipSuccess || khz <= 0) khz = 100000;  // 100 MHz
    hipLaunchKernelGGL(occupy_kernel, dim3(workgroups), dim3(threads), 0, (hipStream_t)stream, (long long)(milliseconds * khz));
    HIP_TRY(hipGetLastError());
    return 0;
}

// Measurement hook: the shader clock a timed region really ran at.  s_memtime ticks once per shader cycle, s_memrealtime at the
// constant reference rate (hipDeviceAttributeWallClockRate, 100 MHz): two samples on the SAME stream around a region give its
// average clock as d(shader) / d(reference) x rate — no concurrent probe, nothing perturbed.  Every XCD has its own counters, so the
// sample is taken by a workgroup that finds itself on XCD 0 (64 workgroups go round-robin over the 8 XCDs; the first claims).
namespace {
__global__ void clock_sample_kernel(unsigned long long* out, unsigned long long ref_khz) {
    if (threadIdx.x) return;
    const unsigned xcc = __builtin_amdgcn_s_getreg((3 << 11) | 20) & 15u;  // HW_REG_XCC_ID, bits 3:0
    if (xcc != 0) return;
    if (atomicCAS(&out[2], 0ull, ref_khz) != 0ull) return;
    out[0] = __builtin_amdgcn_s_memtime();      // shader cycles
    out[1] = __builtin_amdgcn_s_memrealtime();  // reference ticks
    __threadfence_system();
}
}  // namespace
int s3enc_debug_clock_sample(uint64_t* out3_device, void* stream) {
    if (!out3_device) return fail("s3enc_debug_clock_sample: null argument");
    int dev = 0, khz = 0;
    HIP_TRY(hipGetDevice(&dev));
    if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, dev) != hipSuccess || khz <= 0) khz = 100000;  // 100 MHz
    HIP_TRY(hipMemsetAsync(out3_device, 0, 3 * sizeof(uint64_t), (hipStream_t)stream));
    hipLaunchKernelGGL(clock_sample_kernel, dim3(64), dim3(64), 0, (hipStream_t)stream, (unsigned long long*)out3_device,
                       (unsigned long long)khz);
    HIP_TRY(hipGetLastError());
    return 0;
}

int s3enc_debug_gemm_schedule(int32_t M, int32_t N, int32_t batches, int32_t tm, int32_t tail, int32_t cus, int32_t* items4_host,
                              int64_t max_items, int64_t* n_items) {
    if (!n_items) return fail("s3enc_debug_gemm_schedule: null argument");
    if (M < 1 || N < 1 || batches < 1 || tm < 1 || tm > 4 || tail < 0 || tail > 2 || cus < 1)
        return fail("s3enc_debug_gemm_schedule: M, N, batches, cus >= 1, tm 1..4, tail 0..2");
    const GemmTileSched s = gemm_tile_schedule(M, N, batches, tm, tail, 0, cus);
    std::vector<int> items;
    gemm_tile_items(M, N, batches, s, items);
    *n_items = (int64_t)(items.size() / 4);
    if (items4_host && max_items >= *n_items) memcpy(items4_host, items.data(), items.size() * sizeof(int));
    return 0;
}

int s3enc_op_layernorm(int32_t dtype, const float* x, const float* gamma, const float* beta, int32_t rows, int32_t C, int32_t act,
                       float* out32, void* out16, void* stream) {
    HIP_TRY(launch_layernorm(dtype, x, gamma, beta, rows, C, act, out32, out16, (hipStream_t)stream));
    return 0;
}

int s3enc_op_attention(int32_t dtype, const void* qkv, void* out, const int32_t* valid, int32_t B, int32_t T, int32_t H,
                       const float* bias_table, int32_t table_R, const float* gate, void* stream) {
    if (bias_table && (table_R < 0 || T > 6000)) return fail("s3enc_op_attention: bad table_R / T > 6000 with a bias table");
    AttnParams a{};
    a.qkv = qkv;
    a.out = out;
    a.valid = valid;
    a.B = B;
    a.T = T;
    a.H = H;
    a.bias_table = bias_table;
    a.table_R = table_R;
    a.gate = gate;
    HIP_TRY(launch_attention(dtype, a, (hipStream_t)stream));
    return 0;
}

int s3enc_op_conformer_conv(const float* x, const float* taps, const float* shift, int32_t B, int32_t T, int32_t D, int32_t K,
                            float* out, void* stream) {
    if (!x || !taps || !shift || !out) return fail("s3enc_op_conformer_conv: null argument");
    if (B <= 0 || T <= 0 || D <= 0 || D % 64) return fail("s3enc_op_conformer_conv: bad shape (D % 64 == 0)");
    if (K < 1 || K > 63 || !(K & 1)) return fail("s3enc_op_conformer_conv: K must be odd and <= 63");
    ConformerConvParams p{};
    p.x = x;
    p.taps = taps;
    p.shift = shift;
    p.out = out;
    p.B = B;
    p.T = T;
    p.D = D;
    p.K = K;
    HIP_TRY(launch_conformer_conv(p, (hipStream_t)stream));
    return 0;
}

int s3enc_op_gn1_apply(const float* x, const float* gamma, const float* beta, const float* res, float scale, int32_t log_compress,
                       int32_t B, int32_t rows, int32_t C, int32_t pad, int32_t pad_zero, float* dst, float* state, float* acc,
                       float acc_w, int32_t acc_norm, int32_t acc_init, void* stream) {
    if (!x || (!dst && !state && !acc)) return fail("s3enc_op_gn1_apply: null argument");
    if (B <= 0 || rows <= 0 || C <= 0 || (C & 3) || C > 1024) return fail("s3enc_op_gn1_apply: bad shape (C % 4 == 0, C <= 1024)");
    if (pad < 0 || pad > 64 || (pad && !dst)) return fail("s3enc_op_gn1_apply: pad rows need dst (0..64)");
    hipStream_t st = (hipStream_t)stream;
    double* partial = nullptr;
    HIP_TRY(hipMalloc((void**)&partial, (size_t)B * GS_BLOCKS * 2 * sizeof(double)));
    Gn1ApplyParams p{};
    p.x = x;
    p.x_bs = (long)rows * C;
    p.partial = partial;
    p.count = (double)rows * C;
    p.gamma = gamma;
    p.beta = beta;
    p.res = res;
    p.res_bs = (long)rows * C;
    p.scale = scale;
    p.log = log_compress;
    p.B = B;
    p.rows = rows;
    p.C = C;
    p.pad = pad;
    p.pad_zero = pad_zero;
    p.dst = dst;
    p.dst_bs = (long)(pad + rows) * C;
    p.state = state;
    if (acc) {
        p.acc.acc = acc;
        p.acc.w = acc_w;
        p.acc.mode = 2;
        p.acc.norm = acc_norm;
        p.acc.init = acc_init;
    }
    hipError_t er = launch_group1_stats(x, (long)rows * C, (long)rows * C, B, partial, st);
    if (er == hipSuccess) er = launch_gn1_apply(p, st);
    const hipError_t es = hipStreamSynchronize(st);
    (void)hipFree(partial);
    HIP_TRY(er);
    HIP_TRY(es);
    return 0;
}

int s3enc_op_channelnorm_relu(const float* x, const float* gamma, const float* beta, int32_t B, int32_t rows, int32_t C, int32_t pad,
                              float* dst, float* state, void* stream) {
    if (!x || (!dst && !state)) return fail("s3enc_op_channelnorm_relu: null argument");
    if (B <= 0 || rows <= 0 || C < 8 || (C & 3) || C > 1024) return fail("s3enc_op_channelnorm_relu: bad shape (C % 4 == 0, 8 <= C <= 1024)");
    if (pad < 0 || pad > 64 || (pad && !dst)) return fail("s3enc_op_channelnorm_relu: border rows need dst (0..64)");
    ChannelNormParams p{};
    p.x = x;
    p.gamma = gamma;
    p.beta = beta;
    p.B = B;
    p.rows = rows;
    p.C = C;
    p.pad = pad;
    p.dst = dst;
    p.state = state;
    HIP_TRY(launch_channelnorm_relu(p, (hipStream_t)stream));
    return 0;
}

int s3enc_op_rnn(int32_t cell, const float* pre, const float* w_hh_host, const float* b_hn, int32_t B, int32_t T, int32_t H,
                 int64_t ld_pre, float* out, int64_t ldo, void* stream) {
    if (!pre || !w_hh_host || !out) return fail("s3enc_op_rnn: null argument");
    if (cell < 0 || cell > 1) return fail("s3enc_op_rnn: cell must be 0 (LSTM) or 1 (GRU)");
    if ((cell == 1) != (b_hn != nullptr)) return fail("s3enc_op_rnn: b_hn belongs to the GRU cell (NULL for LSTM)");
    if (B <= 0 || T <= 0) return fail("s3enc_op_rnn: bad shape");
    if (H < 64 || H % 64 || H > RNN_H_MAX) return fail("s3enc_op_rnn: H must be a multiple of 64, at most 512");
    const int G = cell == 0 ? 4 : 3;
    if (ld_pre < (int64_t)G * H || ldo < H) return fail("s3enc_op_rnn: ld_pre / ldo smaller than the row");
    std::vector<float> packed;
    pack_rnn_whh(w_hh_host, G, H, packed);
    DevBuf dw;
    HIP_TRY(upload_f32(dw, packed));
    RnnParams p{};
    p.cell = cell;
    p.pre = pre;
    p.w = (const float*)dw.p;
    p.b_hn = b_hn;
    p.B = B;
    p.T = T;
    p.H = H;
    p.ld_pre = ld_pre;
    p.out = out;
    p.ldo = ldo;
    HIP_TRY(launch_rnn(p, (hipStream_t)stream));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));  // the packed weights are freed on return
    return 0;
}

int s3enc_op_rnn_len(int32_t cell, const float* pre, const float* w_hh_host, const float* b_hn, const int32_t* len_host,
                     const float* res, int64_t ld_res, int32_t B, int32_t T, int32_t H, int64_t ld_pre, float* out, int64_t ldo,
                     void* stream) {
    if (!pre || !w_hh_host || !out || !len_host) return fail("s3enc_op_rnn_len: null argument");
    if (cell < 0 || cell > 1) return fail("s3enc_op_rnn_len: cell must be 0 (LSTM) or 1 (GRU)");
    if ((cell == 1) != (b_hn != nullptr)) return fail("s3enc_op_rnn_len: b_hn belongs to the GRU cell (NULL for LSTM)");
    if (B <= 0 || T <= 0) return fail("s3enc_op_rnn_len: bad shape");
    if (H < 64 || H % 64 || H > RNN_H_MAX) return fail("s3enc_op_rnn_len: H must be a multiple of 64, at most 512");
    const int G = cell == 0 ? 4 : 3;
    if (ld_pre < (int64_t)G * H || ldo < H) return fail("s3enc_op_rnn_len: ld_pre / ldo smaller than the row");
    if (res && ld_res < H) return fail("s3enc_op_rnn_len: ld_res smaller than the row");
    if ((((uintptr_t)out) & 15) || (ldo & 3)) return fail("s3enc_op_rnn_len: out must be 16-byte aligned and ldo a multiple of 4");
    for (int b = 0; b < B; ++b)
        if (len_host[b] < 1 || len_host[b] > T) return fail("s3enc_op_rnn_len: every length must be in 1..T");
    std::vector<float> packed;
    pack_rnn_whh(w_hh_host, G, H, packed);
    DevBuf dw, dl;
    HIP_TRY(upload_f32(dw, packed));
    HIP_TRY(dl.ensure((size_t)B * sizeof(int)));
    HIP_TRY(hipMemcpy(dl.p, len_host, (size_t)B * sizeof(int), hipMemcpyHostToDevice));
    RnnLenParams p{};
    p.cell = cell;
    p.pre = pre;
    p.w = (const float*)dw.p;
    p.b_hn = b_hn;
    p.B = B;
    p.T = T;
    p.H = H;
    p.ld_pre = ld_pre;
    p.out = out;
    p.ldo = ldo;
    p.len = (const int*)dl.p;
    p.res = res;
    p.ld_res = ld_res;
    const int S = rnn_split_pick(cell, H, B);
    if (S) {  // the step-split form (tuning key rnn_split, or its default rule)
        if (!rnn_split_ok(H, B, S)) return fail("s3enc_op_rnn_len: rnn_split must be a power of two with H / S a multiple of 64 and S * B <= 256");
        DevBuf dh, dc;
        HIP_TRY(dh.ensure((size_t)2 * B * H * sizeof(float)));
        if (cell == 0) HIP_TRY(dc.ensure((size_t)B * H * sizeof(float)));
        RnnStepParams q{};
        static_cast<RnnLenParams&>(q) = p;
        q.S = S;
        q.max_len = *std::max_element(len_host, len_host + B);
        q.hbuf = (float*)dh.p;
        q.cbuf = (float*)dc.p;
        HIP_TRY(launch_rnn_step(q, (hipStream_t)stream));
        HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
        return 0;
    }
    HIP_TRY(launch_rnn_len(p, (hipStream_t)stream));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));  // the packed weights and the lengths are freed on return
    return 0;
}

int s3enc_pack_lstm_bidir_whh(const float* w_hh_host, int32_t H, float* out_host) {
    if (!w_hh_host || !out_host) return fail("s3enc_pack_lstm_bidir_whh: null argument");
    if (H < 64 || H % 64 || H > RNNB_H_MAX) return fail("s3enc_pack_lstm_bidir_whh: H must be a multiple of 64, at most 1024");
    std::vector<float> packed;
    pack_rnnb_whh(w_hh_host, H, packed);
    std::copy(packed.begin(), packed.end(), out_host);
    return 0;
}

int s3enc_op_lstm_bidir(const float* pre_fwd, const float* pre_bwd, const float* w_hh_fwd_host, const float* w_hh_bwd_host,
                        const int32_t* len_host, int32_t B, int32_t T, int32_t H, int64_t ld_pre, float* out, int64_t ldo, void* stream) {
    if (!pre_fwd || !pre_bwd || !w_hh_fwd_host || !w_hh_bwd_host || !len_host || !out) return fail("s3enc_op_lstm_bidir: null argument");
    if (B <= 0 || T <= 0) return fail("s3enc_op_lstm_bidir: bad shape");
    RnnbParams p{};
    p.pre_fwd = pre_fwd;
    p.pre_bwd = pre_bwd;
    p.B = B;
    p.T = T;
    p.H = H;
    p.ld_pre = ld_pre;
    p.out = out;
    p.ldo = ldo;
    // the checks that need no device memory first: placeholders stand in for the buffers allocated below
    alignas(16) static float stand_in[4];
    p.w_fwd = p.w_bwd = stand_in;
    p.len = (const int*)len_host;
    p.hbuf = p.cbuf = stand_in;
    if (const char* why = rnnb_refusal(p)) return fail(std::string("s3enc_op_lstm_bidir: ") + why);
    for (int b = 0; b < B; ++b)
        if (len_host[b] < 1 || len_host[b] > T) return fail("s3enc_op_lstm_bidir: every length must be in 1..T");
    std::vector<float> packed;
    DevBuf dwf, dwb, dl, dh, dc;
    pack_rnnb_whh(w_hh_fwd_host, H, packed);
    HIP_TRY(upload_f32(dwf, packed));
    pack_rnnb_whh(w_hh_bwd_host, H, packed);
    HIP_TRY(upload_f32(dwb, packed));
    HIP_TRY(dl.ensure((size_t)B * sizeof(int)));
    HIP_TRY(hipMemcpy(dl.p, len_host, (size_t)B * sizeof(int), hipMemcpyHostToDevice));
    HIP_TRY(dh.ensure(2 * rnnb_state_elems(B, H) * sizeof(float)));
    HIP_TRY(dc.ensure(rnnb_state_elems(B, H) * sizeof(float)));
    p.w_fwd = (const float*)dwf.p;
    p.w_bwd = (const float*)dwb.p;
    p.len = (const int*)dl.p;
    p.hbuf = (float*)dh.p;
    p.cbuf = (float*)dc.p;
    p.max_len = *std::max_element(len_host, len_host + B);
    if (const char* why = rnnb_refusal(p)) return fail(std::string("s3enc_op_lstm_bidir: ") + why);
    HIP_TRY(launch_rnnb(p, (hipStream_t)stream));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));  // the packed weights, the lengths and the state are freed on return
    return 0;
}

int s3enc_op_conv_taps(const float* x, const float* w_host, const float* bias, int32_t B, int32_t T, int32_t C, int32_t N, int32_t k,
                       int32_t mask, int32_t act, const float* res, int64_t ld_res, float* dst, int32_t dst_pad, int64_t ldo,
                       float* state, float* sum, int32_t sum_init, int32_t dense, void* stream) {
    if (!x || !w_host) return fail("s3enc_op_conv_taps: null argument");
    if (!dst && !state && !sum) return fail("s3enc_op_conv_taps: no destination (dst, state and sum are all null)");
    if (B <= 0 || T <= 0 || C <= 0 || N <= 0) return fail("s3enc_op_conv_taps: bad shape");
    if (k < 1 || !(k & 1) || k > 63) return fail("s3enc_op_conv_taps: k must be odd, at most 63");
    if (mask < 0 || (mask && !(mask & 1))) return fail("s3enc_op_conv_taps: mask must be 0 or odd");
    if (mask >= k) return fail("s3enc_op_conv_taps: the mask leaves no tap");
    if (dst && (dst_pad < 0 || ldo < N)) return fail("s3enc_op_conv_taps: dst needs dst_pad >= 0 and ldo >= N");
    if (res && ld_res < N) return fail("s3enc_op_conv_taps: ld_res < N");
    const int P = (k - 1) / 2, head = (k - mask) / 2;
    ConvTapsParams p{};
    p.src = x;
    p.src_bs = (long)(T + 2 * P) * C;
    p.C = C;
    p.bias = bias;
    p.T = T;
    p.N = N;
    p.B = B;
    p.taps0 = (dense || !mask) ? k : head;
    p.gap = (dense || !mask) ? 0 : mask;
    p.taps1 = (dense || !mask) ? 0 : k - head - mask;
    p.act = act;
    p.res = res;
    p.res_bs = res ? (long)T * ld_res : 0;
    p.ld_res = res ? ld_res : 0;
    p.dst = dst ? dst + (long)dst_pad * ldo : nullptr;
    p.dst_bs = dst ? (long)(T + 2 * dst_pad) * ldo : 0;
    p.ld_dst = dst ? ldo : 0;
    p.state = state;
    p.state_bs = state ? (long)T * N : 0;
    p.ld_state = state ? N : 0;
    p.sum = sum;
    p.sum_bs = sum ? (long)T * N : 0;
    p.ld_sum = sum ? N : 0;
    p.sum_init = sum_init;
    alignas(16) static float stand_in[4];  // the checks that need no device memory first
    p.W = stand_in;
    if (const char* why = conv_taps_refusal(p)) return fail(std::string("s3enc_op_conv_taps: ") + why);
    std::vector<float> packed;
    pack_conv_taps(w_host, N, C, k, mask, dense != 0, packed);
    DevBuf dw;
    HIP_TRY(upload_f32(dw, packed));
    p.W = (const float*)dw.p;
    HIP_TRY(launch_conv_taps(p, (hipStream_t)stream));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));  // the packed weights are freed on return
    return 0;
}

int s3enc_op_conv_k3s2(const float* x, int64_t x_bs, const float* w_host, const float* bias, const int32_t* row_limit, int32_t B, int32_t M,
                       int32_t C, int32_t act, float* out, int64_t o_bs, void* stream) {
    if (!x || !w_host || !out) return fail("s3enc_op_conv_k3s2: null argument");
    if (B <= 0 || M <= 0 || C <= 0) return fail("s3enc_op_conv_k3s2: bad shape");
    if (act < 0 || act > 1) return fail("s3enc_op_conv_k3s2: act must be 0 (none) or 1 (GELU)");
    ConvF22Params p{};
    p.x = x;
    p.x_bs = x_bs;
    p.bias = bias;
    p.M = M;
    p.C = C;
    p.batches = B;
    p.act = act;
    p.row_limit = row_limit;
    p.out = out;
    p.o_bs = o_bs;
    alignas(16) static float stand_in[4];  // the checks that need no device memory first
    p.W = p.WP = stand_in;
    if (const char* why = conv_f22_refusal(p)) return fail(std::string("s3enc_op_conv_k3s2: ") + why);
    if (((uintptr_t)row_limit) & 3) return fail("s3enc_op_conv_k3s2: row_limit must be 4-byte aligned");
    std::vector<float> w(w_host, w_host + (size_t)C * C * 3), packed, wp;
    pack_conv_f22(w, C, packed, wp);
    DevBuf dw, dwp;
    HIP_TRY(upload_f32(dw, packed));
    HIP_TRY(upload_f32(dwp, wp));
    p.W = (const float*)dw.p;
    p.WP = (const float*)dwp.p;
    HIP_TRY(launch_conv_f22(p, (hipStream_t)stream));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));  // the packed weights are freed on return
    return 0;
}

int s3enc_op_conv2d3x3(const float* x, const float* w_host, const float* bias, int32_t B, int32_t H, int32_t W, int32_t C, int32_t N,
                       int32_t act, int32_t pool, float* dst, int32_t dst_pad, int64_t ldo, void* stream) {
    if (!x || !w_host || !dst) return fail("s3enc_op_conv2d3x3: null argument");
    if (B <= 0 || H <= 0 || W <= 0 || C <= 0 || N <= 0) return fail("s3enc_op_conv2d3x3: bad shape");
    if (H > 32768 || W > 32768 || B > (1 << 24)) return fail("s3enc_op_conv2d3x3: bad shape");
    Conv2dParams p{};
    p.src = x;
    p.src_bs = (long)(H + 2) * (W + 2) * C;
    p.C = C;
    p.bias = bias;
    p.H = H;
    p.W = W;
    p.N = N;
    p.B = B;
    p.act = act;
    p.pool = pool;
    p.dst = dst;
    p.dst_pad = dst_pad;
    p.ld_dst = ldo;
    {
        const long Ho = pool == 1 ? H / 2 : H, Wo = pool == 1 ? W / 2 : W;
        p.dst_bs = (Ho + 2 * (long)dst_pad) * (Wo + 2 * (long)dst_pad) * ldo;
    }
    alignas(16) static float stand_in[4];  // the checks that need no device memory first
    p.Wt = stand_in;
    if (const char* why = conv2d3x3_refusal(p)) return fail(std::string("s3enc_op_conv2d3x3: ") + why);
    std::vector<float> packed;
    pack_conv2d3x3(w_host, N, C, packed);
    DevBuf dw;
    HIP_TRY(upload_f32(dw, packed));
    p.Wt = (const float*)dw.p;
    HIP_TRY(launch_conv2d3x3(p, (hipStream_t)stream));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));  // the packed weights are freed on return
    return 0;
}

int s3enc_op_conv2d3x3_affine(const float* x, const float* w_host, const float* bias, const float* scale, const float* shift, int32_t B,
                              int32_t H, int32_t W, int32_t C, int32_t N, int32_t act, int32_t pool, int32_t pool_floor, float* dst,
                              int32_t dst_pad, int64_t ldo, void* stream) {
    if (!x || !w_host || !dst) return fail("s3enc_op_conv2d3x3_affine: null argument");
    if (B <= 0 || H <= 0 || W <= 0 || C <= 0 || N <= 0) return fail("s3enc_op_conv2d3x3_affine: bad shape");
    if (H > 32768 || W > 32768 || B > (1 << 24)) return fail("s3enc_op_conv2d3x3_affine: bad shape");
    Conv2dParams p{};
    p.src = x;
    p.src_bs = (long)(H + 2) * (W + 2) * C;
    p.C = C;
    p.bias = bias;
    p.scale = scale;
    p.shift = shift;
    p.H = H;
    p.W = W;
    p.N = N;
    p.B = B;
    p.act = act;
    p.pool = pool;
    p.pool_floor = pool_floor;
    p.n64 = 1;
    p.dst = dst;
    p.dst_pad = dst_pad;
    p.ld_dst = ldo;
    {
        const long Ho = pool == 1 ? H / 2 : H, Wo = pool == 1 ? W / 2 : W;
        p.dst_bs = (Ho + 2 * (long)dst_pad) * (Wo + 2 * (long)dst_pad) * ldo;
    }
    alignas(16) static float stand_in[4];  // the checks that need no device memory first
    p.Wt = stand_in;
    if (const char* why = conv2d3x3_refusal(p)) return fail(std::string("s3enc_op_conv2d3x3_affine: ") + why);
    std::vector<float> packed;
    pack_conv2d3x3(w_host, N, C, packed);
    DevBuf dw;
    HIP_TRY(upload_f32(dw, packed));
    p.Wt = (const float*)dw.p;
    HIP_TRY(launch_conv2d3x3(p, (hipStream_t)stream));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));  // the packed weights are freed on return
    return 0;
}

// the two front-end entries: BYOL-A's (hann(1024), its precomputed statistics) and BYOL-S's (hann(400) in 1024, un-normalised)
static int op_melspec(const std::string& who, int win400, float mean, float std_, const float* segments, int32_t nseg, int32_t L, float* out,
                      float* power, void* stream) {
    if (!segments || !out) return fail(who + ": null argument");
    if (nseg <= 0 || nseg > 65535) return fail(who + ": nseg must be 1..65535");
    MelspecParams p{};
    p.nseg = nseg;
    p.L = L;
    p.mean = mean;
    p.std_ = std_;
    p.win400 = win400;
    p.out = out;
    p.o_row = 64;
    p.o_bs = melspec_num_frames(L > 0 ? L : 0) * 64;
    p.power = power;
    p.fft = win400 ? 1 : tuning().melspec_fft;
    static const float* const stand_in_ptr = nullptr;
    static const int stand_in_val = 0;
    p.ptrs = &stand_in_ptr;  // the checks that need no device memory first
    p.valid = &stand_in_val;
    p.sig = p.spec = out;
    if (const char* why = melspec_refusal(p)) return fail(who + ": " + why);
    std::vector<const float*> hp(nseg);
    std::vector<int> hv(nseg, L);
    for (int i = 0; i < nseg; ++i) hp[i] = segments + (size_t)i * L;
    DevBuf dp, dv, dsig, dspec;
    HIP_TRY(dp.ensure(hp.size() * sizeof(const float*)));
    HIP_TRY(dv.ensure(hv.size() * sizeof(int)));
    HIP_TRY(hipMemcpy(dp.p, hp.data(), hp.size() * sizeof(const float*), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dv.p, hv.data(), hv.size() * sizeof(int), hipMemcpyHostToDevice));
    p.ptrs = (const float* const*)dp.p;
    p.valid = (const int*)dv.p;
    p.sig = p.spec = nullptr;
    if (!p.fft) {
        HIP_TRY(dsig.ensure(melspec_sig_elems(nseg, L) * 4 + 64));
        HIP_TRY(dspec.ensure(melspec_spec_elems(nseg, L) * 4 + 64));
        p.sig = (float*)dsig.p;
        p.spec = (float*)dspec.p;
    }
    HIP_TRY(launch_melspec(p, (hipStream_t)stream));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));  // the tables and the scratch are freed on return
    return 0;
}

int s3enc_op_melspec1024(const float* segments, int32_t nseg, int32_t L, float* out, float* power, void* stream) {
    return op_melspec("s3enc_op_melspec1024", 0, -5.4919195f, 5.0389895f, segments, nseg, L, out, power, stream);
}

int s3enc_op_melspec400(const float* segments, int32_t nseg, int32_t L, float* out, float* power, void* stream) {
    return op_melspec("s3enc_op_melspec400", 1, 0.f, 1.f, segments, nseg, L, out, power, stream);
}

int s3enc_op_conv2d_res(const float* x, const float* w_host, const float* bias, const float* scale, const float* shift, const float* res,
                        int32_t B, int32_t H, int32_t W, int32_t C, int32_t N, int32_t k, int32_t stride, int32_t act, float* dst,
                        int32_t dst_pad, int64_t ldo, void* stream) {
    if (!x || !w_host || !dst) return fail("s3enc_op_conv2d_res: null argument");
    if (B <= 0 || H <= 0 || W <= 0 || C <= 0 || N <= 0) return fail("s3enc_op_conv2d_res: bad shape");
    if (H > 32768 || W > 32768 || B > (1 << 24)) return fail("s3enc_op_conv2d_res: bad shape");
    Conv2dParams p{};
    p.src = x;
    p.src_bs = (long)(H + 2) * (W + 2) * C;
    p.C = C;
    p.bias = bias;
    p.scale = scale;
    p.shift = shift;
    p.H = H;
    p.W = W;
    p.N = N;
    p.B = B;
    p.act = act;
    p.n64 = 1;
    p.gen = 1;
    p.k = k;
    p.stride = stride;
    p.dst = dst;
    p.dst_pad = dst_pad;
    p.ld_dst = ldo;
    alignas(16) static float stand_in[4];  // the checks that need no device memory first
    p.Wt = stand_in;
    if ((k == 1 || k == 3) && (stride == 1 || stride == 2)) {
        const long Ho = conv2d_out(H, k, stride), Wo = conv2d_out(W, k, stride);
        p.dst_bs = (Ho + 2 * (long)dst_pad) * (Wo + 2 * (long)dst_pad) * ldo;
        p.res = res;  // a plain contiguous (B, Ho, Wo, N) tensor
        p.res_bs = Ho * Wo * N;
        p.ld_res = N;
    }
    if (const char* why = conv2d3x3_refusal(p)) return fail(std::string("s3enc_op_conv2d_res: ") + why);
    std::vector<float> packed;
    if (k == 3)
        pack_conv2d3x3(w_host, N, C, packed);
    else
        packed.assign(w_host, w_host + (size_t)N * C);  // nn.Conv2d's (N, C, 1, 1) is the kernel's (N, C)
    DevBuf dw;
    HIP_TRY(upload_f32(dw, packed));
    p.Wt = (const float*)dw.p;
    HIP_TRY(launch_conv2d3x3(p, (hipStream_t)stream));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));  // the packed weights are freed on return
    return 0;
}

int s3enc_op_stem7x7_pool(const float* x, const float* w_host, const float* scale, const float* shift, int32_t B, int32_t H, int32_t fused,
                          float* dst, float* map, void* stream) {
    if (!x || !w_host || !scale || !shift || !dst) return fail("s3enc_op_stem7x7_pool: null argument");
    if (B <= 0 || H <= 0 || H > 32768 || B > (1 << 20)) return fail("s3enc_op_stem7x7_pool: bad shape");
    StemParams p{};
    p.src = x;
    p.src_bs = (long)(H + 8) * 72;
    p.H = H;
    p.B = B;
    p.scale = scale;
    p.shift = shift;
    p.dst = dst;
    p.dst_bs = (long)((H - 1) / 2 + 3) * 34 * 64;
    p.fused = fused;
    p.map = map;
    p.map_bs = (long)(H + 2) * 66 * 64;
    alignas(16) static float stand_in[4];  // the checks that need no device memory first
    p.Wt = stand_in;
    if (const char* why = stem_refusal(p)) return fail(std::string("s3enc_op_stem7x7_pool: ") + why);
    std::vector<float> packed;
    pack_stem7x7(w_host, packed);
    DevBuf dw;
    HIP_TRY(upload_f32(dw, packed));
    p.Wt = (const float*)dw.p;
    HIP_TRY(launch_stem(p, (hipStream_t)stream));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));  // the packed weights are freed on return
    return 0;
}

int s3enc_op_patch_embed(const float* img, int64_t img_bs, const float* w_host, const float* bias, const float* pos, const int32_t* kv,
                         int32_t B, int32_t Tt, int32_t kt, int32_t kc, int32_t N, float* out, void* stream) {
    if (!img || !w_host || !out) return fail("s3enc_op_patch_embed: null argument");
    if (B <= 0 || Tt <= 0 || N <= 0) return fail("s3enc_op_patch_embed: bad shape");
    PatchEmbedParams p{};
    p.img = img;
    p.img_bs = img_bs;
    p.bias = bias;
    p.pos = pos;
    p.kv = kv;
    p.B = B;
    p.Tt = Tt;
    p.kt = kt;
    p.kc = kc;
    p.N = N;
    p.out = out;
    patch_embed_geometry(p);
    alignas(16) static float stand_in[4];  // the checks that need no device memory first
    p.W = stand_in;
    if (const char* why = patch_embed_refusal(p)) return fail(std::string("s3enc_op_patch_embed: ") + why);
    std::vector<float> w(w_host, w_host + (size_t)N * kt * kc);
    DevBuf dw, rows;
    HIP_TRY(upload_f32(dw, w));
    p.W = (const float*)dw.p;
    if (tuning().patch_embed_fused) {
        HIP_TRY(launch_patch_embed(p, (hipStream_t)stream));
    } else {
        HIP_TRY(rows.ensure(patch_embed_rows_elems(p) * 4 + 64));
        HIP_TRY(launch_patch_embed_two_step(p, (float*)rows.p, (hipStream_t)stream));
    }
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));  // the weights and the gathered rows are freed on return
    return 0;
}

int s3enc_op_patch_embed_strided(const float* img, int64_t img_bs, const float* w_host, const float* bias, const float* pos,
                                 const float* prefix, int32_t nwin, int32_t rows, int32_t fshape, int32_t tshape, int32_t fstride,
                                 int32_t tstride, int32_t N, int32_t tile_rows, float* out, void* stream) {
    if (!img || !w_host || !out) return fail("s3enc_op_patch_embed_strided: null argument");
    if (nwin <= 0 || rows <= 0 || N <= 0) return fail("s3enc_op_patch_embed_strided: bad shape");
    if (tile_rows != 0 && tile_rows != 64 && tile_rows != 128) return fail("s3enc_op_patch_embed_strided: tile_rows must be 0, 64 or 128");
    PatchStridedParams p{};
    p.img = img;
    p.img_bs = img_bs;
    p.bias = bias;
    p.pos = pos;
    p.prefix = prefix;
    p.nwin = nwin;
    p.rows = rows;
    p.fshape = fshape;
    p.tshape = tshape;
    p.fstride = fstride;
    p.tstride = tstride;
    p.N = N;
    p.out = out;
    patch_strided_geometry(p);
    alignas(16) static float stand_in[4];  // the checks that need no device memory first
    p.W = stand_in;
    if (const char* why = patch_strided_refusal(p)) return fail(std::string("s3enc_op_patch_embed_strided: ") + why);
    std::vector<float> w(w_host, w_host + (size_t)N * tshape * fshape);
    DevBuf dw, gathered;
    HIP_TRY(upload_f32(dw, w));
    p.W = (const float*)dw.p;
    if (tuning().patch_strided_fused) {
        HIP_TRY(tile_rows ? launch_patch_strided_tile(p, tile_rows, (hipStream_t)stream) : launch_patch_strided(p, (hipStream_t)stream));
    } else {
        HIP_TRY(gathered.ensure(patch_strided_rows_elems(p) * 4 + 64));
        HIP_TRY(launch_patch_strided_two_step(p, (float*)gathered.p, (hipStream_t)stream));
    }
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));  // the weights and the gathered rows are freed on return
    return 0;
}

int s3enc_op_argmax_gather(const float* scores, const float* table, int32_t shared, int64_t rows, int32_t G, int32_t V, int32_t Dv,
                           int64_t* ids, float* out, void* stream) {
    if (!scores || (!ids && !out) || (out && !table)) return fail("s3enc_op_argmax_gather: null argument");
    if (rows <= 0 || G <= 0 || V <= 0 || Dv <= 0) return fail("s3enc_op_argmax_gather: bad shape");
    ArgmaxGatherParams p{};
    p.scores = scores;
    p.table = table;
    p.shared = shared;
    p.rows = rows;
    p.G = G;
    p.V = V;
    p.Dv = Dv;
    p.ids = (long long*)ids;
    p.out = out;
    HIP_TRY(launch_argmax_gather(p, (hipStream_t)stream));
    return 0;
}

int s3enc_op_relpos_attention(const float* qkv, float* out, const int32_t* valid, int32_t B, int32_t T, int32_t H, const float* P,
                              const float* qadd, void* stream) {
    if (!qkv || !out || !valid || !P || !qadd) return fail("s3enc_op_relpos_attention: null argument");
    if (B <= 0 || T <= 0 || H <= 0) return fail("s3enc_op_relpos_attention: bad shape");
    AttnParams a{};
    a.qkv = qkv;
    a.out = out;
    a.valid = valid;
    a.B = B;
    a.T = T;
    a.H = H;
    a.rel_P = P;
    a.rel_qadd = qadd;
    HIP_TRY(launch_attention(F32, a, (hipStream_t)stream));
    return 0;
}

int s3enc_op_conv0(int32_t dtype, const float* const* wavs, const int64_t* lengths, int32_t B, int64_t n_max, int32_t normalize,
                   const float* w0, const float* bias, const float* gn_gamma, const float* gn_beta, const float* ln_gamma,
                   const float* ln_beta, int32_t C, int32_t stride, void* out, void* stream) {
    if (!wavs || !lengths || !w0 || !out) return fail("s3enc_op_conv0: null argument");
    if (B <= 0 || C <= 0 || (C % 32) || C > 1024 || stride <= 0) return fail("s3enc_op_conv0: bad shape");
    if (dtype < 0 || dtype > 2) return fail("s3enc_op_conv0: dtype must be S3ENC_F32 / BF16 / F16");
    if ((gn_gamma != nullptr) == (ln_gamma != nullptr)) return fail("s3enc_op_conv0: pass exactly one of gn_gamma / ln_gamma");
    const int k0 = 10;
    long nm = 0;
    for (int b = 0; b < B; ++b) nm = lengths[b] > nm ? lengths[b] : nm;
    if (n_max > 0 && n_max < nm) return fail("s3enc_op_conv0: n_max is smaller than the longest utterance");
    if (n_max > 0) nm = n_max;
    if (nm < k0) return fail("s3enc_op_conv0: input shorter than the kernel");
    const long L0 = (nm - k0) / stride + 1;
    hipStream_t st = (hipStream_t)stream;
    // scratch: table (ptrs, lens), per-utterance norm, per-(b, c) GroupNorm affine, reduction partials
    const size_t tbl = (size_t)B * 16, part = stats_partial_elems(B, nm);
    DevBuf buf;
    Bump sz(nullptr);
    sz.take(tbl);
    sz.take((size_t)B * sizeof(float2));
    sz.take((size_t)B * C * sizeof(float2));
    sz.take(part * 8);
    HIP_TRY(buf.ensure(sz.off + 256));
    Bump bb(buf.p);
    char* d_tbl = (char*)bb.take(tbl);
    float2* d_norm = (float2*)bb.take((size_t)B * sizeof(float2));
    float2* d_gn = (float2*)bb.take((size_t)B * C * sizeof(float2));
    double* d_part = (double*)bb.take(part * 8);
    std::vector<char> host(tbl);
    memcpy(host.data(), wavs, (size_t)B * 8);
    for (int b = 0; b < B; ++b) ((long*)(host.data() + (size_t)B * 8))[b] = (long)lengths[b];
    HIP_TRY(hipMemcpy(d_tbl, host.data(), tbl, hipMemcpyHostToDevice));
    WavTable wt{(const float* const*)d_tbl, (const long*)(d_tbl + (size_t)B * 8), B, nm};
    HIP_TRY(launch_wav_norm_stats(wt, normalize, d_part, d_norm, st));
    if (gn_gamma) HIP_TRY(launch_gn_stats(wt, d_norm, w0, gn_gamma, gn_beta, C, k0, stride, L0, d_part, nullptr, d_gn, st));
    Conv0Params p{};
    p.wav = wt;
    p.norm = d_norm;
    p.w0 = w0;
    p.bias = bias;
    p.gn = gn_gamma ? d_gn : nullptr;
    p.ln_g = ln_gamma;
    p.ln_b = ln_beta;
    p.C = C;
    p.k0 = k0;
    p.s0 = stride;
    p.L0 = L0;
    p.out = out;
    HIP_TRY(launch_conv0(dtype, p, st));
    HIP_TRY(hipStreamSynchronize(st));  // the scratch is freed on return
    return 0;
}

int s3enc_op_wavlm_gate(const float* x, const float* grep_w, const float* grep_b, const float* grep_a, int32_t B, int32_t T,
                        int32_t H, float* gate, void* stream) {
    if (!x || !grep_w || !grep_b || !grep_a || !gate) return fail("s3enc_op_wavlm_gate: null argument");
    if (B <= 0 || T <= 0 || H <= 0) return fail("s3enc_op_wavlm_gate: bad shape");
    HIP_TRY(launch_wavlm_gate(x, grep_w, grep_b, grep_a, B, T, H, gate, (hipStream_t)stream));
    return 0;
}

}  // extern "C"

// the body of both positional-conv entries; `narrow`: the entry of the group widths 24 and 40 (s3enc_op_posconv_narrow)
static int op_posconv(const char* entry, bool narrow, int32_t dtype, const float* x, const float* w_host, const float* bias, int32_t B,
                      int32_t T, int32_t D, int32_t G, int32_t K, float* out, void* stream) {
    const std::string who = std::string(entry) + ": ";
    if (!x || !w_host || !bias || !out) return fail(who + "null argument");
    if (G <= 0 || D % G) return fail(who + "D must be a multiple of groups");
    const int Dg = D / G;
    if (narrow) {
        if (Dg != 24 && Dg != 40) return fail(who + "D / groups must be 24 or 40 (s3enc_op_posconv runs 32, 48 and 64)");
        if (dtype != F32) return fail(who + "group width " + std::to_string(Dg) + " is built for fp32 only (the 16-bit and fp32x3 kernel is not built at 24 and 40)");
    } else if (Dg != 32 && Dg != 48 && Dg != 64) {
        return fail(who + "D / groups must be 32, 48 or 64 (24 and 40, fp32 only: s3enc_op_posconv_narrow)");
    }
    std::vector<float> w(w_host, w_host + (size_t)D * Dg * K), packed;
    DevBuf dw;
    if (dtype == 3) {
        HIP_TRY(upload_posconv_x3(dw, w, D, G, K));
    } else {
        pack_posconv(w, D, G, K, dtype, packed);
        HIP_TRY(upload_cvt(dw, packed, dtype));
    }
    PosConvParams p{};
    p.x = x;
    p.w = dw.p;
    p.bias = bias;
    p.out = out;
    p.B = B;
    p.T = T;
    p.D = D;
    p.G = G;
    p.K = K;
    HIP_TRY(dtype == F32 ? launch_posconv(p, (hipStream_t)stream) : launch_posconv16(dtype, p, (hipStream_t)stream));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));  // the packed weights are freed on return
    return 0;
}

extern "C" {

int s3enc_op_posconv(int32_t dtype, const float* x, const float* w_host, const float* bias, int32_t B, int32_t T, int32_t D,
                     int32_t G, int32_t K, float* out, void* stream) {
    return op_posconv("s3enc_op_posconv", false, dtype, x, w_host, bias, B, T, D, G, K, out, stream);
}

int s3enc_op_posconv_narrow(int32_t dtype, const float* x, const float* w_host, const float* bias, int32_t B, int32_t T, int32_t D,
                            int32_t G, int32_t K, float* out, void* stream) {
    return op_posconv("s3enc_op_posconv_narrow", true, dtype, x, w_host, bias, B, T, D, G, K, out, stream);
}

int s3enc_weighted_sum(const float* hs, int64_t layer_stride, int32_t L, const float* w, int32_t normalize, int64_t rows, int32_t D,
                       float* out, void* stream) {
    if (!hs || !w || !out) return fail("s3enc_weighted_sum: null argument");
    if (L <= 0 || L > S3_WS_MAX_LAYERS) return fail("s3enc_weighted_sum: 1..32 layers");
    if (D <= 0 || (D & 3) || D > 2048) return fail("s3enc_weighted_sum: D must be a multiple of 4, <= 2048");
    HIP_TRY(launch_weighted_sum(hs, layer_stride, L, w, normalize, rows, D, out, (hipStream_t)stream));
    return 0;
}

int64_t s3enc_weighted_sum_backward_scratch(int64_t rows, int32_t L) {
    return rows > 0 && L > 0 ? (int64_t)weighted_sum_bwd_blocks(rows) * L : 0;
}

int s3enc_weighted_sum_backward(const float* hs, int64_t layer_stride, int32_t L, int32_t normalize, int64_t rows, int32_t D,
                                const float* grad_out, float* grad_w, double* scratch, void* stream) {
    if (!hs || !grad_out || !grad_w || !scratch) return fail("s3enc_weighted_sum_backward: null argument");
    if (L <= 0 || L > S3_WS_MAX_LAYERS) return fail("s3enc_weighted_sum_backward: 1..32 layers");
    if (D <= 0 || (D & 3) || D > 2048) return fail("s3enc_weighted_sum_backward: D must be a multiple of 4, <= 2048");
    if (rows <= 0) return fail("s3enc_weighted_sum_backward: no rows");
    HIP_TRY(launch_weighted_sum_bwd(hs, layer_stride, L, normalize, rows, D, grad_out, scratch, grad_w, (hipStream_t)stream));
    return 0;
}

static FbankParams fbank_params(const s3enc_fbank_config* c) {
    FbankParams f;
    f.sample_rate = c->sample_rate;
    f.num_mel_bins = c->num_mel_bins;
    f.frame_length_ms = c->frame_length_ms;
    f.frame_shift_ms = c->frame_shift_ms;
    f.preemph = c->preemphasis;
    f.delta_order = c->delta_order;
    f.delta_win = c->delta_win_length;
    f.use_cmvn = c->use_cmvn;
    f.cmvn_eps = c->cmvn_eps;
    return f;
}

int s3enc_fbank_num_frames(const s3enc_fbank_config* cfg, int64_t n_samples, int32_t* frames) {
    if (!cfg || !frames) return fail("s3enc_fbank_num_frames: null argument");
    *frames = (int32_t)fbank_num_frames(n_samples, fbank_params(cfg));
    return 0;
}

int s3enc_fbank_forward(const s3enc_fbank_config* cfg, const float* const* wavs, const int64_t* lengths, int32_t B, float* out,
                        int64_t T_max, int32_t device, void* stream) {
    return s3enc_fbank_forward_ex(cfg, 0, wavs, lengths, B, out, T_max, device, stream);
}

int s3enc_fbank_forward_ex(const s3enc_fbank_config* cfg, int32_t window, const float* const* wavs, const int64_t* lengths,
                           int32_t B, float* out, int64_t T_max, int32_t device, void* stream) {
    if (!cfg || !wavs || !lengths || !out) return fail("s3enc_fbank_forward: null argument");
    if (B <= 0) return fail("s3enc_fbank_forward: empty batch");
    if (window < 0 || window > 1) return fail("s3enc_fbank_forward_ex: window must be 0 (povey) or 1 (hamming)");
    FbankParams f = fbank_params(cfg);
    f.window = window;
    if (f.delta_order < 0 || f.delta_order > 2 || f.delta_win < 3 || !(f.delta_win & 1)) return fail("s3enc_fbank_forward: unsupported delta configuration");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail("s3enc_fbank_forward: no HIP device (there is no CPU fallback)");
    HIP_TRY(hipSetDevice(device));
    const int F = f.num_mel_bins * (f.delta_order + 1);
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(hipMemsetAsync(out, 0, (size_t)B * T_max * F * sizeof(float), st));
    for (int b = 0; b < B; ++b) {
        const long T = fbank_num_frames(lengths[b], f);
        if (T <= 0) return fail("s3enc_fbank_forward: an utterance is shorter than one analysis window");
        if (T > T_max) return fail("s3enc_fbank_forward: T_max is smaller than an utterance's frame count");
        HIP_TRY(launch_fbank(f, wavs[b], lengths[b], out + (size_t)b * T_max * F, F, st));
    }
    return 0;
}

int s3enc_op_fbank_batch(const s3enc_fbank_config* cfg, int32_t window, const float* pcm, int64_t row_stride, const int64_t* lengths,
                         int32_t B, int64_t n_max, float* out, int64_t spec_cap_bytes, int32_t device, void* stream) {
    if (!cfg || !pcm || !lengths || !out) return fail("s3enc_op_fbank_batch: null argument");
    if (B <= 0) return fail("s3enc_op_fbank_batch: empty batch");
    if (window < 0 || window > 1) return fail("s3enc_op_fbank_batch: window must be 0 (povey) or 1 (hamming)");
    FbankParams f = fbank_params(cfg);
    f.window = window;
    if (f.delta_order != 0) return fail("s3enc_op_fbank_batch: the batch-wide pass has no deltas (delta_order must be 0)");
    if (!f.use_cmvn) return fail("s3enc_op_fbank_batch: the batch-wide pass ends in the CMVN, which writes the rows behind an utterance (use_cmvn must be 1)");
    if (spec_cap_bytes < 0) return fail("s3enc_op_fbank_batch: spec_cap_bytes must not be negative");
    if (((uintptr_t)pcm & 15) || (row_stride & 3)) return fail("s3enc_op_fbank_batch: pcm must be 16-byte aligned and row_stride a multiple of 4");
    long mx = 0;
    std::vector<int> frames(B);
    for (int b = 0; b < B; ++b) {
        const long T = fbank_num_frames(lengths[b], f);
        if (T <= 0) return fail("s3enc_op_fbank_batch: an utterance is shorter than one analysis window");
        frames[b] = (int)T;
        mx = std::max(mx, (long)lengths[b]);
    }
    if (n_max > 0) {
        if (n_max < mx) return fail("s3enc_op_fbank_batch: n_max is smaller than the longest utterance");
        mx = n_max;
    }
    if (mx > row_stride) return fail("s3enc_op_fbank_batch: n_max exceeds row_stride");
    const long Fmax = fbank_num_frames(mx, f);
    if (Fmax > 0x7fffffffL / 1024) return fail("s3enc_op_fbank_batch: batch too long");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail("s3enc_op_fbank_batch: no HIP device (there is no CPU fallback)");
    HIP_TRY(hipSetDevice(device));
    hipStream_t st = (hipStream_t)stream;
    const size_t ws = fbank_batch_workspace(f, B, Fmax, (size_t)spec_cap_bytes);
    // the workspace and the counts stay with the device between calls (a call that timed its own hipMalloc of 66 MB would measure
    // the allocator); one call at a time uses them: the lock is held until the stream has drained
    static std::mutex mu;
    static std::map<int, std::pair<DevBuf, DevBuf>> scratch;
    std::lock_guard<std::mutex> lock(mu);
    DevBuf& spec = scratch[device].first;
    DevBuf& cnt = scratch[device].second;
    HIP_TRY(spec.ensure(ws));
    HIP_TRY(cnt.ensure((size_t)B * sizeof(int)));
    HIP_TRY(hipMemcpyAsync(cnt.p, frames.data(), (size_t)B * sizeof(int), hipMemcpyHostToDevice, st));
    HIP_TRY(launch_fbank_batch(f, pcm, row_stride, (const int*)cnt.p, B, Fmax, out, f.num_mel_bins, (float*)spec.p, ws, (size_t)spec_cap_bytes, st));
    HIP_TRY(hipStreamSynchronize(st));  // `frames` leaves with this scope
    return 0;
}

int s3enc_logmel_frame_counts(const int64_t* lengths, int32_t B, int64_t n_max, int32_t* counts) {
    if (!lengths || !counts) return fail("s3enc_logmel_frame_counts: null argument");
    if (B <= 0) return fail("s3enc_logmel_frame_counts: empty batch");
    long mx = 0;
    for (int b = 0; b < B; ++b) {
        if (lengths[b] <= 0) return fail("s3enc_logmel_frame_counts: empty utterance");
        mx = std::max(mx, (long)lengths[b]);
    }
    if (n_max > 0) {
        if (n_max < mx) return fail("s3enc_logmel_frame_counts: n_max is smaller than the longest utterance");
        mx = n_max;
    }
    for (int b = 0; b < B; ++b) counts[b] = logmel_frame_count(lengths[b], mx);
    return 0;
}

int s3enc_logmel_forward(const float* const* wavs, const int64_t* lengths, int32_t B, int64_t n_max, int32_t n_mels,
                         float target_level, int32_t cmvn, const int32_t* counts, float* out, int32_t device, void* stream) {
    if (!wavs || !lengths || !out) return fail("s3enc_logmel_forward: null argument");
    if (B <= 0 || B > 65535) return fail("s3enc_logmel_forward: bad batch size");
    if (n_mels < 1 || n_mels > 256) return fail("s3enc_logmel_forward: n_mels must be in 1..256");
    if (cmvn && !counts) return fail("s3enc_logmel_forward: cmvn needs the frame counts (s3enc_logmel_frame_counts)");
    long mx = 0;
    for (int b = 0; b < B; ++b) {
        if (!wavs[b]) return fail("s3enc_logmel_forward: null waveform pointer");
        if (lengths[b] <= 200) return fail("s3enc_logmel_forward: an utterance of at most 200 samples has no reflect-padded centred frame");
        mx = std::max(mx, (long)lengths[b]);
    }
    if (n_max > 0) {
        if (n_max < mx) return fail("s3enc_logmel_forward: n_max is smaller than the longest utterance");
        mx = n_max;
    }
    const long T = logmel_num_frames(mx);
    if ((long)B * T > 0x7fffffffL / 402) return fail("s3enc_logmel_forward: batch too large");
    for (int b = 0; cmvn && b < B; ++b)
        if (counts[b] < 2 || counts[b] > T) return fail("s3enc_logmel_forward: every frame count must be in 2..T (the CMVN's standard deviation)");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail("s3enc_logmel_forward: no HIP device (there is no CPU fallback)");
    DeviceGuard dg(device);
    if (!dg.ok) return fail("s3enc_logmel_forward: hipSetDevice failed");
    hipStream_t st = (hipStream_t)stream;
    DevBuf tbl, scale, sig, spec;
    const size_t o_len = (size_t)B * 8, o_cnt = 2 * (size_t)B * 8;
    std::vector<char> host(o_cnt + (size_t)B * 4, 0);
    for (int b = 0; b < B; ++b) {
        ((const float**)host.data())[b] = wavs[b];
        ((long*)(host.data() + o_len))[b] = (long)lengths[b];
        ((int*)(host.data() + o_cnt))[b] = cmvn ? counts[b] : (int)T;
    }
    HIP_TRY(tbl.ensure(host.size()));
    HIP_TRY(hipMemcpy(tbl.p, host.data(), host.size(), hipMemcpyHostToDevice));
    HIP_TRY(scale.ensure((size_t)B * 4));
    HIP_TRY(sig.ensure(logmel_sig_elems(B, mx) * 4));
    HIP_TRY(spec.ensure(logmel_spec_elems(B, mx) * 4));
    LogmelParams p{};
    p.wavs = (const float* const*)tbl.p;
    p.lens = (const long*)((char*)tbl.p + o_len);
    p.counts = (const int*)((char*)tbl.p + o_cnt);
    p.B = B;
    p.max_len = mx;
    p.n_mels = n_mels;
    p.target_level = target_level;
    p.cmvn = cmvn;
    p.scale = (float*)scale.p;
    p.sig = (float*)sig.p;
    p.spec = (float*)spec.p;
    p.out = out;
    p.o_bs = T * n_mels;
    HIP_TRY(launch_logmel(p, st));
    HIP_TRY(hipStreamSynchronize(st));  // the scratch is freed on return
    return 0;
}

int s3enc_op_layernorm_eps(const float* x, const float* gamma, const float* beta, float eps, int64_t rows, int32_t C, float* out,
                           void* stream) {
    if (!x || !gamma || !beta || !out) return fail("s3enc_op_layernorm_eps: null argument");
    if (rows <= 0 || C < 4 || (C & 3) || C > 2048) return fail("s3enc_op_layernorm_eps: bad shape (C a multiple of 4, at most 2048)");
    if (!(eps >= 0.f)) return fail("s3enc_op_layernorm_eps: eps must not be negative");
    LnEpsParams p;
    p.x = x;
    p.gamma = gamma;
    p.beta = beta;
    p.eps = eps;
    p.rows = rows;
    p.C = C;
    p.out = out;
    HIP_TRY(launch_layernorm_eps(p, (hipStream_t)stream));
    return 0;
}

int s3enc_op_input_repr(const float* feat, const float* w, const float* bias, const float* pos_host, int32_t Tc, const float* gamma,
                        const float* beta, float eps, int64_t rows, int32_t F, int32_t D, float* out, void* stream) {
    if (!feat || !w || !bias || !pos_host || !gamma || !beta || !out) return fail("s3enc_op_input_repr: null argument");
    if (rows <= 0 || rows > 0x7fffffffL / 4 || Tc < 1) return fail("s3enc_op_input_repr: bad shape");
    if (F < 4 || (F & 3) || D < 4 || (D & 3) || D > 2048) return fail("s3enc_op_input_repr: F and D must be multiples of 4 (D at most 2048)");
    hipStream_t st = (hipStream_t)stream;
    DevBuf pos, tmp;
    HIP_TRY(pos.ensure((size_t)Tc * D * 4));
    HIP_TRY(hipMemcpy(pos.p, pos_host, (size_t)Tc * D * 4, hipMemcpyHostToDevice));
    HIP_TRY(tmp.ensure((size_t)rows * D * 4));
    GemmParams g{};
    g.A = feat;
    g.lda = F;
    g.W = w;
    g.bias = bias;
    g.M = (int)rows;
    g.N = D;
    g.K = F;
    g.batches = 1;
    g.out32 = (float*)tmp.p;
    g.ldo = D;
    HIP_TRY(launch_gemm(F32, g, st));
    LnEpsParams p;
    p.x = (const float*)tmp.p;
    p.pos = (const float*)pos.p;
    p.Tc = Tc;
    p.gamma = gamma;
    p.beta = beta;
    p.eps = eps;
    p.rows = rows;
    p.C = D;
    p.out = out;
    HIP_TRY(launch_layernorm_eps(p, st));
    HIP_TRY(hipStreamSynchronize(st));  // the position rows and the projection are freed on return
    return 0;
}

}  // extern "C"
