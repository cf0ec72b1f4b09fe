// engine_internal.h — what the translation units of the engine share: error reporting, device buffers, the weight containers,
// the checkpoint reader (Ckpt, GET / UP), the handle (struct s3enc_encoder), per-kernel profiling, the plumbing every family's
// forward starts with (batch checks, the pinned staging ring, Sink: where the states go), the Linear / layer weights / layer schedule
// of the Transformer encoders, the workspace allocator and the multires-HuBERT plan.
//   engine.hip    s3enc_create (weight packing), the single-resolution forward schedule, the handle's C ABI, and the shared
//                 plumbing's definitions (Ckpt::get, tap_major, load_rnn_layer, batch_n_max, check_out, stage_begin / stage_commit)
//   transformer.hip  what the Transformer encoders share: the un-batched Linear every dense product goes through (linear_f32 / linear),
//                 one layer's weights from a checkpoint (load_layer) and one layer's schedule in either LayerNorm order (encoder_layer)
//   multires.hip  the multires-HuBERT U-net behind post_extract_proj
//   wav2vec.hip / cpc.hip  the convolutional families (wav2vec, modified CPC); rnn.hip: the LSTM / GRU recurrence
//   apc.hip / mockingjay.hip  the log-mel families (APC / VQ-APC on GRU layers; Mockingjay / TERA / AudioALBERT on BERT layers)
//   decoar.hip  DeCoAR: the log-mel front end, a projection and two LSTM stacks on rnnb.hip's batch-shared step
//   npc.hip     NPC: the log-mel front end, ConvBlocks and masked convolutions on convtaps.hip's two-run implicit GEMM
//   vggish.hip  VGGish: the un-padded log-mel examples, the 3 x 3 conv + pool stack on conv2d.hip, three Linears, the quantiser
//   byol_a.hip  BYOL-A: per-segment FFT log-mel (melspec.hip), conv + BatchNorm + floor-pool on conv2d.hip, two Linears, max + mean
//   mae_ast.hip MAE-AST: per-utterance kaldi fbank, the fused patch embedding (patchembed.hip), pre- / post-LN layers of transformer.hip
//   byol_s.hip  BYOL-S: centred windows -> hann(400) FFT log-mel -> whole-batch statistics -> ResNet on stem.hip + conv2d.hip (or BYOL-A's
//               network) -> max + mean, the windows in chunks
//   ssast.hip   SSAST: fixed windows -> window-wise hanning kaldi fbank -> the strided patch embedding (patchstrided.hip) -> timm pre-LN
//               blocks of transformer.hip at eps 1e-6 -> a compacting emit per layer, the windows in chunks
//   (a family file holds its configuration check, its weights, its forward schedule and its shape rules, and hands them to the engine
//   as one FamilyOps record: nothing of the plumbing above)
//   ops.hip       single-kernel entry points (s3enc_op_*), the weighted sum, fbank, tuning keys
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/s3enc.h"
#include "kernels.h"

namespace s3e {
using namespace s3;


extern thread_local std::string g_err;  // s3enc_last_error()

inline int fail(const std::string& msg) {
    g_err = msg;
    return 1;
}

#define HIP_TRY(expr)                                                                                  \
    do {                                                                                               \
        hipError_t _e = (expr);                                                                        \
        if (_e != hipSuccess) {                                                                        \
            char _b[512];                                                                              \
            snprintf(_b, sizeof(_b), "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
            return fail(_b);                                                                           \
        }                                                                                              \
    } while (0)

// ---- checkpoint lookup: the tensors of s3enc_create* by name ------------------------------------------------------------------
struct Ckpt {
    std::map<std::string, const s3enc_tensor*> m;
    Ckpt(const s3enc_tensor* tensors, int n_tensors) {
        for (int i = 0; i < n_tensors; ++i)
            if (tensors[i].name && tensors[i].data) m[tensors[i].name] = &tensors[i];
    }
    int get(const std::string& name, long expect, std::vector<float>& out) const;  // non-zero after fail(): missing / wrong size
};
// inside a creator (or a lambda of one) that returns int and has the reader as `ck`: fetch a tensor / run an upload, or return 1
#define GET(name, n, vec) \
    if (ck.get(name, n, vec)) return 1
#define UP(call)                                                                                          \
    do {                                                                                                  \
        hipError_t _e = (call);                                                                           \
        if (_e != hipSuccess) return fail(std::string("weight upload failed: ") + hipGetErrorString(_e)); \
    } while (0)
// (Cout, Cin, k) as nn.Conv1d holds it -> tap-major [co][j * Cin + ci]: the K order of the channel-last implicit GEMM
void tap_major(const std::vector<float>& t, int cout, int cin, int k, std::vector<float>& o);
// convf22.hip's weights from nn.Conv1d's (C, C, 3): w = tap_major's (C, 3C) image, wp = (C, C) fl(W0 + W2).  s3enc_create and
// s3enc_op_conv_k3s2 both pack through here
void pack_conv_f22(const std::vector<float>& t, int C, std::vector<float>& w, std::vector<float>& wp);

// ---- host-side dtype conversion -------------------------------------------------------------------------
inline uint16_t h_bf16(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}
inline uint16_t h_f16(float f) {
    _Float16 h = (_Float16)f;
    uint16_t r;
    memcpy(&r, &h, 2);
    return r;
}
inline float h_from16(uint16_t v, int dtype) {
    if (dtype == BF16) {
        uint32_t u = ((uint32_t)v) << 16;
        float f;
        memcpy(&f, &u, 4);
        return f;
    }
    _Float16 h;
    memcpy(&h, &v, 2);
    return (float)h;
}

struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    ~DevBuf() {
        if (p) (void)hipFree(p);
    }
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p(o.p), bytes(o.bytes) {
        o.p = nullptr;
        o.bytes = 0;
    }
    hipError_t ensure(size_t n) {
        if (n <= bytes) return hipSuccess;
        if (p) {
            hipError_t e = hipFree(p);  // implicit device sync: nothing in flight still uses it
            p = nullptr;
            bytes = 0;
            if (e != hipSuccess) return e;
        }
        hipError_t e = hipMalloc(&p, n);
        if (e == hipSuccess) bytes = n;
        return e;
    }
    // Growth on the forward path, ordered on `st` instead of synchronising the device: the old block is released with
    // hipFreeAsync (it may still be read by launches already enqueued on `st`) and the new one comes from the
    // stream-ordered allocator, 25 % larger than asked so a serving loop with drifting batch shapes settles after a few
    // growths.  Falls back to the synchronising path if the runtime has no stream-ordered pool.
    hipError_t ensure_on_stream(size_t n, hipStream_t st) {
        if (n <= bytes) return hipSuccess;
        const size_t want = n + n / 4;
        void* np = nullptr;
        hipError_t e = hipMallocAsync(&np, want, st);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            return ensure(want);
        }
        if (p) {
            e = hipFreeAsync(p, st);
            if (e != hipSuccess) {
                (void)hipGetLastError();
                (void)hipStreamSynchronize(st);
                (void)hipFree(p);
            }
        }
        p = np;
        bytes = want;
        return hipSuccess;
    }
};

// current-device RAII: the entry points never leave the caller's (torch's) current device changed
struct DeviceGuard {
    int prev = -1;
    bool ok = true;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) ok = hipSetDevice(dev) == hipSuccess;
    }
    ~DeviceGuard() {
        int cur = -1;
        if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
    }
};

inline hipError_t upload_f32(DevBuf& d, const std::vector<float>& v) {
    hipError_t e = d.ensure(v.size() * 4 + 16);
    if (e != hipSuccess) return e;
    return hipMemcpy(d.p, v.data(), v.size() * 4, hipMemcpyHostToDevice);
}
// Host-side packers run over independent ranges on up to 16 threads (a large model's 315 M weights: 4.6 s of s3enc_create in the
// fp16x2 mode on one thread).  Thread creation can fail (pids cgroup, ulimit -u, bad_alloc) and nothing may throw across the C
// boundary: the ranges whose thread did not start run on the calling thread, the started ones are always joined.
template <typename F>
inline void parallel_ranges(long n, long min_per_thread, F&& fn) {  // fn(begin, end)
    unsigned nt = std::thread::hardware_concurrency();
    nt = nt < 1 ? 1 : (nt > 16 ? 16 : nt);
    if ((long)nt > n / std::max<long>(1, min_per_thread)) nt = (unsigned)std::max<long>(1, n / std::max<long>(1, min_per_thread));
    if (nt <= 1) {
        fn(0L, n);
        return;
    }
    std::vector<std::thread> th;
    unsigned started = 0;
    try {
        th.reserve(nt);
        for (; started < nt; ++started) th.emplace_back([&fn, n, nt, started]() { fn(n * started / nt, n * (started + 1) / nt); });
    } catch (...) {
    }
    for (unsigned t = started; t < nt; ++t) fn(n * t / nt, n * (t + 1) / nt);
    for (auto& x : th) x.join();
}

inline hipError_t upload_cvt(DevBuf& d, const std::vector<float>& v, int dtype) {
    if (dtype == F32) return upload_f32(d, v);
    std::vector<uint16_t> h(v.size());
    const float* src = v.data();
    uint16_t* dst = h.data();
    if (dtype == BF16)
        parallel_ranges((long)v.size(), 1 << 20, [=](long a, long b) { for (long i = a; i < b; ++i) dst[i] = h_bf16(src[i]); });
    else
        parallel_ranges((long)v.size(), 1 << 20, [=](long a, long b) { for (long i = a; i < b; ++i) dst[i] = h_f16(src[i]); });
    hipError_t e = d.ensure(h.size() * 2 + 16);
    if (e != hipSuccess) return e;
    return hipMemcpy(d.p, h.data(), h.size() * 2, hipMemcpyHostToDevice);
}

// Positional-conv weight (folded, [D][Dg][K] like nn.Conv1d.weight) -> the layout of the kernel of `dtype`:
//   fp32   [G][K][Dg/16][Dg(co)][16]         (posconv_kernel: tap-major 16-deep input-channel chunks; inside a row of 16 the
//                                             four 16-byte slots are stored at slot ^ pc_w_swizzle(co): the kernel's
//                                             ds_read_b128 of a (16 co) x (16 ci) fragment block is then bank-conflict free)
//          Dg = 24, 40: per tap the Dg/16 full chunks as above, then the last 8 input channels as [Dg(co)][8] with the
//                                             four 8-byte slots of a row swizzled the same way — Dg * Dg floats per tap, no padding
//   16-bit [G][Dg(co)][k = tap*Dg + ci]       (posconv16_kernel: the W operand of the implicit GEMM)
inline void pack_posconv(const std::vector<float>& w, int D, int G, int K, int dtype, std::vector<float>& out) {
    const int Dg = D / G, full = Dg & ~15;  // input channels in 16-deep chunks; Dg = 24, 40: the last 8 follow as [Dg(co)][8]
    out.assign((size_t)G * K * Dg * Dg, 0.f);
    for (int gi = 0; gi < G; ++gi)
        for (int n = 0; n < Dg; ++n)
            for (int ci = 0; ci < Dg; ++ci)
                for (int k = 0; k < K; ++k) {
                    const float x = w[((long)(gi * Dg + n) * Dg + ci) * K + k];
                    if (dtype == F32 && ci < full)
                        out[((long)gi * K + k) * Dg * Dg + ((long)(ci / 16) * Dg + n) * 16 + ((((ci % 16) >> 2) ^ pc_w_swizzle(n)) << 2) + (ci & 3)] = x;
                    else if (dtype == F32)
                        out[((long)gi * K + k) * Dg * Dg + (long)full * Dg + n * 8 + ((((ci - full) >> 1) ^ pc_w_swizzle(n)) << 1) + (ci & 1)] = x;
                    else
                        out[(((long)gi * Dg + n) * K + k) * Dg + ci] = x;
                }
}

// S3ENC_F16X2: a GEMM weight (N, K) as fp16 rows [hi(K) | lo(K)], w = hi + lo + O(2^-22 |w|)
inline hipError_t upload_f16_hi_lo(DevBuf& d, const std::vector<float>& v, long N, long K) {
    std::vector<uint16_t> h((size_t)N * 2 * K);
    const float* src = v.data();
    uint16_t* dst = h.data();
    parallel_ranges(N, std::max<long>(1, (1 << 19) / std::max<long>(1, K)), [=](long n0, long n1) {
        for (long n = n0; n < n1; ++n)
            for (long k = 0; k < K; ++k) {
                const float w = src[(size_t)n * K + k];
                const uint16_t hi = h_f16(w);
                dst[(size_t)n * 2 * K + k] = hi;
                dst[(size_t)n * 2 * K + K + k] = h_f16(w - h_from16(hi, F16));
            }
    });
    hipError_t e = d.ensure(h.size() * 2 + 16);
    if (e != hipSuccess) return e;
    return hipMemcpy(d.p, h.data(), h.size() * 2, hipMemcpyHostToDevice);
}
// a GEMM operand weight (N, K) in the handle's operand format
inline hipError_t upload_gemm_w(DevBuf& d, const std::vector<float>& v, long N, long K, int dtype, bool x2) {
    return x2 ? upload_f16_hi_lo(d, v, N, K) : upload_cvt(d, v, dtype);
}

// S3ENC_F16X2, round 5: the MX-fp4 image of a weight's lo term (lo = w - fp16(w)) for gemm16.hip's MXW K step.  Per row and
// 32-k block: an E8M0 scale 2^e, e = ceil(log2(max|lo| / 6)) (e2m1's largest magnitude is 6), and 32 e2m1 values lo / 2^e rounded
// to nearest (ties to the even code), element i of the block in nibble i of its 16 bytes.  data: (N, K/32, 16) bytes, scales:
// (N, K/32) bytes (bias 127).
inline unsigned mx_e2m1(float x) {  // |x| <= 6 expected (larger saturates); returns the 4-bit code (sign in bit 3)
    const unsigned sign = x < 0.f ? 8u : 0u;
    const float a = x < 0.f ? -x : x;
    // codes 0..7 = 0, 0.5, 1, 1.5, 2, 3, 4, 6; midpoints 0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5 go to the even code
    unsigned c;
    if (a < 0.25f) c = 0; else if (a == 0.25f) c = 0;
    else if (a < 0.75f) c = 1; else if (a == 0.75f) c = 2;
    else if (a < 1.25f) c = 2; else if (a == 1.25f) c = 2;
    else if (a < 1.75f) c = 3; else if (a == 1.75f) c = 4;
    else if (a < 2.5f) c = 4; else if (a == 2.5f) c = 4;
    else if (a < 3.5f) c = 5; else if (a == 3.5f) c = 6;
    else if (a < 5.f) c = 6; else if (a == 5.f) c = 6;
    else c = 7;
    return sign | c;
}
inline void pack_mx4_lo_rows(const float* w, long K, long n0, long n1, uint8_t* data, uint8_t* scales) {
    const long kb = K / 32;
    for (long n = n0; n < n1; ++n)
        for (long b = 0; b < kb; ++b) {
            float lo[32], amax = 0.f;
            for (int i = 0; i < 32; ++i) {
                const float x = w[(size_t)n * K + b * 32 + i];
                lo[i] = x - h_from16(h_f16(x), F16);
                const float a = lo[i] < 0.f ? -lo[i] : lo[i];
                amax = a > amax ? a : amax;
            }
            int ex = -127;
            if (!(amax <= 3.0e38f)) {
                // a weight outside the fp16 range (hi = inf, lo = -inf) or NaN: the product is non-finite whatever this image says
                // (the forward's status word reports it); E8M0 0xFF is the format's NaN
                ex = 128;
            } else if (amax > 0.f) {
                ex = (int)ceilf(log2f(amax / 6.f));
                while (ex < 127 && ldexpf(6.f, ex) < amax) ++ex;  // (log2f rounding: the scaled maximum must not exceed 6)
                ex = ex < -127 ? -127 : (ex > 127 ? 127 : ex);
            }
            const float inv = ex > 127 ? 0.f : ldexpf(1.f, -ex);
            uint8_t* d = data + ((size_t)n * kb + b) * 16;
            for (int i = 0; i < 32; ++i) d[i >> 1] |= (uint8_t)(mx_e2m1(lo[i] * inv) << ((i & 1) * 4));
            scales[(size_t)n * kb + b] = (uint8_t)(ex + 127);
        }
}
// (rows are independent: a large model's 277 M weights take 6.6 s on one host thread, under a second on eight)
inline void pack_mx4_lo(const std::vector<float>& w, long N, long K, std::vector<uint8_t>& data, std::vector<uint8_t>& scales) {
    const long kb = K / 32;
    data.assign((size_t)N * kb * 16, 0);
    scales.assign((size_t)N * kb, 0);
    const float* src = w.data();
    uint8_t *dd = data.data(), *ds = scales.data();
    parallel_ranges(N, 64, [=](long n0, long n1) { pack_mx4_lo_rows(src, K, n0, n1, dd, ds); });
}
struct MxImage {
    DevBuf data, scales;
    long N = 0, K = 0;
    int kind = 0;  // which GEMM of the path the weight belongs to: a bit of the tuning key gemm16_mx (1 conv, 2 q|k|v, 4 fc1, 8 fc2)
};
inline hipError_t upload_mx4_lo(MxImage& m, const std::vector<float>& v, long N, long K) {
    std::vector<uint8_t> d, s;
    pack_mx4_lo(v, N, K, d, s);
    hipError_t e = m.data.ensure(d.size() + 256);
    if (e != hipSuccess) return e;
    e = m.scales.ensure(s.size() + 256);
    if (e != hipSuccess) return e;
    m.N = N;
    m.K = K;
    e = hipMemcpy(m.data.p, d.data(), d.size(), hipMemcpyHostToDevice);
    return e != hipSuccess ? e : hipMemcpy(m.scales.p, s.data(), s.size(), hipMemcpyHostToDevice);
}

// S3ENC_F32X3: upload the pair-packed bf16 hi / lo image of an (N, K) fp32 weight (K % 32 == 0, else left empty: that
// GEMM then runs on the exact kernel)
inline hipError_t upload_x3(DevBuf& d, const std::vector<float>& v, long N, long K) {
    if (K % 32 || (long)v.size() < N * K) return hipSuccess;
    std::vector<uint16_t> pk;
    pack_x3(v.data(), N, K, pk);
    hipError_t e = d.ensure(pk.size() * 2 + 16);
    if (e != hipSuccess) return e;
    return hipMemcpy(d.p, pk.data(), pk.size() * 2, hipMemcpyHostToDevice);
}

// S3ENC_F32X3 positional conv: the 16-bit layout [G][Dg][K*Dg] as a bf16 hi image followed by the lo image
inline hipError_t upload_posconv_x3(DevBuf& d, const std::vector<float>& w, int D, int G, int K) {
    std::vector<float> lay;
    pack_posconv(w, D, G, K, BF16, lay);
    std::vector<uint16_t> img(lay.size() * 2);
    for (size_t i = 0; i < lay.size(); ++i) {
        const uint16_t h = h_bf16(lay[i]);
        img[i] = h;
        img[lay.size() + i] = h_bf16(lay[i] - h_from16(h, BF16));
    }
    hipError_t e = d.ensure(img.size() * 2 + 16);
    if (e != hipSuccess) return e;
    return hipMemcpy(d.p, img.data(), img.size() * 2, hipMemcpyHostToDevice);
}

// One Transformer layer as transformer.hip's load_layer packs it: q|k|v stacked as one (3 D, D) operand with q pre-scaled, the other
// projections, the LayerNorm affines (ln1: behind the attention, ln2: behind the FFN) and, for WavLM, the gate's tensors
struct LayerW {
    DevBuf wqkv, bqkv, wo, bo, ln1g, ln1b, w1, b1, w2, b2, ln2g, ln2b;
    DevBuf wqkv3, wo3, w13, w23;  // S3ENC_F32X3: pair-packed bf16 hi / lo images of the four weight matrices
    DevBuf grep_w, grep_b, grep_a;
};
// wav2vec 2.0 Conformer layer (ConformerEncoderLayer, wav2vec2_model.py:440-578), exact fp32.  Packed at s3enc_create:
//   FFN1 / FFN2: the 0.5 of `x * 0.5 + residual` folded into w_2 and its bias (a power of two: exact);
//   q | k | v: one (3D, D) matrix with head_dim^-0.5 folded into the q rows and bias, rel_pos: (b_q + pos_bias_u) * head_dim^-0.5;
//   rel_pos: linear_pos (D, D) and qadd = (pos_bias_v - pos_bias_u) * head_dim^-0.5 (the attention kernel's position term);
//   conv module: pointwise_conv1 (2D, D), the depthwise taps (D, K) times BatchNorm's gamma / sqrt(var + eps) and the shift
//   beta - mean * gamma / sqrt(var + eps), pointwise_conv2 (D, D).
struct ConformerLayerW {
    DevBuf f1_lng, f1_lnb, f1_w1, f1_b1, f1_w2, f1_b2;
    DevBuf at_lng, at_lnb, wqkv, bqkv, wo, bo, wpos, qadd;
    DevBuf cv_lng, cv_lnb, pw1, taps, shift, pw2;
    DevBuf f2_lng, f2_lnb, f2_w1, f2_b1, f2_w2, f2_b2;
    DevBuf fin_g, fin_b;
};
struct ConvW {
    DevBuf w, bias, lng, lnb;  // w: conv0 fp32 [C][k]; conv>=1 compute dtype [C][k*Cin]
    DevBuf w3;                 // S3ENC_F32X3: pair-packed image of w (conv >= 1)
    DevBuf wp;                 // S3ENC_F32, k = 3: fp32 (C, C) image of tap 0 + tap 2 (convf22.hip)
    bool has_bias = false;
};

// multires-HuBERT (multires_hubert/hubert_model.py:337-530): one TransformerEncoder of the U-net, and a conv adapter
struct BlockW {
    std::vector<LayerW> layers;
    DevBuf eln_g, eln_b;  // the block's own encoder.layer_norm
};
struct AdapterConvW {
    DevBuf w, w3;  // the convolution as a GEMM operand (N, K) in the compute dtype (+ the S3ENC_F32X3 image)
    DevBuf g, b;   // Fp32GroupNorm(1, D) affine
};
struct AdapterW {
    AdapterConvW up, down;  // ConvTranspose1d(stride = up_rate) / Conv1d(stride = down_rate); plain variants hold one
    int kind = 0;           // 0 ConvAdapter (both), 1 ConvDownsampler, 2 ConvUpsampler
    int up_rate = 1, down_rate = 1;
};

// wav2vec / vq-wav2vec (wav2vec.hip): conv0 [C][10]; every other convolution tap-major (C, k * C); GroupNorm(1, C) affine per
// block (empty with non_affine_group_norm); the quantizer's projection(s) and its codebook as the gather table (Gt, V, Dv)
struct W2vW {
    std::vector<DevBuf> ext_w, ext_g, ext_b;
    std::vector<DevBuf> agg_w, agg_bias, agg_g, agg_b;
    std::vector<DevBuf> vq_w, vq_b;  // gumbel: weight_proj's Linear layers
    std::vector<DevBuf> km_w;        // k-means: the grouped 1x1 projection, one (Cg, Cg) matrix per group
    DevBuf km_g, km_b, emb_t;        // its GroupNorm(G, C) affine; the embedding as (G, Cg, V) for the distance kernel
    DevBuf table;
};

// LSTM (G = 4 gates) / GRU (G = 3) layers: per layer weight_ih (G H, I) as the input projection's GEMM operand, its bias b_ih + the
// foldable part of b_hh, weight_hh in rnn.hip's k-quad-major layout and, for a GRU, b_hn
struct RnnW {
    std::vector<DevBuf> w_ih, b_pre, w_hh, b_hn;
};
// appends the layer whose tensors are named `prefix` + {weight_ih, weight_hh, bias_ih, bias_hh} + `suffix` (I: its input width)
int load_rnn_layer(const Ckpt& ck, const std::string& prefix, const std::string& suffix, int G, int H, int I, RnnW& w);

// modified CPC (cpc.hip): conv0 [C][10]; conv1.. tap-major (C, k * C); every convolution's bias and ChannelNorm affine; the
// recurrent layers (layer 0 reads the encoder output: I = H)
struct CpcW : RnnW {
    std::vector<DevBuf> conv_w, conv_b, cn_g, cn_b;
};

// APC / VQ-APC (apc.hip): GRU layers (I = the mel bins for layer 0)
using ApcW = RnnW;

// DeCoAR (decoar.hip): post_extract_proj; per layer the input projections of both stacks and their weight_hh in rnnb.hip's layout.
// Layer 0's two projections read the same rows and are stacked as one (8 H, H) operand; the later layers keep one per direction.
struct DecoarW {
    DevBuf proj_w, proj_b;
    std::vector<DevBuf> w_ih[2], b_pre[2], w_hh[2];  // [0] forward_lstm, [1] backward_lstm
    DevBuf w_ih0, b_pre0;                            // layer 0: forward rows, then backward rows
};

// NPC (npc.hip): per block the k = 3 and 1 x 1 convolutions with their BatchNorms folded in, and (where the block has one) the masked
// convolution packed twice: the live taps only, and all k taps with the masked ones stored as zeros (tuning key npc_skip_taps)
struct NpcW {
    std::vector<DevBuf> w3, b3, w1, b1, wm, wm_dense, bm;
    std::vector<int> has_mask;
};

// VGGish (vggish.hip): per conv layer conv2d.hip's packed image and the bias, the three Linears, the post-processor's PCA matrix and
// means (postprocess only), and the front end's constants: the windowed DFT (2 nbin, window) and the mel matrix (nbin, bands)
struct VggishW {
    std::vector<DevBuf> cw, cb;
    DevBuf fw[3], fb[3];
    DevBuf pca, pca_mean;
    DevBuf dft, bands, wts;  // the folded hann x DFT operand; the mel matrix band by band (spectral.h's sparsify)
};

// BYOL-A (byol_a.hip): per conv layer conv2d.hip's packed image (taps transposed: the image is time x mel) and the BatchNorm as the
// epilogue's per-channel scale / shift (the conv bias inside the shift), and the two Linears
struct ByolAW {
    DevBuf cw[3], scale[3], shift[3];
    DevBuf fw[2], fb[2];
};

// BYOL-S (byol_s.hip): the ResNet's stem (stem.hip's tap-major image) and per BasicBlock conv2d.hip's packed images with the
// BatchNorms as per-channel scale / shift; `ntt` is the `default` network, AudioNTT2020 itself
struct ByolSBlockW {
    DevBuf w1, s1, t1, w2, s2, t2, wd, sd, td;  // conv1 / bn1, conv2 / bn2, downsample.0 / .1 (first block of layers 2-4)
    int cin = 0, cout = 0, stride = 1;
    bool down = false;
};
struct ByolSW {
    DevBuf stem_w, stem_s, stem_t;
    std::vector<ByolSBlockW> blocks;
    ByolAW ntt;
};
// byol_a.hip's network behind its front end, shared with byol_s.hip: the workspace of nseg segments
struct ByolANet {
    float* act[3];
    float* fcb[2];
};

// Mockingjay / TERA / AudioALBERT (mockingjay.hip): the input representation, the position table and the BERT layers (ONE layer with
// share_layer)
struct MjW {
    DevBuf in_w, in_b, in_g, in_beta, pos;
    int pos_rows = 0;
    std::vector<LayerW> layers;
};

// MAE-AST (mae_ast.hip): the patch Linear with the eval BatchNorm folded in (W' = s W, b' = b - s mean rowsum(W)), the leading rows
// of the checkpoint's own sinusoidal table, encoder.layer_norm (post-LN only) and the layers
struct MaeAstW {
    DevBuf pw, pb, pos, eln_g, eln_b;
    std::vector<LayerW> layers;
};

// SSAST (ssast.hip): the patch conv as (D, tshape * fshape) in [n][t][f] order with its bias, the two prefix rows (cls_token + pos[0],
// dist_token + pos[1]), the patch tokens' position rows in the time-major order and the timm blocks
struct SsastW {
    DevBuf pw, pb, prefix, pos;
    std::vector<LayerW> layers;
};

struct ProfRec {
    int kind;
    hipEvent_t a, b;
};
struct FamilyOps;

}  // namespace s3e

using namespace s3e;  // (internal header: only the engine's own translation units include it)

struct s3enc_encoder {
    // (the names below are s3e:: / s3:: types)
    s3enc_config cfg;
    int device = 0;
    int dtype = F32;
    bool x3 = false;  // S3ENC_F32X3
    bool x2 = false;  // S3ENC_F16X2: fp16 data flow, GEMM weights as [hi | lo] fp16 halves (GemmParams.wsplit)
    // S3ENC_F16X2 on a GroupNorm extractor (base models: conv1..6 are GELU-only, nothing renormalises between them): from
    // this conv layer on, the stack runs on fp32 ACTIVATIONS through the three-term GEMM (gemm_x3.hip) instead of rounding
    // every layer's output to fp16 — six stacked roundings are the largest single term of the mode's error on
    // released-checkpoint statistics (tools/fp16_error_budget.py, profiles/r04_fp16_error_budget.md); 0 = off
    int x2_conv_f32_from = 0;
    // S3ENC_F16X2: post_extract_proj reads the fp32 LayerNorm(C) output through the three-term GEMM (0.4 % of the path's FLOPs;
    // the rounding of its operand is the third-largest term of the mode's error budget)
    bool x2_proj_f32 = false;
    // S3ENC_F16X2: the attention output stays fp32 and out_proj reads it through the three-term GEMM (4 % of the path's FLOPs at
    // 1.45x their two-term cost): the rounding of out_proj's operand is the largest non-conv term of the mode's error budget on
    // released-checkpoint statistics (profiles/r04_fp16_error_budget.md)
    bool x2_attn_f32 = false;
    int es = 4;  // element size of the compute dtype
    std::vector<ConvW> conv;
    DevBuf gn_g, gn_b;
    DevBuf fln_g, fln_b, proj_w, proj_b, pos_w, pos_b, eln_g, eln_b;
    DevBuf proj_w3, pos_w3;  // S3ENC_F32X3
    std::vector<LayerW> layers;
    std::vector<ConformerLayerW> cf_layers;  // cfg.layer_type == 1 (then `layers` is empty)
    // Conformer position tables, built on the host with the reference's fp32 formulas for the largest T seen and grown on demand
    // (rows for a smaller T are a window: every entry depends on its position only):
    //   rope:    (rope_T, 64) rows {cos[32], sin[32]} of t * inv_freq (RotaryPositionalEmbedding, wav2vec2_model.py:40-71)
    //   rel_pos: (2 pe_T - 1, D) sin / cos of relative positions pe_T - 1 ... -(pe_T - 1) (RelPositionalEncoding, :1525-1588)
    DevBuf rope_tab, pe_tab;
    int rope_T = 0, pe_T = 0;
    DevBuf rel_table;  // WavLM: [H][2R+1], entry (h, rel + R), R = max_distance (the bucket saturates there)
    int rel_R = 0;
    // data2vec positional-conv stack (cfg.pos_conv_depth > 1): per block the packed conv weight + bias; pos_k = the kernel
    // width as packed (zero taps appended so that the 16-bit implicit GEMM's k axis is a multiple of 128), pos_pad = the
    // real kernel's K / 2; ones / zeros = the affine of LayerNorm(elementwise_affine=False)
    std::vector<DevBuf> pos_ws, pos_bs;
    int pos_k = 0, pos_pad = 0;
    DevBuf ones, zeros;
    DevBuf head_w1, head_b1, head_w2, head_b2, head_w13, head_w23;  // DistilHuBERT prediction heads (+ S3ENC_F32X3 images)
    DevBuf wsum_part;  // persistent partials of s3enc_weighted_sum_backward
    std::vector<BlockW> mr_blocks;      // S3ENC_MULTIRES: encoders..., middle_encoder, decoders... (execution order)
    std::vector<AdapterW> mr_adapters;  // downsample_modules[0..R-2], then upsample_modules[0..R-2]
    DevBuf ws_mr;                       // activation workspace of the U-net behind post_extract_proj
    std::unique_ptr<W2vW> w2v;          // S3ENC_WAV2VEC
    s3enc_wav2vec_config w2v_cfg = {};  // ... and its second configuration block (s3enc_create_ex)
    std::unique_ptr<CpcW> cpc;          // S3ENC_CPC
    s3enc_cpc_config cpc_cfg = {};      // ... and its second configuration block (s3enc_create_cpc)
    std::unique_ptr<ApcW> apc;          // S3ENC_APC
    s3enc_apc_config apc_cfg = {};      // ... and its second configuration block (s3enc_create_apc)
    std::unique_ptr<MjW> mj;            // S3ENC_MOCKINGJAY
    s3enc_mockingjay_config mj_cfg = {};  // ... and its second configuration block (s3enc_create_mockingjay)
    std::unique_ptr<DecoarW> decoar;    // S3ENC_DECOAR
    s3enc_decoar_config decoar_cfg = {};  // ... and its second configuration block (s3enc_create_decoar)
    std::unique_ptr<NpcW> npc;          // S3ENC_NPC
    s3enc_npc_config npc_cfg = {};      // ... and its second configuration block (s3enc_create_npc)
    std::unique_ptr<VggishW> vggish;    // S3ENC_VGGISH
    s3enc_vggish_config vggish_cfg = {};  // ... and its second configuration block (s3enc_create_vggish)
    std::unique_ptr<ByolAW> byol_a;     // S3ENC_BYOL_A
    s3enc_byol_a_config byol_a_cfg = {};  // ... and its second configuration block (s3enc_create_byol_a)
    std::unique_ptr<MaeAstW> mae_ast;   // S3ENC_MAE_AST
    s3enc_mae_ast_config mae_ast_cfg = {};  // ... and its second configuration block (s3enc_create_mae_ast)
    std::unique_ptr<ByolSW> byol_s;     // S3ENC_BYOL_S
    s3enc_byol_s_config byol_s_cfg = {};  // ... and its second configuration block (s3enc_create_byol_s)
    std::unique_ptr<SsastW> ssast;      // S3ENC_SSAST
    s3enc_ssast_config ssast_cfg = {};  // ... and its second configuration block (s3enc_create_ssast)
    const FamilyOps* ops = nullptr;     // the record of a family with a second configuration block (set at create time)
    float* aux_codewords = nullptr;     // s3enc_forward_aux: where the running forward writes the quantizer's outputs
    long long* aux_codeids = nullptr;

    // S3ENC_F16X2: MX-fp4 images of the weights' lo terms, keyed by the device pointer of the [hi | lo] rows they belong to
    std::map<const void*, std::unique_ptr<MxImage>> mx_images;

    Tuning tun;               // s3enc_set_handle_tuning: this handle's own kernel-variant selection ...
    bool has_tuning = false;  // ... in force (for the calling thread) while its forward enqueues kernels

    DevBuf ws;      // activation workspace
    DevBuf small;   // tables, stats
    void* pinned = nullptr;  // host staging ring
    static constexpr int RING = 4;
    size_t slot_bytes = 0;
    hipEvent_t slot_ev[RING] = {};
    int slot_next = 0;

    std::vector<hipEvent_t> layer_events;  // caller-owned, recorded when hidden_states[l] is final

    // s3enc_forward_status (ABI 6): the device word the row kernels OR into (kernels.h, t_status) is cleared at the start of
    // every forward and copied at its end into the next slot of a small pinned ring, with an event behind the copy — so a
    // status read folds the slots whose event has fired and never touches the device; a host running more than STATUS_RING
    // forwards ahead of the GPU waits for the oldest one when it comes round to its slot
    static constexpr int STATUS_RING = 8;
    DevBuf status_dev;
    int* status_host = nullptr;  // STATUS_RING words
    hipEvent_t status_ev[STATUS_RING] = {};
    bool status_busy[STATUS_RING] = {};
    int status_next = 0;
    int status_sticky = 0;  // bits of finished forwards not yet handed to the caller
    // fold the finished slots into status_sticky; wait: block for all of them.  Returns the number still running.
    int status_collect(bool wait) {
        int running = 0;
        for (int k = 0; k < STATUS_RING; ++k) {
            const int i = (status_next + k) % STATUS_RING;  // oldest first
            if (!status_busy[i]) continue;
            const hipError_t q = wait ? hipEventSynchronize(status_ev[i]) : hipEventQuery(status_ev[i]);
            if (q == hipErrorNotReady) {
                (void)hipGetLastError();
                ++running;
                continue;
            }
            status_busy[i] = false;
            if (q == hipSuccess) status_sticky |= ((volatile int*)status_host)[i];
        }
        return running;
    }

    // profiling
    int prof = 0;  // 0 off, 1 every kernel, 2 only the GEMM launches (the dominant kernel: cheap enough for a timed region)
    std::vector<std::string> kinds;
    std::vector<double> kflops, kbytes;
    std::vector<long> klaunches;
    std::vector<ProfRec> recs;
    std::vector<hipEvent_t> ev_pool;  // timing events are recycled across profile_reset, never created per forward twice

    // debug taps of the last forward
    struct Tap {
        const void* p;
        long elems;
        int dtype;
    };
    std::map<std::string, Tap> taps;

    ~s3enc_encoder() {
        for (auto& r : recs) {
            (void)hipEventDestroy(r.a);
            (void)hipEventDestroy(r.b);
        }
        for (auto ev : ev_pool) (void)hipEventDestroy(ev);
        for (int i = 0; i < RING; ++i)
            if (slot_ev[i]) (void)hipEventDestroy(slot_ev[i]);
        if (pinned) (void)hipHostFree(pinned);
        if (status_host) (void)hipHostFree(status_host);
        for (int i = 0; i < STATUS_RING; ++i)
            if (status_ev[i]) (void)hipEventDestroy(status_ev[i]);
    }

    int kind_id(const char* name) {
        for (size_t i = 0; i < kinds.size(); ++i)
            if (kinds[i] == name) return (int)i;
        kinds.push_back(name);
        kflops.push_back(0);
        kbytes.push_back(0);
        klaunches.push_back(0);
        return (int)kinds.size() - 1;
    }
    bool take_event(hipEvent_t* ev) {
        if (!ev_pool.empty()) {
            *ev = ev_pool.back();
            ev_pool.pop_back();
            return true;
        }
        return hipEventCreate(ev) == hipSuccess;
    }
};

namespace s3e {

struct Prof {
    s3enc_encoder* e;
    hipStream_t st;
    int idx = -1;
    Prof(s3enc_encoder* enc, hipStream_t s, const char* kind, double flops, double bytes) : e(enc), st(s) {
        if (!e || !e->prof) return;
        if (e->prof == 2 && strncmp(kind, "gemm", 4) != 0) return;
        const int k = e->kind_id(kind);
        e->kflops[k] += flops;
        e->kbytes[k] += bytes;
        e->klaunches[k] += 1;
        ProfRec r;
        r.kind = k;
        if (!e->take_event(&r.a)) return;
        if (!e->take_event(&r.b)) {
            e->ev_pool.push_back(r.a);
            return;
        }
        (void)hipEventRecord(r.a, st);
        e->recs.push_back(r);
        idx = (int)e->recs.size() - 1;
    }
    ~Prof() {
        if (idx >= 0) (void)hipEventRecord(e->recs[idx].b, st);
    }
};

struct FwdOpts {
    int selection = S3ENC_SEL_HIDDEN;
    int out_dtype = F32;
    bool featurize = false;
    int feat_norm = 0;
    const float* w = nullptr;  // host, one per state
};

// ---- what every family's forward starts with ----------------------------------------------------------------------------------------
// B, the waveform pointers, the lengths and the caller's n_max (0: none); n_max: the batch's padded length in samples
int batch_n_max(const float* const* wav_ptrs_host, const int64_t* lengths, int32_t B, int64_t n_max_in, long& n_max);
// the caller's output: non-null, 16-byte aligned and — for a slab of states — a layer_stride of at least `min_stride` elements
int check_out(const void* out, const FwdOpts& fo, int64_t layer_stride, long min_stride);
// Pinned staging ring (so the async H2D copy never reads freed / overwritten host memory).  stage_begin hands out the next slot's
// host pointer once the copy that last read it has finished (growing the ring when `bytes` outgrow a slot); the caller fills `bytes`
// there and stage_commit enqueues their copy to `dst` on `st` with the slot's event behind it.
int stage_begin(s3enc_encoder* e, size_t bytes, hipStream_t st, char*& hp);
int stage_commit(s3enc_encoder* e, const char* hp, void* dst, size_t bytes, hipStream_t st);

// Where the selected states go: straight into the caller's fp32 slab (the producing kernel writes the slot, nothing is
// copied), as 16-bit copies next to an internal fp32 residual stream, or only as their term of the Featurizer sum.
struct Sink {
    s3enc_encoder* e;
    hipStream_t st;
    int mode;  // 0 fp32 slab, 1 16-bit slab, 2 featurize
    void* out;
    long stride;
    int dt;  // the handle's compute dtype (the 16-bit slab's type)
    long M;
    int D;
    const float* w;
    int norm;
    bool first = true;

    float* slot32(int si) const { return (mode == 0 && si >= 0) ? (float*)out + (long)si * stride : nullptr; }
    void* slot16(int si) const { return (mode == 1 && si >= 0) ? (void*)((u16*)out + (long)si * stride) : nullptr; }
    bool term(int si) const { return mode == 2 && si >= 0 && w[si] != 0.f; }  // state `si` adds a term to the Featurizer sum
    bool wanted(int si) const { return si >= 0 && (mode != 2 || w[si] != 0.f); }
    // featurize with no non-zero weight among the NS states: no kernel writes the (rows, D) sum, it is zeroed here
    hipError_t zero_without_terms(int NS, long rows) const {
        for (int i = 0; mode == 2 && i < NS; ++i)
            if (w[i] != 0.f) return hipSuccess;
        return mode == 2 ? hipMemsetAsync(out, 0, (size_t)rows * D * 4, st) : hipSuccess;
    }
    // Featurizer term of state `si`, fused into a row kernel that holds the state as its input (1) or output (2)
    LnAcc acc(int si, int where) {
        LnAcc a;
        if (!term(si)) return a;
        a.acc = (float*)out;
        a.w = w[si];
        a.mode = where;
        a.norm = norm;
        a.init = first;
        first = false;
        return a;
    }
    // a state a non-LayerNorm kernel left in fp32 outside the slab: its 16-bit copy / its Featurizer term
    hipError_t emit(int si, const float* x, bool copy16 = true) {
        if (si < 0) return hipSuccess;
        if (mode == 1 && copy16) return launch_emit_state(dt, x, M, D, slot16(si), LnAcc(), st);
        if (term(si)) return launch_emit_state(F32, x, M, D, nullptr, acc(si, 1), st);
        return hipSuccess;
    }
    hipError_t done(int si) {
        if (si < 0 || mode == 2 || e->layer_events.empty() || si >= (int)e->layer_events.size()) return hipSuccess;
        return hipEventRecord(e->layer_events[si], st);
    }
};

// S3ENC_F16X2 hybrids: would the three-term GEMM take an (N, K) product whose A rows are `lda` fp32 elements apart?  The REAL
// predicate (gemm_x3_eligible) on a representative call — 256-byte aligned operands as the workspace allocator hands them out, a
// dense fp32 output — instead of a hand-copied subset of it: s3enc_create decides the hybrids with this, so the forward's
// "not a shape of the three-term GEMM" failures cannot be reached through a drift between two predicates (round-4 ADVICE).
inline bool x3_shape_ok(long N, long K, long lda) {
    GemmParams g{};
    g.A = (const void*)(uintptr_t)256;
    g.W_x3 = (const void*)(uintptr_t)256;
    g.out32 = (float*)(uintptr_t)256;
    g.lda = lda;
    g.a_bs = 4 * lda;  // any multiple of lda: the extractor's batch stride is L * C, the encoder's GEMMs are one batch
    g.M = 256;
    g.N = (int)N;
    g.K = (int)K;
    g.batches = 1;
    g.ldo = N;
    g.o_bs = 256 * N;
    return gemm_x3_eligible(g);
}

// S3ENC_F16X2: every GEMM of the handle runs on its [hi | lo] weight rows — with the lo term as an MX-fp4 image where one was
// packed for exactly this weight (round 5: gemm16.hip MXW; launch_gemm falls back to the two-term loop for other shapes)
inline GemmParams wsplit_of(const s3enc_encoder* e, GemmParams g) {
    g.wsplit = e->x2 ? 1 : 0;
    if (e->x2) {
        auto it = e->mx_images.find(g.W);
        if (it != e->mx_images.end() && it->second->N == g.N && it->second->K == g.K && (tuning().gemm16_mx & it->second->kind)) {
            g.W4 = it->second->data.p;
            g.W4s = it->second->scales.p;
            g.mxw = 1;
        }
    }
    return g;
}

// ---- transformer.hip: the Linear, the layer weights and the layer schedule behind every Transformer encoder -------------------------
// out(M, N) = act(A(M, K) . W(N, K)^T + bias) (+ residual), one batch, under the profile record `kind`: 2 M N K flops and
// (M K + N K) es_in + M N es_out (+ 4 M N for the residual) bytes
struct Linear {
    const char* kind;
    const void *A, *W;
    const void* bias;  // fp32 (N), or null
    long M;
    int N, K;
    int act = 0;  // GemmParams::act
    const float* residual = nullptr;
    float* out32 = nullptr;
    void* out16 = nullptr;
    long lda = 0, ldo = 0;             // row pitches of A and of the output; 0: dense (K, N)
    const void* W_x3 = nullptr;        // `linear`: the S3ENC_F32X3 image of W, or null
    const char* x3_or_fail = nullptr;  // S3ENC_F16X2 hybrids: A is fp32 — the three-term GEMM takes the product or the forward fails, naming this
    const float2* res_ln_stats = nullptr;  // GemmParams::res_ln_*
    const float *res_ln_g = nullptr, *res_ln_b = nullptr;
};
hipError_t linear_f32(s3enc_encoder* e, hipStream_t st, const Linear& l);  // exact fp32 operands, whatever the handle's mode
// operands in the handle's mode (e->dtype, W_x3, wsplit_of), 16-bit output unless out32 is set; non-zero after fail()
int linear(s3enc_encoder* e, hipStream_t st, const Linear& l);
GemmParams linear_params(const s3enc_encoder* e, const Linear& l);  // what `linear` launches (for the eligibility predicates)

// a GEMM weight in the handle's operand format; S3ENC_F16X2: + the MX-fp4 image of its lo term for the weights gemm16.hip's MXW K
// step pays for (gemm16_mx_weight_rule: decided per weight, never per batch; wsplit_of finds the image by the weight's pointer).
// Only the kinds the tuning key gemm16_mx names AT CREATE TIME get an image (default 14: conv1's would never be read, and with
// gemm16_mx = 0 none would — seconds of host packing and the device bytes on a large model): the mask can be narrowed after
// s3enc_create, widening it needs a new handle.
hipError_t upload_gemm_w_mx(s3enc_encoder* e, DevBuf& buf, const std::vector<float>& v, long N, long K, int kind);
// the tensor names of a layer under its prefix: fairseq's TransformerSentenceEncoderLayer, BERT's (Mockingjay)
struct LayerNames {
    const char *qkv[3], *out, *ln1, *fc1, *fc2, *ln2;
    const char* qkv_fused = nullptr;  // set: ONE (3 D, D) tensor with rows q | k | v under this name (timm's attn.qkv); qkv[] is not read
};
extern const LayerNames kFairseqLayer, kBertLayer, kTimmLayer;
// the layer named `prefix` (ending in '.') in the handle's operand mode, the q rows and bias times `qscale`; gate: WavLM's grep tensors too
int load_layer(s3enc_encoder* e, const Ckpt& ck, const std::string& prefix, const LayerNames& n, float qscale, bool gate, LayerW& L);

// One layer of B sequences of T rows, enqueued on `st`.  The caller owns the buffers and decides where states go: the layer sees pointers.
struct LayerRun {
    int B;
    long T;
    const int* valid;  // [B] keys >= valid[b] are masked
    bool pre_ln;
    const float* x;   // the layer's input: the fp32 residual stream
    const void* x16;  // post-LN 16-bit modes: its 16-bit copy, the q|k|v operand
    float* x_next;    // the layer's output — pre-LN: fc2's, post-LN: LayerNorm 2's
    void* x16_next;   // ... and its 16-bit copy (pre-LN: a slab slot or null)
    void *xT, *qkv, *attn, *hbuf;  // (M, D) LayerNorm output, (M, 3 D), (M, D), (M, F) in the compute dtype (attn: fp32 with x2_attn_f32)
    float *tmp1, *tmp2;            // (M, D) fp32
    float2* lnst = nullptr;        // (M) row statistics of LayerNorm 1 (allow_ln1_fold)
    const float* bias_table = nullptr;  // WavLM: AttnParams::bias_table / table_R / gate
    int table_R = 0;
    const float* gate = nullptr;
    LnGate gate_here, gate_next;  // the gate of this layer's attention (pre-LN: LayerNorm 1 writes it), of the next layer's (post-LN: LayerNorm 2)
    LnAcc acc_in, acc_out;        // Featurizer terms: of the input (pre-LN, LayerNorm 1 adds it), of the output (post-LN, LayerNorm 2)
    // the ffn_out selection (ffn_out32 set): fc2 exports fc2(x) + bias here, `ffn_exported` runs behind it (non-zero after fail()),
    // then an elementwise add re-applies the residual
    float* ffn_out32 = nullptr;
    void* ffn_out16 = nullptr;
    std::function<int()> ffn_exported;
    bool allow_ln1_fold = false;  // post-LN 16-bit: fc2's epilogue rebuilds LayerNorm 1's output where its shape class can (tuning key ln1_fold)
    bool ln1_inplace = false;     // post-LN: LayerNorm 1 overwrites tmp1 instead of writing tmp2 (tuning key ws_inplace)
    float ln_eps = 0.f;           // 0: the LayerNorms at the engine's LN_EPS (launch_layernorm); > 0: at this eps through launch_layernorm_eps
                                  // (fp32 handles, pre-LN, no fused Featurizer term / gate / row statistics)
    bool taps = false;            // keep the debug taps qkv0 / attn0
    int stop_after = 0;           // S3ENC_DEBUG_STOP 30..34: return LAYER_STOPPED behind q|k|v, attention, out_proj, LayerNorm 1 / 2, fc1
};
enum { LAYER_DONE = 0, LAYER_FAILED = 1, LAYER_STOPPED = 2 };
int encoder_layer(s3enc_encoder* e, hipStream_t st, const LayerW& Lw, const LayerRun& r);

long conv_len(const s3enc_config& c, long n, int upto /*exclusive*/);  // frames after the first `upto` conv layers
int valid_frames(const s3enc_config& c, long length, long n_max);      // un-masked frames under the family's mask rule

// ---- multires-HuBERT frame geometry (mirrors EncoderConfig.multires_plan in s3prl_amd/config.py) ----------------
struct MrBlockPlan {
    int layers;
    long T;       // frames the block runs on
    int factor;   // repeat_interleave factor of its states (multires_hubert/expert.py:41-47)
    int adapter;  // index into mr_adapters of the conv adapter applied before the block, -1 for the first
    long T_in;    // frames entering that adapter
    long T_sum;   // decoders: min(T, residual frames) of align_size_sum (hubert_model.py:777-783)
};
struct MrPlan {
    std::vector<MrBlockPlan> blocks;
    long T_out = 0;  // common length every (repeated) state is cut to (expert.py:93-101)
};
void mr_plan(const s3enc_config& c, long T0, MrPlan& plan);
long output_frames(const s3enc_config& c, long n_samples);  // frames of the states a forward writes

// bump allocator over the workspace
struct Bump {
    char* base;
    size_t off = 0;
    explicit Bump(void* b) : base((char*)b) {}
    void* take(size_t bytes) {
        void* p = base ? base + off : nullptr;
        off += (bytes + 255) & ~(size_t)255;
        return p;
    }
};

int num_states(const s3enc_config& c, int selection);
// multires.hip: the U-net behind post_extract_proj (xproj: (B, T0, D) fp32, padded frames zero)
int multires_tail(s3enc_handle e, hipStream_t st, int B, const MrPlan& plan, const std::vector<const int*>& d_valid, float* xproj,
                  void* out, long layer_stride, const FwdOpts& fo);

// ---- the families that come with a second configuration block ------------------------------------------------------------------------
// All the engine knows about such a family is its record: a family file defines it at its end, beside the thin adapters to its own
// functions, and engine.hip lists the records (kFamilies).  The handle points at its family's record; null: a Transformer family.
struct FamilyOps {
    int family;
    const char *block, *name, *entry, *needs;  // the refusals of an entry that met the wrong family (engine.hip, wrong_entry)
    const char* one_list;  // s3enc_num_states: "feature_selection is not defined for <one_list>"; null: every selection is defined
    int (*check)(const s3enc_config& c, const void* block);
    int (*create)(s3enc_encoder* e, const Ckpt& ck, const void* block);  // copies the block into the handle, then packs the weights
    int (*forward)(s3enc_handle e, const float* const* wav_ptrs_host, const int64_t* lengths, int32_t B, int64_t n_max_in,
                   const FwdOpts& fo, void* out, int64_t layer_stride, hipStream_t st);
    // the shape rules; null: the rule the Transformer families have
    long (*frames)(const s3enc_encoder* h, long n_samples);         // s3enc_num_frames / s3enc_num_output_frames
    int (*valid)(const s3enc_encoder* h, long length, long n_max);  // s3enc_valid_frames; null with `frames`: the utterance's own
                                                                    // count of them, clamped to the batch's
    int (*rate)(const s3enc_encoder* h);                            // s3enc_downsample_rate
    int (*states)(const s3enc_encoder* h);                          // s3enc_num_states
};
// (read-only, but not declared const: the compiler would emit a constant-initialised const object into the device code as well, where
// the host functions it points to do not exist)
extern FamilyOps kWav2vecFamily, kCpcFamily, kApcFamily, kMockingjayFamily, kDecoarFamily, kNpcFamily, kVggishFamily, kByolAFamily,
    kMaeAstFamily, kByolSFamily, kSsastFamily;

// byol_a.hip, for byol_s.hip: AudioNTT2020's weights, its workspace (taken from `wb`; fails when a layer is not addressable with 32-bit
// offsets), the network on nseg bordered (T + 2) x (64 + 2) images up to dst (nseg, D), and out = max_t relu(y) + mean_t relu(y)
int byol_a_load(ByolAW& w, const Ckpt& ck, long feature_d, float bn_eps);
int byol_a_net_plan(long nseg, int T, int D, Bump& wb, ByolANet& nb);
int byol_a_net_run(s3enc_encoder* e, const ByolAW& w, int D, const float* img, long nseg, int T, const ByolANet& nb, float* dst, hipStream_t st);
hipError_t launch_byol_tail(const float* y, int T8, int d, long nseg, float* out, hipStream_t st);

}  // namespace s3e
