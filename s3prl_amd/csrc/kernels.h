// kernels.h — host-side launch interface of the HIP kernels (internal to libs3enc).
#pragma once
#include <cstring>
#include <vector>

#include "common.h"

namespace s3 {
int device_cus();  // gemmt.hip: CUs of the device the process first launched on (256 on an MI355X)

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) once per (kernel instantiation, device) instead of once per launch:
// the call costs several microseconds of host time, and a forward is ~290-560 launches.
template <auto Kern>
inline hipError_t ensure_dynamic_lds(int bytes) {
    static int granted[64] = {};
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    if (dev >= 0 && dev < 64 && granted[dev] >= bytes) return hipSuccess;
    e = hipFuncSetAttribute((const void*)Kern, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e == hipSuccess && dev >= 0 && dev < 64) granted[dev] = bytes;
    return e;
}

// ---- kernel-variant selection (A/B measurement knobs; results never depend on them) -------------------------
// One struct instead of scattered globals: `g_tuning` holds the process defaults (s3enc_set_tuning); a handle may carry its
// own copy (s3enc_set_handle_tuning), which the engine makes current for the calling thread while that handle's forward
// enqueues its kernels (TuningScope) — so two handles, or two threads, never see each other's settings.
struct Tuning {
    int gemm_variant = 3;  // gemm.hip: bit 0 = 64-byte K stages, bit 1 = LDS-DMA staging, bit 2 = no XCD-aware tile order
    int gemm_lds_pad = 0;  // gemm.hip occupancy probe: extra (unused) dynamic LDS per workgroup
    int gemm32_big = 1;    // gemmt.hip, fp32: 0 off, 1 = tile height by shape, 2..5 = force 256 / 192 / 128 / 64 rows
    int gemm_x3_tile = 1;  // gemmt.hip, S3ENC_F32X3: 0 off, 1 = only the shapes with few tiles, 2..5 = force a height
    int gemm32_tail = 1;   // gemmt.hip, fp32: a launch of 128 / 192 / 256-row tiles may end with a tail region of 64-row tiles (the last
                           // workgroups dispatched; same bits): 0 = never, 1 = where the round model says it pays, 2 = every launch, largest tail
    int gemm32_tail_units = 0;  // lab probe under gemm32_tail = 1: 0 = the model's tail, n = a tail of n 64-row units of every batch's M
    int gemm16_big = 3;    // gemm16.hip: 0 off, 3 = choose by shape, 1 / 2 / 4 / 5 / 6 / 7 = force one configuration
    int gemm16_pp = 0;     // gemm16.hip, persistent loop: 0 = every wave issues its LDS-DMA pieces behind fragment steps 0 / 1;
                           // non-zero = waves 4-7 (the SIMD partners of waves 0-3) behind steps 1 / 2 instead (PP 3; measured
                           // within +-1-3 % of 0: profiles/r05_gemm16_loop_probe.md — opt-in)
    int gemm16_mx = 14;    // S3ENC_F16X2, bit mask: which GEMMs take their second weight term as an MX-fp4 image on the scaled-MFMA pipe
                           // where the shape allows (gemm16.hip MXW) — 1 conv1, 2 q|k|v, 4 fc1, 8 fc2; 0 = two fp16 terms everywhere;
                           // 16 = (read at s3enc_create) also the weights whose 256-row tiling is cheaper at the reference batch (measurements).  Default 14: conv1 stays on two fp16 terms —
                           // its A operand (conv0's GroupNorm'd output with loud channels) is the one block-scaled fp4 images suit least
                           // (wav2vec2_base_pl 6.0e-4 with 14, 7.9e-4 with 15: profiles/r05_mx_second_term.md)
    int reserve_cus = 0;   // gemm16.hip, persistent loop: CUs left out of the one-workgroup-per-CU grid.  Measured (profiles/r05_cu_contention.md):
                           // 8-32 foreign workgroups holding CU slots cost the 16-bit step +2 % whatever their number, while a grid of
                           // 240 costs +20 % (the tile rounds are tuned to 256 CUs: q|k|v's 756 tiles become four rounds) — keep 0
    int gemm16_rows = 1;   // gemm16.hip: 1 = GELU epilogues with a 16-bit output take the row-per-lane (no LDS) form, 0 = never
    int attn_lds_pad = 0;  // 16-bit attention occupancy probe
    int attn_persist = 0;  // attention.hip: 1 = persistent workgroups that fetch the next (batch, head, query block) item's Q and first
                           // K / V tile under the current item's last tile (round 6; bit-identical).  MEASURED AND LEFT OFF: the 16-bit
                           // form is 20-30 % slower than the one-shot grid (lab 58 -> 78 us, forward 48.7 -> 53.3 us per launch), the
                           // fp32 form -7 % in the lab and +0.7 % in the forward (profiles/r06_attn_lab.md, r06_attention_persist.md);
                           // against the one-shot kernel of the second session: 43.6 vs 38.5 us HuBERT-base, 54.8 vs 50.4 HuBERT-large,
                           // 110 vs 107 / 130 vs 121 WavLM-large (profiles/r06b_attn_lab_variants.md)
    int conv0_nt = 1;      // frontend.hip, fp32 output: 1 = non-temporal row stores (the 2 GB activation streams past the caches:
                           // 0.578 -> 0.436 ms on HuBERT-base 32 x 10 s, round 4), 0 = plain stores
    int conv_f22 = 1;      // convf22.hip, S3ENC_F32: 1 = conv layers with k = 3, stride 2 in the two-output form (a sixth fewer MFMAs;
                           // different association, same fp32 operands), 0 = the implicit GEMM of gemmt.hip
    int conv0_fast = 1;    // frontend.hip, 16-bit outputs (S3ENC_BF16 / F16 / F16X2) and the split-precision modes' fp32 output: 1 = packed fp32 taps + the packed one-transcendental GELU,
                           // 0 = scalar taps + libm erff (the FAST = false instantiation: ~2x the kernel's time, results a few 16-bit ulps
                           // apart).  Round 6, fourth session: the rows that differ when >= 4 handles' forwards overlap ORIGINATE in
                           // conv0_kernel<16-bit, FAST> — single frames, lanes 48-63, the low halves of the packed outputs — and with 0
                           // (and forward_chain = 0) 32 of 32 overlapping runs kept their bits; neither half of FAST alone, nor wait states,
                           // nor the transcendental unit explains it (profiles/r06d_concurrent_forwards_exclusions.md).  A diagnostic
                           // switch, not a fix: the forward chain stays the default protection
    int ws_inplace = 1;    // engine.hip, post-LN layers: 1 = LayerNorm 1 and fc2 work in place on ONE fp32 buffer (49 MB less
                           // working set per layer: fc2 -3.6 %, LayerNorm -4 % in the bf16 forward, round 4), 0 = two buffers
    int gelu32 = 1;        // S3ENC_F32: 1 = the one-transcendental GELU of every mode (common.h gelu_fast; fp32 rounding level), 0 = libm erff
    int x3_pack_cache = 0; // s3enc_op_gemm(S3ENC_F32X3): keep the packed image of the last weight (micro-benchmarks)
    int fp16x2_conv1_f32 = 0;  // engine.hip, S3ENC_F16X2 (read at s3enc_create): 1 = conv0 writes fp32 and conv1 runs on the three-term GEMM too
    int ln_rows = 1;       // norm.hip: rows per wave of the row LayerNorm.  2 = both rows' loads in flight before the first reduction (launches of
                           // >= 8192 rows; bit-identical by test).  MEASURED AND LEFT OFF (round 6, second session, same lease, HuBERT-base
                           // 32 x 10 s): LN1 + LN2 0.536 -> 0.551 ms per bf16 forward, 0.513 -> 0.529 fp32 — the kernel is at the memory
                           // side's rate (5.3-6.1 TB/s), not short of loads in flight
    int ln_preload = 1;    // norm.hip: 1 = a wave fetches its gamma / beta chunks together with its row instead of behind the two reductions
    int ln1_fold = 1;      // engine.hip, post-LN layers in the 16-bit modes: 1 = LayerNorm 1 writes its 16-bit output and the rows' statistics only, fc2's
                           // epilogue rebuilds the fp32 rows it adds (bit-identical to 0 = LayerNorm 1 writes them)
    int gn_lag_one_block = 1;  // frontend.hip: 1 = GroupNorm lag sums from ONE workgroup per (4096-frame chunk, utterance) over an LDS-staged
                           // window (bit-identical to the k0-workgroups form, 95.7 -> see profiles/r06b_gn_stats.md), 0 = the earlier kernel
    int forward_chain = 1; // engine.hip: 1 = a forward of a 16-bit / split-precision handle waits (hipStreamWaitEvent, no host wait) for the previous
                           // such forward of ANY handle on the same device, whatever stream that one ran on.  With one handle on one stream the
                           // wait is already implied by stream order.  Why: forwards of SEVERAL handles running at once on >= 4 streams are NOT
                           // bit-stable in the modes whose GEMMs stage through global_load_lds (bf16 / fp16 at four streams, fp16x2 / fp32x3 at
                           // eight; never exact fp32, which is left free to overlap): rare rows come out a few 16-bit ulps off
                           // (tools/two_stream_probe.py, profiles/r06c_concurrent_forwards.md; no kernel or pair of kernels reproduces it in
                           // isolation, two streams never do).  Price: sub-batches that under-fill the chip no longer overlap (four
                           // 8-utterance forwards: 8.5 -> 12.1 ms; the same 32 utterances as ONE batch: 6.8 ms).  0 = forwards may overlap
    int rnn_split = -1;    // rnn.hip, the length-aware recurrence: 0 = one launch runs all steps (one workgroup per utterance), 1 / 2 / 4 / 8 =
                           // the step-split form with that many workgroups per utterance, one launch per step (bit-identical);
                           // -1 (default) = the step form with S = 8 where it was measured to win (a GRU at H = 512 with
                           // 8 B <= 256: 27.0 against 88.8 ms per apc_360hr forward, profiles/apc_360hr_fp32.md), else one launch
    int npc_skip_taps = 1; // npc.hip: 1 = the masked convolutions walk their two runs of live taps only (convtaps.hip), 0 = the same kernel over
                           // all k taps on weights whose masked taps are stored as zeros (equal values; the A/B of profiles/npc_360hr_fp32.md)
    int conv2d_n64 = 1;    // conv2d.hip: 1 = launches that allow it (Conv2dParams::n64) run Cout <= 64 on the (256 | 128) x 64 tile, 0 = on the
                           // 128-wide tile, half of whose MFMA columns are then padding (bit-identical; the A/B of profiles/byol_a_fp32.md)
    int melspec_fft = 1;   // melspec.hip: 1 = the 1024-point STFT as a real FFT in LDS, one workgroup per frame; 0 = the overlapping-row GEMM
                           // against the folded hann x DFT matrix (fbank.hip's form at K = 1024: the yardstick and the fallback)
    int patch_embed_fused = 1;  // patchembed.hip: 1 = the patch embedding as ONE implicit GEMM that reads the image in place, 0 = a gather kernel
                           // that writes the (B * tokens, kt * kc) rows, the tile GEMM, then the position add (the yardstick and a second
                           // implementation, held to the fixture bound; the A/B of profiles/mae_ast_fp32.md)
    int patch_strided_fused = 1;  // patchstrided.hip: 1 = SSAST's overlapping patch embedding as ONE implicit GEMM that reads the image in place,
                           // 0 = a gather kernel that writes the (windows * tokens, tshape * fshape) rows, the tile GEMM storing at the
                           // sequence pitch, then the position add (the yardstick and a second implementation, held to the same bound)
    int ssast_chunk = 65536;  // ssast.hip: tokens per pass of the embedding and the layers (whole windows, at least one); bounds the workspace,
                           // never changes a row's bits
    int stem_fused = 0;    // byol_s.hip: 1 = the ResNet stem as one kernel (stem.hip: conv 7 x 7 + affine + ReLU + 3 x 3 / stride-2 pool, 2.25 x the
                           // multiply-adds, no un-pooled map), 0 = the un-pooled map and a pool kernel (bit-identical; measured 223.0
                           // against 222.2 ms per forward: profiles/byol_s_fp32.md)
    int byol_s_chunk = 1024;  // byol_s.hip: windows per pass of the network; bounds the workspace (about 6.2 MB per window), never changes a
                           // window's bits; 128 / 256 / 512 / 1024: 246.9 / 222.2 / 207.5 / 193.2 ms per 32 x 10 s byol_s_resnetish34 forward
                           // (the late layers' few pixels per window fill the chip only across many windows: profiles/byol_s_fp32.md)
    int comm_self_p2p = 0; // comm.hip, S3ENC_EXCHANGE_DIRECT: 1 = a rank's OWN block also travels as an ncclSend-to-self / ncclRecv-from-self
                           // pair inside the state's group instead of a device copy — on a one-GPU box this is the only way the
                           // all-pairs code (symbols, counts, datatype, group bracketing, stream order behind the layer events)
                           // executes at all: RCCL refuses two ranks on one device.  A test hook; same bytes in the same places
};
extern Tuning g_tuning;
extern thread_local const Tuning* t_tuning;  // the current handle's override, or null
inline const Tuning& tuning() { return t_tuning ? *t_tuning : g_tuning; }
struct TuningScope {
    const Tuning* prev;
    explicit TuningScope(const Tuning* t) : prev(t_tuning) { if (t) t_tuning = t; }
    ~TuningScope() { t_tuning = prev; }
};
int tuning_set(Tuning& t, const char* key, int value, const char** err);  // 0 ok; ops.hip

// ---- forward status word (s3enc_forward_status, ABI 6) ---------------------------------------------------------
// A device int32 owned by the handle; the row LayerNorm kernels OR bit 0 into it when a row's mean or variance is not
// finite (every hidden state passes through one of them: a post-LN state IS a LayerNorm output, a pre-LN residual stream
// is the next LayerNorm's input) — the symptom of a 16-bit overflow upstream of the row, or of non-finite PCM.  Current for
// the calling thread while a handle's forward enqueues its kernels, like the tuning scope above; null outside.
extern thread_local int* t_status;
struct StatusScope {
    int* prev;
    explicit StatusScope(int* p) : prev(t_status) { t_status = p; }
    ~StatusScope() { t_status = prev; }
};

// ---- gemm.hip -----------------------------------------------------------------------------------------
struct GemmParams {
    const void* A;  // (batches, M, K) rows at A + b*a_bs + m*lda (elements of the compute dtype)
    long lda, a_bs;
    const void* W;  // (N, K) row-major, compute dtype
    const void* W_x3 = nullptr;  // fp32 mode only: the same matrix pair-packed as bf16 hi / lo (gemm_x3.hip), or null
    const float* bias;
    int M, N, K, batches;
    int act;                // 0 none, 1 erf-GELU (2: its one-transcendental form, set by launch_gemm), 3 swish x*sigmoid(x)
                            // (Conformer FFNs; the fp32 kernels of gemm.hip / gemmt.hip only)
    const float* residual;  // fp32, indexed like out32; added after the activation
    const int* row_limit;   // per batch: rows >= row_limit[b] are written as 0
    // round 6 (second session): the residual is NOT read as stored — `residual` holds the INPUT rows t of a LayerNorm and the epilogue
    // adds LayerNorm(t) = ln_affine(t, mu, rs, gamma, beta) rebuilt from the row's statistics (res_ln_stats[m] = (mu, rs), written by
    // launch_layernorm(..., stats_out)): the post-LN layers' LayerNorm 1 no longer writes its fp32 output (49 MB per layer at the
    // reference batch), fc2 re-reads the row it normalised.  gemm16_big residual epilogue only (gemm16_res_ln_ok)
    const float2* res_ln_stats = nullptr;
    const float* res_ln_g = nullptr;
    const float* res_ln_b = nullptr;
    float* out32;
    void* out16;
    long ldo, o_bs;
    int variant = -1;  // tuning knob: -1 = the current tuning().gemm_variant
    // 16-bit modes: W row stride in elements (0 = K, or 2K with wsplit) and the two-term weight split of S3ENC_F16X2:
    // every W row is [hi(K) | lo(K)] with w = hi + lo (two fp16), and the contraction runs over 2K with A read twice:
    //   sum_k a[k] * hi[k] + sum_k a[k] * lo[k]   — the weights' rounding error disappears at twice the matrix cost
    long ldw = 0;
    int wsplit = 0;
    // S3ENC_F16X2, round 5: the lo term as an MX-fp4 image — W4: (N, K/32, 16 bytes) e2m1 nibbles, element e of a block in nibble e;
    // W4s: (N, K/32) E8M0 scale bytes; mxw: run the contraction over the hi half of the [hi | lo] rows + this image (gemm16.hip, MXW)
    // instead of over both halves.  Set by the engine when the image exists; launch_gemm falls back to `wsplit` when the shape is
    // not the MX kernel's (gemm16_mx_eligible).
    const void* W4 = nullptr;
    const void* W4s = nullptr;
    int mxw = 0;
};
bool gemm16_mx_eligible(int dtype, const GemmParams& p);
bool gemm16_mx_weight_rule(long N, long K);  // which weights get an MX image at s3enc_create (per weight, batch-independent)
// gemm_x3.hip: fp32-class GEMM from three bf16 MFMAs per product (opt-in compute mode S3ENC_F32X3)
bool gemm_x3_eligible(const GemmParams& p);
hipError_t launch_gemm_x3(const GemmParams& p, hipStream_t stream);
void pack_x3(const float* w, long N, long K, std::vector<uint16_t>& out);  // host: fp32 (N, K) -> pair-packed bf16 hi / lo
// gemm16.hip: large-tile LDS-DMA kernel for the 16-bit modes (tuning().gemm16_big)
bool gemm16_big_eligible(int dtype, const GemmParams& p);
bool gemm16_res_ln_ok(int dtype, const GemmParams& p);  // may this call carry GemmParams::res_ln_* ?
hipError_t launch_gemm16_big(int dtype, const GemmParams& p, hipStream_t stream);
// gemmt.hip: (256 | 192 | 128 | 64) x 128 tiles, several independent workgroups per CU; fp32 results bit-identical to
// gemm.hip's kernel.  tuning().gemm32_big (fp32) / .gemm_x3_tile (S3ENC_F32X3 = dtype code 3 below: fp32 operands, the
// pair-packed p.W_x3)
bool gemm_tile_eligible(int dtype, const GemmParams& p);
// The schedule of one fp32 launch: per batch `m_bulk` tiles of 64 tm rows from row 0, then `m_tail` tiles of 64 rows (the last
// one of a region may be ragged); both regions cover every 128-column tile and every batch.  Host arithmetic on (M, N, batches,
// tm, the "gemm32_tail" setting, its probe units, CUs) only.  gemm_tile_items lists the (batch, m0, rows, n0) of every
// workgroup in blockIdx order through the kernel's own block -> tile map (s3enc_debug_gemm_schedule).
struct GemmTileSched {
    int tm, m_bulk, m_tail;
};
GemmTileSched gemm_tile_schedule(int M, int N, int batches, int tm, int tail_mode, int tail_units, int cus);
void gemm_tile_items(int M, int N, int batches, const GemmTileSched& s, std::vector<int>& items4);
hipError_t launch_gemm_tile(int dtype, const GemmParams& p, hipStream_t stream);
hipError_t launch_gemm(int dtype, const GemmParams& p, hipStream_t stream);
// convf22.hip: exact-fp32 Conv1d(C, C, k = 3, stride = 2) on channel-last rows in the two-output form (5 block products per
// pair of outputs instead of 6).  out[b][t] = act(W0 x[2t] + W1 x[2t+1] + W2 x[2t+2] + bias), W = (C, 3C) tap-major, WP = W0 + W2
struct ConvF22Params {
    const float* x;     // (batches, L_in, C) rows, utterance b at x + b * x_bs
    long x_bs;          // elements per utterance (L_in * C)
    const float* W;     // (C, 3C) [n][j*C + c]
    const float* WP;    // (C, C) fl(W0 + W2)
    const float* bias;  // [C] or null
    int M, C, batches;  // M = output frames per utterance
    int act;            // 0 none, 1 erf-GELU (the launcher maps it like launch_gemm)
    const int* row_limit;
    float* out;         // (batches, M, C), utterance b at out + b * o_bs
    long o_bs;
};
bool conv_f22_eligible(const ConvF22Params& p);  // tuning().conv_f22, C a multiple of 32, alignment, 32-bit offsets
const char* conv_f22_refusal(const ConvF22Params& p);  // null, or why launch_conv_f22 would refuse (eligibility, then M, B, x_bs, o_bs)
hipError_t launch_conv_f22(const ConvF22Params& p, hipStream_t stream);
// convtaps.hip: exact-fp32 stride-1 Conv1d on channel-last rows whose K walk is up to two tap runs (NPC's masked convolutions:
// the masked taps in the middle are neither fetched nor multiplied), with a pre-activation residual and up to three destinations.
// Utterance b's operand is P zero rows, T data rows, P zero rows; `src` points at the row that tap 0 of output row 0 reads.
struct ConvTapsParams {
    const float* src;    // utterance b at src + b * src_bs; output row t, tap j reads the C floats at src + b * src_bs + (t + j) * C
    long src_bs;
    int C;               // input channels, a multiple of 16
    const float* W;      // (N, (taps0 + taps1) * C): the live taps only, tap-major (pack_conv_taps)
    const float* bias;   // [N] or null
    int T, N, B;
    int taps0, gap, taps1;  // run 0 = taps [0, taps0); `gap` masked taps; run 1 = the taps1 taps behind them (0: one run)
    int act;             // 0 none, 1 ReLU, 2 tanh — applied to acc + bias + res
    const float* res;    // optional: row (b, t) at res + b * res_bs + t * ld_res, added BEFORE the activation
    long res_bs, ld_res;
    float* dst;          // optional: row (b, t) at dst + b * dst_bs + t * ld_dst (a bordered operand: point it at the first data row)
    long dst_bs, ld_dst;
    float* state;        // optional: a second copy, same addressing (a contiguous (B, T, N) state slot)
    long state_bs, ld_state;
    float* sum;          // optional: sum = sum_init ? v : sum + v
    long sum_bs, ld_sum;
    int sum_init;
};
// host: nn.Conv1d's (N, C, k) weight -> the kernel's (N, live * C) image; taps [(k - mask) / 2, (k + mask) / 2) are masked.
// dense: all k taps, the masked ones stored as zeros (the form the skip form must equal)
void pack_conv_taps(const float* w, int N, int C, int k, int mask, bool dense, std::vector<float>& out);
const char* conv_taps_refusal(const ConvTapsParams& p);  // null, or why launch_conv_taps would refuse
hipError_t launch_conv_taps(const ConvTapsParams& p, hipStream_t stream);
// conv2d.hip: exact-fp32 stride-1 3 x 3 Conv2d(C, N, padding = 1) on channel-last images + bias + ReLU + optional 2 x 2 / stride-2
// max-pool in one pass (VGGish's features stack).  Example b's operand is an (H + 2) x (W + 2) x C image with a zero border; the
// result goes to the interior of a (Ho + 2 dst_pad) x (Wo + 2 dst_pad) image of pixel pitch ld_dst (Ho, Wo = H, W, halved under
// pool), whose border is never touched.  C = 1 runs the VALU first-layer kernel, any other C (a multiple of 16) the MFMA kernel.
struct Conv2dParams {
    const float* src;    // example b at src + b * src_bs; bordered pixel (r, c) at + (r * (W + 2) + c) * C
    long src_bs;
    int C;               // input channels: 1, or a multiple of 16
    const float* Wt;     // pack_conv2d3x3: (N, 9 C) with k = (ky * 3 + kx) * C + c; C = 1: (9, N)
    const float* bias;   // [N] or null
    int H, W, N, B;
    int act;             // 0 none, 1 ReLU
    int pool;            // 1: 2 x 2 / stride-2 max-pool behind the activation (H, W even)
    float* dst;          // example b at dst + b * dst_bs; output pixel (y, x) at + ((y + dst_pad) * (Wo + 2 dst_pad) + x + dst_pad) * ld_dst
    long dst_bs;
    int dst_pad;
    long ld_dst;
    // BYOL-A's additions; all zero is the launch as it was (VGGish's)
    const float* scale;  // [N] or null: v = act(acc * scale[n] + shift[n]) — an eval-mode BatchNorm behind the conv; `bias` must be null
    const float* shift;  // [N], with scale
    int pool_floor;      // under pool: odd H / W allowed, Ho = H / 2 and Wo = W / 2 rounded down (nn.MaxPool2d's floor mode); the
                         // dropped last row / column is never computed
    int n64;             // 1: Cout <= 64 may run on the 64-wide n-tile (tuning().conv2d_n64); same bits as the 128-wide one
    // BYOL-S's additions (the ResNet's layers); all zero is the launch as it was
    int gen;             // 1: the general instantiation: k x k taps at padding (k - 1) / 2 and stride 1 or 2 over the SAME bordered
                         // (H + 2) x (W + 2) operand, Ho = (H + 2 p - k) / stride + 1 as nn.Conv2d rounds, the epilogue act(acc *
                         // scale[n] + shift[n] + res[pixel][n]); no pooling, C a multiple of 16.  k = 3, stride = 1, no residual is
                         // bit for bit the launch without `gen`
    int k;               // with gen: 3, or 1 (Wt is then the plain (N, C) matrix and the border is never read)
    int stride;          // with gen: 1 or 2
    const float* res;    // with gen, or null: example b at res + b * res_bs, output pixel (y, x) at + ((y + res_pad) * (Wo + 2 res_pad)
    long res_bs;         // + x + res_pad) * ld_res; added behind the affine and before the activation (a BasicBlock's identity)
    int res_pad;
    long ld_res;
};
void pack_conv2d3x3(const float* w, int N, int C, std::vector<float>& out);  // host: nn.Conv2d's (N, C, 3, 3) -> the kernel's image
const char* conv2d3x3_refusal(const Conv2dParams& p);  // null, or why launch_conv2d3x3 would refuse
hipError_t launch_conv2d3x3(const Conv2dParams& p, hipStream_t stream);
__host__ __device__ inline int conv2d_out(int H, int k, int stride) { return (H + 2 * ((k - 1) / 2) - k) / stride + 1; }  // nn.Conv2d's output size

// stem.hip: BYOL-S's ResNet stem on single-channel (H, 64) images, exact fp32 on the VALU (K = 49 is not matrix work): a 7 x 7
// convolution at stride 1 and padding 3 to 64 channels, the per-channel affine (an eval-mode BatchNorm), ReLU, and MaxPool2d(3, 2, 1):
// Hp = (H - 1) / 2 + 1 rows of 32 pixels.  fused = 1: one kernel, every pooled pixel computes the 3 x 3 un-pooled pixels of its window
// (2.25 x the multiply-adds, the un-pooled map never exists); fused = 0: the un-pooled map is written to `map`, a second kernel pools
// it.  Both forms walk the 49 taps in one order and give the same bits.  Every pooled value is behind the ReLU (negative zero is
// written as +0), so the zero border of `map` stands for -inf padding; a NaN stays a NaN.
struct StemParams {
    const float* src;    // example b at src + b * src_bs: an (H + 8) x (64 + 8) image whose 4 outermost rows / columns are zeros
    long src_bs;
    int H, B;
    const float* Wt;     // pack_stem7x7: (49, 64), tap-major
    const float* scale;  // [64]
    const float* shift;  // [64]
    float* dst;          // example b at dst + b * dst_bs: an (Hp + 2) x (32 + 2) x 64 image; its interior is written, its border never touched
    long dst_bs;
    int fused;
    float* map;          // fused = 0: example b at map + b * map_bs, an (H + 2) x (64 + 2) x 64 image with a zero border
    long map_bs;
};
void pack_stem7x7(const float* w, std::vector<float>& out);  // host: nn.Conv2d's (64, 1, 7, 7) -> (49, 64)
const char* stem_refusal(const StemParams& p);               // null, or why launch_stem would refuse
hipError_t launch_stem(const StemParams& p, hipStream_t stream);

// patchembed.hip: exact-fp32 patch embedding of (frames, 128) images as an implicit GEMM over the tokens of all utterances (MAE-AST's
// nn.Unfold((kt, kc), stride = kernel) + Linear + position row): token t * V + v of utterance b is the kt x kc patch at image row
// t * kt, column v * kc, V = 128 / kc, its content in (time, channel) row-major order — the Linear's own K order.
struct PatchEmbedParams {
    const float* img;   // utterance b at img + b * img_bs: rows of 128 floats; rows at or past Tt * kt are never read
    long img_bs;        // floats, a multiple of 4, at least Tt * kt * 128
    const float* W;     // (N, kt * kc) row-major
    const float* bias;  // [N] or null
    const float* pos;   // (>= Tt * V, N) or null: row m is added to token m of utterance b where m < kv[b]
    const int* kv;      // device [B], with pos
    int B, Tt, kt, kc, N;
    int vshift, sshift;  // log2(128 / kc), log2(kc / 16): patch_embed_geometry fills them
    float* out;         // (B, Tt * V, N) contiguous
};
void patch_embed_geometry(PatchEmbedParams& p);            // vshift / sshift from kc (0 / 0 for a kc the kernel refuses)
const char* patch_embed_refusal(const PatchEmbedParams& p);  // null, or why launch_patch_embed would refuse
hipError_t launch_patch_embed(const PatchEmbedParams& p, hipStream_t stream);
// the two-step form: a gather into `rows` (patch_embed_rows_elems floats, 16-byte aligned), launch_gemm, the position add
size_t patch_embed_rows_elems(const PatchEmbedParams& p);
hipError_t launch_patch_embed_two_step(const PatchEmbedParams& p, float* rows, hipStream_t stream);

// patchstrided.hip: exact-fp32 patch embedding with overlapping patches (SSAST's Conv2d(1, N, (fshape, tshape), stride (fstride,
// tstride)) on the transpose of a (rows, 128) image) as an implicit GEMM over the tokens of all windows.  Token (ti, fi) of window w is
// the tshape x fshape patch at image row ti * tstride, column fi * fstride, its content in (time, frequency) row-major order; it is row
// 2 + ti * f_dim + fi of the window's sequence of 2 + f_dim * t_dim rows (time-major), behind the two prefix rows.
struct PatchStridedParams {
    const float* img;     // window w at img + w * img_bs: `rows` rows of 128 floats; nothing behind them is read
    long img_bs;          // floats, a multiple of 4, at least rows * 128
    const float* W;       // (N, tshape * fshape) row-major: the conv weight permuted to [n][t][f]
    const float* bias;    // [N] or null
    const float* pos;     // (f_dim * t_dim, N) in the time-major token order, or null
    const float* prefix;  // (2, N): rows 0 and 1 of every sequence, or null (they are then left as they are)
    int nwin, rows, fshape, tshape, fstride, tstride, N;
    int f_dim, t_dim, sshift;  // (128 - fshape) / fstride + 1, (rows - tshape) / tstride + 1, log2(fshape / 16): patch_strided_geometry
    float* out;           // (nwin, 2 + f_dim * t_dim, N) contiguous
};
void patch_strided_geometry(PatchStridedParams& p);              // f_dim / t_dim / sshift (0 where the geometry has none)
const char* patch_strided_refusal(const PatchStridedParams& p);  // null, or why launch_patch_strided would refuse
hipError_t launch_patch_strided(const PatchStridedParams& p, hipStream_t stream);
hipError_t launch_patch_strided_tile(const PatchStridedParams& p, int tile_rows, hipStream_t stream);  // 64 | 128: the tile height named
// the two-step form: a gather into `rows` (patch_strided_rows_elems floats, 16-byte aligned), launch_gemm per window, the position add
size_t patch_strided_rows_elems(const PatchStridedParams& p);
hipError_t launch_patch_strided_two_step(const PatchStridedParams& p, float* rows, hipStream_t stream);

// ---- frontend.hip ---------------------------------------------------------------------------------------
// Waveform table: wav b is `ptrs[b]` with `lens[b]` valid samples; reads beyond are zeros (the padding).
struct WavTable {
    const float* const* ptrs;  // device array [B]
    const long* lens;          // device array [B]
    int B;
    long n_max;
};
constexpr int STAT_K0_MAX = 16;  // conv0 kernel width limit for the closed-form GroupNorm statistics
// per-utterance mean / rstd of the raw waveform (task_cfg.normalize); norm[b] = {mean, rstd}; identity if !normalize
hipError_t launch_wav_norm_stats(const WavTable& w, int normalize, double* partial, float2* norm, hipStream_t s,
                                 float eps = 0.f /* 0 = LN_EPS; Hugging Face feature extractors: 1e-7 */);
// GroupNorm(C,C) statistics of conv0's output from the k0 + k0*(k0+1)/2 lag sums of the waveform, then the
// fused per-(b,c) affine:  gn[b][c] = {scale, shift} with  y = conv0_raw * scale + shift
hipError_t launch_gn_stats(const WavTable& w, const float2* norm, const float* w0 /*[C][k0]*/, const float* gamma,
                           const float* beta, int C, int k0, int s0, long L0, double* partial, double* sums,
                           float2* gn, hipStream_t s);
size_t stats_partial_elems(int B, long n_max);  // doubles needed for `partial`
struct Conv0Params {
    WavTable wav;
    const float2* norm;   // [B] {mean, rstd}
    const float* w0;      // [C][k0]
    const float* bias;    // [C] or null
    const float2* gn;     // [B][C] {scale, shift} (GroupNorm mode) or null
    const float* ln_g;    // [C] (layer_norm mode) or null
    const float* ln_b;
    int C, k0, s0;
    long L0;
    void* out;            // (B, L0, C) compute dtype
    int fast = 0;         // fp32 output with the packed one-transcendental GELU (the split-precision modes)
    int nt = 0;           // fp32 output: non-temporal stores
    int relu = 0;         // wav2vec: ReLU instead of GELU behind the GroupNorm table (fp32 output, gn != null)
};
// wav2vec: GroupNorm(1, C) statistics of conv0's output (one mean / variance per utterance over all C x L0 values) from the
// waveform's lag sums, as the per-(b, c) table {rstd * gamma_c, beta_c - mean * rstd * gamma_c}; gamma / beta may be null (1 / 0)
hipError_t launch_gn1_stats(const WavTable& w, const float2* norm, const float* w0 /*[C][10]*/, const float* gamma,
                            const float* beta, int C, int k0, int s0, long L0, double* partial, float2* gn, hipStream_t s);
hipError_t launch_conv0(int dtype, const Conv0Params& p, hipStream_t s);

// ---- norm.hip -------------------------------------------------------------------------------------------
// Featurizer term fused into a row kernel: acc[row] (+)= w * state_row  (norm: w * layer_norm(state_row), no affine)
struct LnAcc {
    float* acc = nullptr;  // (rows, C) fp32
    float w = 0.f;
    int mode = 0;  // 0 none; 1: the kernel's INPUT row is the state; 2: its OUTPUT row is
    int norm = 0;
    int init = 0;  // first term: write instead of add
};
// WavLM gate (wavlm/modules.py:535-549) of the attention module that will read this LayerNorm's OUTPUT, fused into the
// LayerNorm pass (the row is in registers): gate[b][h][t] for the (b, t) row; needs C == H * 64.  Replaces a separate
// pass over the (B*T, D) fp32 tensor (and, in the 16-bit modes, the fp32 copy written only for it).
struct LnGate {
    const float* gw = nullptr;  // grep_linear.weight (8, 64)
    const float* gb = nullptr;  // grep_linear.bias (8)
    const float* ga = nullptr;  // grep_a (H)
    float* gate = nullptr;      // (B, H, T) or null: no gate
    int T = 0, H = 0;
};
// act: 0 none, 1 erf-GELU of the mode (16-bit: common.h gelu_fast; fp32: the same unless tuning gelu32 = 0 -> libm erff),
//      2 gelu_fast regardless of dtype and tuning
hipError_t launch_layernorm(int dtype, const float* x, const float* gamma, const float* beta, long rows, int C, int act,
                            float* out32, void* out16, hipStream_t s, const LnAcc& fa = LnAcc(), const LnGate& gt = LnGate(),
                            float2* stats_out = nullptr);  // stats_out[row] = (mean, 1 / sqrt(var + eps)) of the row
// a state produced by a non-LayerNorm kernel: its 16-bit copy (out16, dtype BF16 / F16) and / or its Featurizer term
hipError_t launch_emit_state(int dtype, const float* x, long rows, int C, void* out16, const LnAcc& fa, hipStream_t s);
hipError_t launch_add(const float* a, const float* b, float* out, long n, hipStream_t s);  // out = a + b, n % 4 == 0

// ---- attention.hip ----------------------------------------------------------------------------------------
struct AttnParams {
    const void* qkv;  // (B*T, 3D): q | k | v, q already scaled by head_dim^-0.5
    void* out;        // (B*T, D)
    const int* valid; // [B] keys >= valid[b] are masked
    int B, T, H;
    const float* bias_table;  // WavLM: [H][2R+1], entry (h, clamp(key - query, -R, R) + R), or null
    int table_R = 0;
    const float* gate;        // WavLM: [B][H][T] or null (then gate = 1)
    int out_f32 = 0;          // 16-bit kernels only: write the (B*T, D) result as fp32 (S3ENC_F16X2: out_proj then reads it
                              // through the three-term GEMM — its operand's rounding is the largest non-conv term of the mode's error)
    int probe = 0;            // timing probes (tools/micro/attn_lab.hip builds the kernels with S3_ATTN_PROBE; ignored otherwise)
    // Conformer rel_pos (Transformer-XL relative attention, wav2vec2_model.py:165-252), fp32 only: score(i, j) += (q_i + qadd_h) .
    // rel_P[(j - i) + T - 1][h*64 .. h*64+63] with rel_P = linear_pos(pe) for THIS T ((2T-1, D) rows, row stride D) and
    // qadd = (pos_bias_v - pos_bias_u) * head_dim^-0.5 (q arrives as (q + pos_bias_u) * head_dim^-0.5).  No bias table / gate.
    const float* rel_P = nullptr;
    const float* rel_qadd = nullptr;  // (H, 64)
};
hipError_t launch_attention(int dtype, const AttnParams& p, hipStream_t s);
// WavLM gate (wavlm/modules.py:535-549) from the layer input x (fp32 rows of D): gate[b][h][t]
hipError_t launch_wavlm_gate(const float* x, const float* grep_w /*[8][64]*/, const float* grep_b /*[8]*/,
                             const float* grep_a /*[H]*/, int B, int T, int H, float* gate, hipStream_t s);

// ---- conformer.hip (wav2vec 2.0 Conformer block, wav2vec2_model.py:313-393,25-71) ------------------------------------
struct ConformerConvParams {
    const float* x;      // (B*T, 2D) fp32: pointwise_conv1's output (a | g halves of the GLU)
    const float* taps;   // (D, K) depthwise taps with BatchNorm's scale folded in
    const float* shift;  // (D) BatchNorm's folded shift
    float* out;          // (B*T, D) fp32 = swish(BN(DW(GLU(x))))
    int B, T, D, K;      // K odd, <= 63; zero padding (K-1)/2 inside each utterance's T-row block
};
hipError_t launch_conformer_conv(const ConformerConvParams& p, hipStream_t s);
// rot(x) per 64-wide head chunk; table: (>= T, 64) fp32 rows {cos[32], sin[32]} of position t = row % T
hipError_t launch_rope(const float* x, const float* table, long rows, int T, int D, float* out, hipStream_t s);

// ---- posconv.hip --------------------------------------------------------------------------------------------
struct PosConvParams {
    const float* x;     // (B, T, D) fp32, padded frames already zero
    const void* w;      // fp32 mode: packed [G][K][Dg/16][Dg(n)][16] (+ [Dg(n)][8] at Dg = 24, 40: pack_posconv); 16-bit modes: see launch_posconv16
    const float* bias;  // [D]
    float* out;         // (B, T, D) fp32 = x + gelu(conv(x) + bias)
    int B, T, D, G, K;
    int pad = -1;       // left zero padding in frames; -1 = K / 2 (a K padded with zero taps keeps the real kernel's K / 2)
    int plain = 0;      // 1: out = conv(x) + bias only (data2vec's conv -> LayerNorm -> GELU stack, wav2vec2_model.py:2999-3017)
};
hipError_t launch_posconv(const PosConvParams& p, hipStream_t s);
// fp32 pack: slot permutation inside a 16-float weight row.  ds_read_b128 serves a wave in four groups of 16 lanes ({0-3, 12-15,
// 20-27}, ... — MI355X_MICROARCH.md §LDS); lane (co & 15, s) reads slot s of row co.  Rows are 64 bytes, so rows co and co + 4
// start on the same bank: with the slots of rows 8..15 XORed by 2, the 16 lanes of every group touch 16 different slot positions
// modulo the 256-byte bank row (round 3 measured SQ_LDS_BANK_CONFLICT / active = 0.315 on the linear layout).
__host__ __device__ inline int pc_w_swizzle(int co) { return ((co & 15) >> 3) << 1; }
// 16-bit operand modes: p.w = 16-bit pack [G][Dg][K*Dg] with k = tap*Dg + ci; x / out / bias fp32
hipError_t launch_posconv16(int dtype, const PosConvParams& p, hipStream_t s);

// ---- adapter.hip (multires-HuBERT: the row passes of the conv adapters, multires_hubert/hubert_model.py:970-1266) ------
// Operand geometry of the adapter convolutions: per utterance `total` rows of D — `lead` zero rows, the data rows, zero
// rows to the end — so that a Conv1d / ConvTranspose1d window that hangs over either end reads zeros and the convolution
// is a plain GEMM over contiguous k*D-element rows (multires.hip; weights packed by load_conv in engine.hip).
struct PadCopyParams {
    const float* a;      // (B, >= rows, D) fp32, utterance b at a + b*a_bs
    long a_bs;
    const float* b;      // optional second term added row by row (x + residual, align_size_sum), or null
    long b_bs;
    int B, rows, D;      // data rows copied per utterance
    int lead, total;     // output rows: [0, lead) zero, [lead, lead + rows) data, [lead + rows, total) zero
    const int* zero_from;  // optional [B]: data rows >= zero_from[b] are written as zero
    float* out32;        // (B, total, D) fp32 and / or ...
    void* out16;         // ... the 16-bit compute dtype; either may be null
};
hipError_t launch_pad_copy(int dtype, const PadCopyParams& p, hipStream_t s);
constexpr int GS_BLOCKS = 64;  // partial sums per utterance of the one-group GroupNorm statistics
// partial[b][blk] = {sum, sum of squares} over slice blk of the `count` contiguous fp32 values at x + b*bs
hipError_t launch_group1_stats(const float* x, long bs, long count, int B, double* partial /*[B][GS_BLOCKS][2]*/, hipStream_t s);
struct AdapterApplyParams {
    const float* conv;      // (B, L, D) fp32 conv output, utterance b at conv + b*conv_bs
    long conv_bs;
    const double* partial;  // launch_group1_stats of that output
    double count;           // elements per utterance the statistics run over (L * D: ALL conv frames, kept or not)
    const float* gamma;     // GroupNorm(1, D) affine
    const float* beta;
    const float* r1;        // skip term: row (t * r1_mul) / r1_div of utterance b at r1 + b*r1_bs
    long r1_bs;
    int r1_mul, r1_div;
    const float* r2;        // highway term (ConvAdapter) or null
    long r2_bs;
    int r2_mul, r2_div;
    float scale;            // sqrt(residual_scale)
    int B, rows, D;         // kept output frames per utterance
    int lead, total;        // output geometry as in PadCopyParams (lead = 0, total = rows: a plain (B, rows, D) tensor)
    const int* zero_from;   // optional [B]: frames >= zero_from[b] are written as zero (the next encoder's index_put)
    float* out32;
    void* out16;
    int fast_gelu;          // fp32 instantiation only: gelu_fast (S3ENC_F32X3); the 16-bit ones always use it
};
hipError_t launch_adapter_apply(int dtype, const AdapterApplyParams& p, hipStream_t s);
// state of a block -> (B, rows_out, D) slot: out[b][t] = x[b][t / factor]  (repeat_interleave + cut, expert.py:26-27,93-101)
hipError_t launch_emit_upsampled(int dtype, const float* x, long x_bs, int factor, int B, int rows_out, int D, float* out32,
                                 void* out16, hipStream_t s);

// the same state as its Featurizer term only: fa.acc[b][t] (+)= fa.w * (fa.norm ? layer_norm(x[b][t / factor]) : x[b][t / factor])
hipError_t launch_emit_upsampled_acc(const float* x, long x_bs, int factor, int B, int rows_out, int D, const LnAcc& fa,
                                     hipStream_t s);

// ---- wav2vec.hip (wav2vec / vq-wav2vec: upstream/wav2vec/wav2vec_model.py:59-286, wav2vec2_model.py:1591-1782) ------------
// The row pass behind every convolution but the first: GroupNorm(1, C) + ReLU from the double partials of launch_group1_stats,
//   y = relu((x - mean_b) * rstd_b * gamma_c + beta_c);  res: y = (y + res) * scale;  log: y = log(|y| + 1)
// written to up to three places in one pass: `dst` (the next convolution's operand: per utterance `pad` rows in front of the
// `rows` data rows, filled with frame 0 — ReplicationPad1d — or zeros), `state` (a (B, rows, C) hidden-state slot) and the
// Featurizer term `acc`.  dst == x with pad == 0 works in place.
struct Gn1ApplyParams {
    const float* x;         // (B, rows, C) raw conv output, utterance b at x + b * x_bs
    long x_bs;
    const double* partial;  // [B][GS_BLOCKS][2] of launch_group1_stats over that output
    double count;           // rows * C
    const float* gamma;     // [C] or null (non_affine_group_norm)
    const float* beta;
    const float* res;       // skip term: row t of utterance b at res + b * res_bs + t * C, or null
    long res_bs;
    float scale;            // sqrt(residual_scale), used with res
    int log;                // log(|y| + 1) (log_compression)
    int B, rows, C;
    int pad, pad_zero;      // rows in front of every utterance in dst; 1 = zeros (agg_zero_pad), 0 = copies of frame 0
    float* dst;             // (B, pad + rows, C), utterance b at dst + b * dst_bs; or null
    long dst_bs;
    float* state;           // (B, rows, C) contiguous, or null
    LnAcc acc;              // mode != 0: acc.acc (B, rows, C) (+)= w * (norm ? layer_norm(y) : y)
};
hipError_t launch_gn1_apply(const Gn1ApplyParams& p, hipStream_t s);
// Per (row, group): the index of the largest of V scores (ties: the lowest index, like torch.max / argmin of the negated
// distances), as int64, and the gathered codeword.  scores: (rows, G, V); table: (Gt, V, Dv) with Gt = G, or 1 when the
// groups share their variables (combine_groups); ids: (rows, G) or null; out: (rows, G * Dv) or null.
struct ArgmaxGatherParams {
    const float* scores;
    const float* table;
    int shared;  // 1: table has one group
    long rows;
    int G, V, Dv;
    long long* ids;
    float* out;
};
hipError_t launch_argmax_gather(const ArgmaxGatherParams& p, hipStream_t s);
hipError_t launch_relu(float* x, long n, hipStream_t s);  // in place, n % 4 == 0
// (B, rows, C) contiguous -> the padded operand geometry of Gn1ApplyParams::dst
hipError_t launch_w2v_pad_rows(const float* x, int B, int rows, int C, int pad, int pad_zero, float* dst, hipStream_t s);
// k-means quantizer (wav2vec_model.py:117-232) behind the grouped 1x1 projection: GroupNorm(G, C) statistics per (b, group) over
// the (rows x Cg) block of proj, then scores[row][g][v] = -|| norm(proj)[row][g] - emb[v][g] ||^2.  emb_t: (G, Cg, V).
hipError_t launch_kmeans_stats(const float* proj, int B, int rows, int C, int G, float2* stats, hipStream_t s);
hipError_t launch_kmeans_scores(const float* proj, const float2* stats, const float* gamma, const float* beta, const float* emb_t,
                                int B, int rows, int C, int G, int V, float* scores, hipStream_t s);

// ---- cpc.hip (modified CPC encoder: upstream/cpc/model.py:33-104) ------------------------------------------------------
// conv0 from the waveform table: Conv1d(1, C, k0 = 10, stride s0, padding pad0) + bias -> ChannelNorm (per frame over the C
// channels, unbiased variance, eps 1e-5) -> ReLU, written channel-last into the next convolution's operand: per utterance
// `pad` zero rows, the L0 frames, `pad` zero rows.  Samples outside [0, lens[b]) read as zero.
struct CpcConv0Params {
    WavTable wav;
    const float* w0;     // [C][10]
    const float* bias;   // [C]
    const float* gamma;  // [C] or null
    const float* beta;
    int C, s0, pad0;
    long L0;
    int pad;             // border rows of dst
    float* dst;          // (B, pad + L0 + pad, C)
};
hipError_t launch_cpc_conv0(const CpcConv0Params& p, hipStream_t s);
// The row pass behind conv1..: ChannelNorm + ReLU of the raw convolution output (bias already added), a wave per frame.
struct ChannelNormParams {
    const float* x;      // (B, rows, C) contiguous
    const float* gamma;  // [C] or null
    const float* beta;
    int B, rows, C;
    int pad;             // zero rows in front of and behind every utterance in dst
    float* dst;          // (B, pad + rows + pad, C) or null
    float* state;        // (B, rows, C) or null
};
hipError_t launch_channelnorm_relu(const ChannelNormParams& p, hipStream_t s);

// ---- rnn.hip (nn.LSTM / nn.GRU recurrence, one workgroup per utterance, all T steps in one launch) ---------------------
constexpr int RNN_H_MAX = 512;  // hidden width limit (a multiple of 64): gate rows are walked by up to 1024 threads, two rows each
struct RnnParams {
    int cell;            // 0 LSTM (i, f, g, o), 1 GRU (r, z, n)
    const float* pre;    // row (b, t) at pre + (b * T + t) * ld_pre: gates * H values, x W_ih^T + the foldable biases
    const float* w;      // pack_rnn_whh image of weight_hh
    const float* b_hn;   // GRU: [H]; LSTM: null
    int B, T, H;
    long ld_pre;
    float* out;          // row (b, t) at out + (b * T + t) * ldo
    long ldo;
};
// host: weight_hh (gates * H, H) -> [H / 4][gates * H][4]: thread r of a step reads 16 consecutive bytes next to thread r + 1's
void pack_rnn_whh(const float* w, int gates, int H, std::vector<float>& out);
hipError_t launch_rnn(const RnnParams& p, hipStream_t s);
// The same recurrence with packed-sequence semantics (pack_padded_sequence / pad_packed_sequence; APC: upstream/apc/apc.py:118-139):
// utterance b stops at len[b] steps and its rows [len[b], T) are written as zeros.  For t < len[b] the row written is h_t (+ res[b, t]
// when `res` is given: the layer's residual operand); the carried state is the un-summed h_t.  A struct of its own, so that the
// kernels behind launch_rnn keep their argument block.
struct RnnLenParams : RnnParams {
    const int* len;      // device [B], each in 1..T
    const float* res;    // row (b, t) at res + (b * T + t) * ld_res, H values; or null
    long ld_res;
};
// out must be 16-byte aligned and ldo a multiple of 4 (the zero tail is written with 16-byte stores)
hipError_t launch_rnn_len(const RnnLenParams& p, hipStream_t s);
// The step-split form of launch_rnn_len: one launch per time step on a (S, B) grid, workgroup (s, b) owning H / S hidden units of
// utterance b with all their gate rows; bit-identical to launch_rnn_len for every S.  S a power of two, H / S a multiple of 64,
// S * B <= 256 (rnn_split_ok).
struct RnnStepParams : RnnLenParams {
    int S;               // workgroups per utterance
    int max_len;         // the largest len[b] (host): the number of launches
    int t;               // (set per launch)
    float* hbuf;         // device (2, B, H) ping-pong of h; need not be initialised
    float* cbuf;         // LSTM: device (B, H); GRU: null
};
bool rnn_split_ok(int H, int B, int S);
int rnn_split_pick(int cell, int H, int B);  // tuning().rnn_split, or its default rule: 0 = launch_rnn_len, S = launch_rnn_step
hipError_t launch_rnn_step(const RnnStepParams& p, hipStream_t s);

// ---- rnnb.hip (the batch-shared bidirectional LSTM step: W_hh read once per step for the whole batch, fp32 MFMA) ------------
constexpr int RNNB_H_MAX = 1024;  // hidden width limit (a multiple of 64)
constexpr int RNNB_B_MAX = 128;   // four 32-wide batch tiles per workgroup
struct RnnbParams {
    const float* pre_fwd;  // row (b, t) at pre + (b * T + t) * ld_pre: 4 H values (i, f, g, o), x W_ih^T + b_ih + b_hh
    const float* pre_bwd;  // the backward stack's, in the utterance's own time order (no flip)
    const float* w_fwd;    // pack_rnnb_whh image of the forward stack's weight_hh
    const float* w_bwd;
    const int* len;        // device [B], each in 1..T
    int B, T, H;
    long ld_pre;
    float* out;            // row (b, t) at out + (b * T + t) * ldo: forward h in columns [0, H), backward h in [H, 2 H)
    long ldo;              // a multiple of 4, at least 2 H
    int max_len;           // the largest len[b] (host): the number of launches
    int t;                 // (set per launch)
    float* hbuf;           // device, 2 * rnnb_state_elems floats: h ping-pong of both directions; need not be initialised
    float* cbuf;           // device, rnnb_state_elems floats
};
// host: weight_hh (4 H, H) -> [H / 8 slices][H / 8 k blocks][64 lanes][4]: lane l of slice s, k block kb holds
// w[(l & 31) / 8 * H + 8 s + (l & 7)][8 kb + 4 (l >> 5) + j], j = 0..3 — a workgroup's 32 rows are contiguous
void pack_rnnb_whh(const float* w, int H, std::vector<float>& out);
int rnnb_batch_pad(int B);                  // columns of the state buffers: 32, 64 or 128
size_t rnnb_state_elems(int B, int H);      // floats of cbuf (hbuf: twice that)
const char* rnnb_refusal(const RnnbParams& p);  // null, or why launch_rnnb would refuse
hipError_t launch_rnnb(const RnnbParams& p, hipStream_t s);

// ---- featurizer.hip (weighted sum over layers, the consumer of hidden_states) ---------------------
#define S3_WS_MAX_LAYERS 32
// out[row] = sum_l w[l] * (normalize ? layer_norm(hs[l][row]) : hs[l][row]);  w: HOST array (softmax already applied,
// 0 for unselected layers); hs[l] at hs + l*layer_stride, rows x D fp32
hipError_t launch_weighted_sum(const float* hs, long layer_stride, int L, const float* w_host, int normalize, long rows, int D,
                               float* out, hipStream_t st);
// grad_w[l] = sum <grad_out, hn_l>;  partial: device scratch of weighted_sum_bwd_blocks(rows) * L doubles
int weighted_sum_bwd_blocks(long rows);
hipError_t launch_weighted_sum_bwd(const float* hs, long layer_stride, int L, int normalize, long rows, int D,
                                   const float* grad_out, double* partial, float* grad_w, hipStream_t st);

// ---- fbank.hip (the `fbank` baseline upstream, BASELINE configs[0]) -----------------------------------------------
struct FbankParams {
    int sample_rate = 16000;
    int num_mel_bins = 80;
    float frame_length_ms = 25.f, frame_shift_ms = 10.f;
    float preemph = 0.97f;
    int delta_order = 2, delta_win = 5;
    int use_cmvn = 1;
    float cmvn_eps = 1e-10f;
    int window = 0;  // 0 povey (hann ** 0.85), 1 hamming (0.54 - 0.46 cos(2 pi i / (N - 1))), 2 hanning (0.5 - 0.5 cos(2 pi i / (N - 1))):
                     // kaldi's window_type
};
long fbank_num_frames(long n_samples, const FbankParams& c);
// one utterance: wav (device) -> out (device, frames x ldo), columns [0, num_mel_bins * (delta_order + 1))
hipError_t launch_fbank(const FbankParams& c, const float* wav, long n, float* out, int ldo, hipStream_t st);
// The batch-wide pass (delta_order 0, use_cmvn 1): one overlapping-row GEMM over the batch, one mel_rows launch, one CMVN launch with
// counts.  pcm: (B, row_stride) device rows, 16-byte aligned, row_stride a multiple of 4; frames: device [B] frame counts; out: (B, Fmax,
// ldo) with zeros behind an utterance's own frames and every valid row bit-equal to launch_fbank on that utterance alone.  spec: the
// caller's workspace of fbank_batch_workspace bytes; cap_bytes: the spectrum cap (0: fbank_batch_spec_cap, 128 MiB), above which the
// batch is walked fbank_batch_chunk whole utterances at a time
size_t fbank_batch_spec_cap();
int fbank_batch_chunk(int B, long Fmax, int nbin, size_t cap_bytes);
size_t fbank_batch_workspace(const FbankParams& c, int B, long Fmax, size_t cap_bytes);
hipError_t launch_fbank_batch(const FbankParams& c, const float* pcm, long row_stride, const int* frames, int B, long Fmax, float* out,
                              int ldo, float* spec, size_t spec_bytes, size_t cap_bytes, hipStream_t st);

// The window-wise pass (delta_order 0, use_cmvn 0): `nwin` windows of one length, each its own kaldi fbank of F frames (snip_edges), in
// one overlapping-row GEMM and one mel_rows launch whose epilogue is the affine (y + add) / div as two fp32 operations.  pcm: (nwin,
// row_stride) device rows, 16-byte aligned, row_stride a multiple of 4 and at least size + (F - 1) * shift; out: window w's F rows at out
// + w * out_bs + t * ldo, columns [0, nmel) — rows behind F are not touched (the caller's zeros).  spec: fbank_batch_workspace(c, nwin, F,
// cap_bytes) bytes.  A frame's log-mel is launch_fbank's arithmetic on that window alone: the same operand, K order and band sums.
hipError_t launch_fbank_windows(const FbankParams& c, const float* pcm, long row_stride, int nwin, long F, float add, float div, float* out,
                                long out_bs, int ldo, float* spec, size_t spec_bytes, size_t cap_bytes, hipStream_t st);

// ---- logmel.hip (OnlinePreprocessor: decibel scale, centred hann STFT on the padded batch, HTK mel, log, CMVN) --------
long logmel_num_frames(long max_len);               // 1 + max_len / 160
int logmel_frame_count(long length, long max_len);  // round(length / (max_len / T)) as Python rounds, clamped to [0, T]
size_t logmel_sig_elems(int B, long max_len);       // floats of LogmelParams::sig
size_t logmel_spec_elems(int B, long max_len);      // floats of LogmelParams::spec
struct LogmelParams {
    const float* const* wavs;  // device [B]
    const long* lens;          // device [B] samples
    const int* counts;         // device [B] frames the CMVN runs over (read only with cmvn)
    int B;
    long max_len;              // > 200: the length the batch is padded to
    int n_mels;
    float target_level;        // dB
    int cmvn;
    float* scale;              // scratch, B floats
    float* sig;                // scratch, logmel_sig_elems floats, 16-byte aligned
    float* spec;               // scratch, logmel_spec_elems floats
    float* out;                // row (b, t) at out + b * o_bs + t * n_mels, t < logmel_num_frames(max_len)
    long o_bs;
    int no_level;              // 1: no level scaling in front (the `mel` / `linear` baselines); 0 is Mockingjay's call, bit for bit
    int linear;                // 1: log(|X|^2 + 1e-10) of the 201 bins themselves, rows of 201 floats (n_mels is not read)
};
hipError_t launch_logmel(const LogmelParams& p, hipStream_t st);

// ---- melspec.hip (BYOL-A: per-segment centred 1024-point hann STFT, |X|^2, 64 HTK triangles 60..7800 Hz, log, (x - mean) / std) ----
long melspec_num_frames(long L);                 // 1 + L / 160
size_t melspec_sig_elems(long nseg, long L);     // floats of MelspecParams::sig
size_t melspec_spec_elems(long nseg, long L);    // floats of MelspecParams::spec
void melspec_bank(std::vector<int>& bands, std::vector<float>& wts);  // host: [3][64] first bin / bins / offset, and the weights
struct MelspecParams {
    const float* const* ptrs;  // device [nseg]: the segment's first sample (not read where valid <= 0)
    const int* valid;          // device [nseg]: samples readable behind ptrs[i]; the segment's samples at or past it are zeros
    int nseg;
    int L;                     // samples per segment, >= 1120; every segment is reflect-padded by 512 about its own ends
    float mean, std_;          // out = (log(mel + FLT_EPSILON) - mean) / std_
    float* out;                // value (i, t, m) at out + i * o_bs + t * o_row + m
    long o_bs, o_row;
    float* power;              // null, or (nseg, frames, 513): |X|^2 before the mel sum
    int fft;                   // 1 the FFT kernel, 0 the GEMM form (needs sig and spec)
    float* sig;                // GEMM form: melspec_sig_elems floats, 16-byte aligned
    float* spec;               // GEMM form: melspec_spec_elems floats
    // BYOL-S's additions; all zero is the launch as it was
    int win400;                // 1: MelSpectrogram(win_length = 400): a periodic hann(400) zero-padded to 1024 with 312 zeros in front
                               // (torch.stft's centring of a short window), a second window table of the FFT kernel; the FFT form only,
                               // and L only has to exceed 512 (the 8-frame rule is BYOL-A's network's)
    const int* lead;           // device [nseg] or null: samples of segment i before lead[i] are zeros (a window that starts in front of
                               // its utterance); ptrs[i] is then only ever read at offsets lead[i] .. valid[i] - 1
};
const char* melspec_refusal(const MelspecParams& p);  // null, or why launch_melspec would refuse
hipError_t launch_melspec(const MelspecParams& p, hipStream_t st);

// ---- mockingjay.hip (TF-style LayerNorm with a run-time eps; the input representation's row pass) -----------------
// y = (x (+ pos[row % Tc]) - mean) / sqrt(var + eps) * gamma + beta per row of C (biased variance), one wave per row.
// out: (rows, C) or null; out2: row r = (b, t) of a (B, Tp) layout goes to out2 + (b * T + t) * C when t < T (the rows the
// chunk padding adds are not emitted), or null.  In place (out == x) is allowed.
struct LnEpsParams {
    const float* x;
    const float* pos = nullptr;  // (>= Tc, C) or null
    int Tc = 1;
    const float* gamma;
    const float* beta;
    float eps;
    long rows;
    int C;
    float* out = nullptr;
    float* out2 = nullptr;
    int Tp = 1, T = 1;
};
hipError_t launch_layernorm_eps(const LnEpsParams& p, hipStream_t st);

}  // namespace s3
