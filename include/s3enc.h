/*
 * s3enc.h — C ABI of libs3enc.so: the MI355X (gfx950) speech-SSL upstream encoder.
 *
 * One hot path of s3prl, behind plain C:  raw 16 kHz waveforms  ->  the list of per-layer
 * hidden_states of a wav2vec 2.0 / HuBERT / WavLM encoder.  The reference is pure Python on top of
 * PyTorch ATen, so there is no reference FFI to bind; each entry point below names the reference
 * Python interface it stands in for (paths relative to the s3prl tree).
 *
 * Conventions
 *   - every function returns 0 on success, non-zero on failure; s3enc_last_error() (thread-local)
 *     describes the last failure.  Nothing throws across this boundary.
 *   - pointers documented "device" are HIP device pointers on the handle's GPU; "host" are host pointers.
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream).  Work is enqueued
 *     asynchronously on it and ordered with the caller's own work on that stream.
 *   - a handle is not re-entrant and serves ONE stream at a time: its workspaces are grown and released in the order of the
 *     stream of the call that grows them, so before moving a handle to another stream the caller orders that stream after
 *     the handle's last forward (an event, or a synchronise).  Distinct handles are independent (one per GPU / rank / stream).
 *   - there is no CPU fallback: without a gfx950 device s3enc_create fails.
 */
#ifndef S3ENC_H
#define S3ENC_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define S3ENC_VERSION 8
#define S3ENC_MAX_CONV 16
#define S3ENC_MAX_RES 4 /* resolutions of a multires-HuBERT U-net: up to 3 rate pairs, 7 encoder blocks */

typedef struct s3enc_encoder* s3enc_handle;

enum { S3ENC_HUBERT = 0, S3ENC_WAV2VEC2 = 1, S3ENC_WAVLM = 2,
       /* DistilHuBERT (upstream/distiller/model.py:83-268): HuBERT-style encoder without the LayerNorm before
        * post_extract_proj, wav2vec2's conv-length frame mask, prediction heads on the last layer */
       S3ENC_DISTILLER = 3,
       /* multi-resolution HuBERT (upstream/multires_hubert/hubert_model.py:337-852): a U-net of TransformerEncoders
        * (encoders[i] -> conv adapter -> ... middle_encoder ... -> conv adapter -> decoders[i] + skip) over the frame rates
        * of mr_ratios; HuBERT's frame mask; the states are every block's layer inputs and output, repeated to the
        * finest rate and cut to their common length (multires_hubert/expert.py:26-27,49-101) */
       S3ENC_MULTIRES = 4,
       /* wav2vec / vq-wav2vec (upstream/wav2vec/wav2vec_model.py:59-286,565-700, expert.py:15-62): a convolutional feature
        * extractor, an optional vector quantizer and a causal convolutional aggregator — no Transformer, no frame mask.  The
        * states are z (the extractor output) and every aggregator layer's output: n_agg + 1 states of (B, T, conv_dim).
        * compute_dtype S3ENC_F32 only. */
       S3ENC_WAV2VEC = 5,
       /* modified CPC (upstream/cpc/model.py:62-104,146-191, expert.py:25-49): five strided Conv1d layers with symmetric zero
        * padding, each followed by a per-frame channel norm and ReLU, then a multi-layer LSTM or GRU over the whole padded
        * time axis — no frame mask.  Two states of (B, T, width): the encoder output and the recurrent output.
        * compute_dtype S3ENC_F32 only; built by s3enc_create_cpc. */
       S3ENC_CPC = 6,
       /* APC / VQ-APC (upstream/apc/apc.py:101-169, audio.py:53-115, expert.py:18-59): a kaldi log-mel front end (hamming window, no
        * deltas, CMVN over time) and 3 or 4 unidirectional GRU layers run on PACKED sequences: an utterance's recurrence stops at
        * its own frame count and the rows behind it are zeros.  Three states of (B, T, hidden): the inputs of rnn_layers[1] and
        * rnn_layers[2] and the last layer's output.  compute_dtype S3ENC_F32 only; built by s3enc_create_apc. */
       S3ENC_APC = 7,
       /* Mockingjay / TERA / AudioALBERT (upstream/mockingjay/{expert,builder,model}.py): a spectrogram front end (the
        * OnlinePreprocessor log-mel or the kaldi fbank of upstream/baseline), Linear + sinusoid position table + LayerNorm, then
        * post-LN BERT layers (optionally one layer's weights run encoder_layers times), inputs over `sequence_length` frames
        * forwarded in chunks.  encoder_layers + 1 states of (B, T, embed_dim).  compute_dtype S3ENC_F32 only; built by
        * s3enc_create_mockingjay. */
       S3ENC_MOCKINGJAY = 8,
       /* DeCoAR / DeCoAR-layers (upstream/decoar/{decoar,audio,expert}.py, upstream/decoar_layers/): a kaldi log-mel front end
        * (hamming window, no deltas, CMVN over time), Linear 80 -> hidden, then a forward and a backward stack of unidirectional
        * nn.LSTM layers on PACKED sequences, their outputs concatenated.  One state of (B, T, 2 hidden) — the last layer — or one per
        * layer.  compute_dtype S3ENC_F32 only; built by s3enc_create_decoar. */
       S3ENC_DECOAR = 9,
       /* NPC (upstream/npc/{npc,audio,expert}.py): APC's kaldi log-mel front end (hamming window, CMVN over time), then n_blocks
        * ConvBlocks (Conv1d k = 3 -> BatchNorm -> act -> Conv1d k = 1 -> BatchNorm -> + input -> act) each followed by a masked
        * Conv1d (kernel_size taps with a hole of mask_size + 2 (i + 1) in the middle) -> tanh, summed over the blocks.  No length
        * masking anywhere: 2 n_blocks + 1 states of (B, T, hidden) (n_blocks + 2 with disable_cross_layer) whose rows behind an
        * utterance's own frames are the reference's values, not zeros.  compute_dtype S3ENC_F32 only; built by s3enc_create_npc. */
       S3ENC_NPC = 10,
       /* VGGish (upstream/vggish/{audio,vggish,expert}.py): a log-mel front end without padding (periodic Hann window, |rfft|, HTK
        * mel, log(. + offset)) cut into examples of example_frames frames, a stack of 3 x 3 Conv2d + ReLU (+ 2 x 2 max-pool) layers
        * over every example, three Linear + ReLU layers and — with postprocess — the PCA / clamp / 8-bit quantiser.  One state of
        * (B, E_max, fc[2]): an utterance's examples, exact zeros behind them (pad_sequence).  compute_dtype S3ENC_F32 only; built by
        * s3enc_create_vggish. */
       S3ENC_VGGISH = 11,
       /* BYOL-A (upstream/byol_a/{expert,byol_a}.py): every utterance zero-padded and cut into segments of `window` samples every
        * `stride` samples; per segment a centred 1024-point hann STFT (the segment reflect-padded about its own ends), |X|^2, 64 HTK
        * mel triangles, (log(. + FLT_EPSILON) - mean) / std; three Conv2d(3 x 3) + BatchNorm2d (eval) + ReLU + MaxPool2d(2, 2) (floor)
        * layers, Linear + ReLU + Linear + ReLU per pooled time step, max + mean over time.  One state of (B, S, feature_d), S =
        * ceil(n_max / stride).  NOTHING is masked: the rows behind an utterance's own segments are the network's response to the
        * zero padding, the reference's values and not zeros (NPC's convention).  compute_dtype S3ENC_F32 only; built by
        * s3enc_create_byol_a. */
       S3ENC_BYOL_A = 12,
       /* MAE-AST (upstream/mae_ast/{expert,mae_ast}.py; mae_ast_frame, mae_ast_patch): per utterance a kaldi log-mel front end at 128
        * bins (25 ms / 10 ms povey frames, pre-emphasis 0.97, snip_edges; F = 1 + (n - 400) / 160 frames), zero-padded to the batch's
        * F_max; BatchNorm2d(1, affine = False) on its running statistics times 0.5; nn.Unfold into kt x kc patches (token t * V + v, V =
        * 128 / kc, time the slow axis); Linear(kt * kc, D); the checkpoint's own sinusoidal position rows on the live tokens;
        * encoder_layers Transformer layers (encoder.layer_norm in front of post-LN layers; pre-LN layers when layer_norm_first) with
        * the padded tokens masked as keys.  encoder_layers states of (B, F_max / kt, V * D): the layer outputs, V tokens per row.  The
        * rows at or behind an utterance's valid count are the reference's values, not zeros: zero log-mel rows through the folded
        * Linear, no position row, queries over the utterance's live keys.  compute_dtype S3ENC_F32 only; built by
        * s3enc_create_mae_ast. */
       S3ENC_MAE_AST = 13,
       /* BYOL-S (upstream/byol_s/{expert.py,serab_byols/{serab,utils}.py,byol_a/models/{resnetish,audio_ntt}.py}; byol_s_default,
        * byol_s_resnetish34): the batch zero-padded to n_max, every row padded with window / 2 zeros in front and window - window / 2
        * behind and cut into windows of `window` samples every `step` samples (HEAR's centred frames), S = n_max / step + 1; per
        * window BYOL-A's front end with win_length = 400 (a periodic hann(400) centred in the 1024-point frame), log(mel +
        * FLT_EPSILON); the statistics of ALL B * S windows of the batch, mean = x.mean() / (B S) and std = x.std() / (B S) (unbiased; both
        * divided by the number of windows, the reference's own arithmetic); (x - mean) / std; then either AudioNTT2020 (`default`:
        * BYOL-A's network) or a ResNet of BasicBlocks (`resnetish`: a 7 x 7 stem + BatchNorm + ReLU + MaxPool2d(3, 2, 1), four
        * layers of blocks at 64 / 128 / 256 / 512 channels, the first block of layers 2-4 at stride 2 with a 1 x 1 shortcut), and
        * mean + max over time.  One state of (B, S, 2048).  NOTHING is masked and a row depends on the WHOLE batch through the two
        * statistics, its zero padding included; the rows behind an utterance's own len / step + 1 windows are the reference's
        * values, not zeros.  BatchNorm runs on its running statistics.  compute_dtype S3ENC_F32 only; built by s3enc_create_byol_s. */
       S3ENC_BYOL_S = 14,
       /* LightHuBERT (upstream/lighthubert/expert.py and its lighthubert/ package; lighthubert_small, lighthubert_base,
        * lighthubert_stage1): a HuBERT-base post-LN encoder cut out of a 768-wide supernet by leading rows and columns.  The binder
        * passes the SLICED tensors under HuBERT's checkpoint names (embed_dim 640 / 384 / 768) through s3enc_create /
        * s3enc_create_ex, except the positional conv: the reference resolves the weight-norm over the UNSLICED weight_v (768, 48, K)
        * and slices afterwards, so the binder folds it and passes "encoder.pos_conv.0.weight" (D, D / 16, K) in place of weight_g /
        * weight_v (s3prl_amd/ckpt.py: lighthubert_slice); fc1 / fc2 are cut per block of 768 rows / columns (SLinear's splits), every
        * other tensor by leading rows and columns.  HuBERT's frame mask; the waveform is always normalised (normalize = 1).  What differs is the state
        * list: encoder_layers + 1 states whose element 0 is the post_extract_proj output with its padded frames exactly zero (the
        * reference's in-place index_put aliases it), followed by the encoder_layers layer OUTPUTS; the layer-0 input (behind the
        * positional conv and encoder.layer_norm), HuBERT's element 0, is not a state.  One selection (S3ENC_SEL_HIDDEN).
        * compute_dtype S3ENC_F32 only, layer_norm_first = 0, pos_conv_depth <= 1 (s3enc_create refuses the rest by name). */
       S3ENC_LIGHTHUBERT = 15,
       /* DeCoAR 2.0 (upstream/decoar2/{audio,decoar2,expert}.py; decoar2, decoar2_custom, decoar2_local, decoar2_url): HuBERT-base's
        * post-LN encoder behind DeCoAR's kaldi front end instead of a conv extractor.  Through s3enc_create / s3enc_create_ex, no second
        * block: s3enc_config carries the frame geometry as a one-layer "conv stack", n_conv = 1, conv_kernel[0] / conv_stride[0] = 400 /
        * 160, conv_dim = 80 mel bins (the family's constants: every other value is refused), extractor_layer_norm = 0, conv_bias = 0,
        * normalize = 0.  Front end: torchaudio.compliance.kaldi.fbank(80 bins, hamming) at 16 kHz -> CMVN over the utterance's own F
        * frames (unbiased std, eps 1e-10 added to it) -> every second frame: T = ceil(F / 2), F = 1 + (n - 400) / 160; one batch-wide
        * pass (fbank.hip: launch_fbank_batch).  post_extract_proj Linear(80, embed_dim) reads every second row and zeroes rows at and
        * after T_b; from there HuBERT's path: positional conv, encoder.layer_norm, the layers with key padding.  The front end and the
        * projection are exact fp32 in every compute_dtype.  encoder_layers + 1 states for S3ENC_SEL_HIDDEN — the layer inputs, then the
        * encoder output; the other selections are refused (the expert has one list).  Padded rows: HuBERT's rule, the reference's values.
        * s3enc_num_frames / s3enc_valid_frames are ceil(F / 2), s3enc_downsample_rate 320.  Checkpoint tensors: post_extract_proj.{weight
        * (embed_dim, 80), bias}, encoder.pos_conv.0.{weight_g,weight_v,bias}, encoder.layer_norm.*, encoder.layers.N.*.  Refused by name:
        * layer_norm_first, pos_conv_depth > 1, the Conformer / WavLM / DistilHuBERT options, and by the forward an utterance with F < 2
        * (the reference's std over one frame is NaN). */
       S3ENC_DECOAR2 = 16,
       /* SSAST (upstream/ssast/{expert,ast_models,audio}.py; ssast_frame_base, ssast_patch_base): every utterance zero-padded to nseg =
        * ceil(n_max / window_samples) windows of window_samples samples; per window a kaldi log-mel front end at 128 bins with a hanning
        * window (25 ms / 10 ms, pre-emphasis 0.97, snip_edges), (y + 4.2677393) / (4.5689974 * 2), zero rows up to target_length; a
        * Conv2d(1, D, (fshape, tshape), stride (fstride, tstride)) patch embedding on the (128, target_length) image, f_dim x t_dim
        * tokens behind a cls and a dist token, the checkpoint's position rows (cut or interpolated at load); encoder_layers pre-LN timm
        * blocks (one fused attn.qkv Linear, LayerNorm eps from the block, erf-GELU) with no key mask.  encoder_layers states of (B,
        * T_out, f_dim * D), T_out = min(nseg * t_dim, ceil(n_max / (160 * tstride))): the layer outputs without the two prefix tokens,
        * row s * t_dim + ti the f_dim tokens of time step ti of window s.  Nothing is masked: rows behind an utterance's own length
        * are the reference's values (zero samples through the whole model), not zeros.  compute_dtype S3ENC_F32 only; built by
        * s3enc_create_ssast.  (17 is not assigned: the suite keeps it as its probe of an unknown family id.) */
       S3ENC_SSAST = 18 };
/* arithmetic type of the GEMM / attention operands; accumulation, norms, softmax, GELU and the residual
 * stream are always fp32 (the reference's Fp32GroupNorm / Fp32LayerNorm / fp32 softmax guards,
 * wav2vec2_model.py:1826-1853,1899-1900). */
enum { S3ENC_F32 = 0, S3ENC_BF16 = 1, S3ENC_F16 = 2,
       /* fp32 data flow (activations, norms, softmax, attention, positional conv exactly as S3ENC_F32) with the GEMMs
        * computed as three bf16 MFMAs per product on split operands (x = hi + lo): ~1e-5 relative error per GEMM at
        * 3/16 of the exact-fp32 matrix cost.  Opt-in; S3ENC_F32 stays the exact default. */
       S3ENC_F32X3 = 3,
       /* fp16 data flow (exactly S3ENC_F16: fp16 activations / attention, fp32 accumulate, norms, softmax, residual) with
        * every GEMM weight kept as TWO terms (w = hi + lo) and the contraction run over both: the weights' rounding error
        * disappears, leaving the activations'.  What a binder gets BY DEFAULT:
        *   - hi = fp16(w); lo = a second fp16 term — or, for q|k|v, fc1 and fc2 where the weight's shape pays for it, an MX-fp4
        *     image of lo (per row and 32 k an E8M0 scale + 32 e2m1 values, packed at s3enc_create) multiplied on the scaled-MFMA
        *     pipe in the same K step: 4.8e-5 of weight error per GEMM instead of 5e-7.  Tuning key "gemm16_mx" (read at
        *     s3enc_create, default 14; 0 = two fp16 terms everywhere) selects the GEMMs;
        *   - where a rounded fp16 OPERAND carries the error budget the GEMM reads fp32 activations through the three-term
        *     kernel instead: conv2.. of EVERY extractor (GroupNorm and layer-norm: conv1 writes fp32), post_extract_proj (the
        *     fp32 LayerNorm(C) output) and out_proj (the attention kernel writes fp32).  "fp16x2_conv1_f32" = 1 adds conv1.
        * Measured on outputs of the reference itself (profiles/r06_parity_seeds.md, 39 full-dimension fixtures on
        * released-checkpoint-like weight statistics, weight seeds 0-6 x five models): max relative error of a hidden state
        * 2.5e-4 ... 8.6e-4, median 5.3e-4 (8.0e-4 worst with conv1 on fp32 rows) — inside the path's 1e-3 on every seed, where
        * S3ENC_F16 is 0.9e-3 ... 2.8e-3 and S3ENC_BF16 0.7e-2 ... 1.5e-2 — at 3.1x the S3ENC_F32 throughput on HuBERT-base.
        * Its stated limit: an FFN whose hidden activation leaves the fp16 range (GELU(fc1) > 65504: fc1 scaled x1000+ on the
        * pretrained-like models, profiles/r05_fp16_cliff.md) returns non-finite states — reported by s3enc_forward_status; with
        * fc1 x10 ... x1000 WavLM-large settles at 1.2-1.4e-3.  Opt-in. */
       S3ENC_F16X2 = 4 };

/* Hyper-parameters that select kernel variants.
 * Replaces: HubertConfig / HubertPretrainingConfig (upstream/hubert/hubert_model.py:33-278),
 *           Wav2Vec2Config / AudioPretrainingConfig (upstream/wav2vec2/wav2vec2_model.py:2103-2350,3325-3345),
 *           WavLMConfig (upstream/wavlm/WavLM.py:162-245). */
typedef struct s3enc_config {
    int32_t family;                        /* S3ENC_HUBERT / WAV2VEC2 / WAVLM: selects the frame-mask rule */
    int32_t n_conv;                        /* number of conv feature layers (7) */
    int32_t conv_dim;                      /* channels of every conv layer (512) */
    int32_t conv_kernel[S3ENC_MAX_CONV];   /* (10,3,3,3,3,2,2) */
    int32_t conv_stride[S3ENC_MAX_CONV];   /* (5,2,2,2,2,2,2) */
    int32_t extractor_layer_norm;          /* 0: "default" (GroupNorm after conv0); 1: "layer_norm" */
    int32_t conv_bias;
    int32_t encoder_layers;
    int32_t embed_dim;
    int32_t ffn_dim;
    int32_t heads;
    int32_t layer_norm_first;              /* 0: post-LN (base); 1: pre-LN (large) */
    int32_t conv_pos;                      /* positional conv kernel (128): 1..256 */
    int32_t conv_pos_groups;               /* (16): embed_dim / conv_pos_groups, the group width, must be 24, 32, 40, 48 or 64 (24 and 40: S3ENC_F32
                                            * only, the 16-bit and split-precision positional conv is not built at those widths) — for every
                                            * layer_type (a Conformer handle packs the positional conv of its checkpoint too);
                                            * EncoderConfig.validate refuses the same */
    int32_t normalize;                     /* per-utterance waveform layer-norm (task_cfg.normalize) */
    int32_t rel_pos;                       /* WavLM: relative_position_embedding */
    int32_t num_buckets;
    int32_t max_distance;
    int32_t gru_rel_pos;
    int32_t compute_dtype;                 /* S3ENC_F32 / BF16 / F16 / F32X3 / F16X2 */
    int32_t no_feature_layer_norm;         /* 1: post_extract_proj reads the conv output directly (distiller/model.py:170-176) */
    int32_t pos_conv_depth;                /* data2vec: > 1 = that many {Conv1d(D, D, max(3, conv_pos / depth), groups) -> LayerNorm(no
                                            * affine) -> GELU} blocks instead of the single weight-normed conv (wav2vec2_model.py:2995-3023);
                                            * 0 / 1 = the standard positional conv */
    float wav_norm_eps;                    /* eps of the waveform normalisation; 0 = 1e-5 (F.layer_norm, hubert/expert.py:57-58);
                                            * Hugging Face's Wav2Vec2FeatureExtractor uses 1e-7 (upstream/hf_hubert/expert.py:30-37) */
    int32_t pred_heads;                    /* DistilHuBERT: N prediction heads Linear(D, N*D) -> GELU -> SplitLinear(D, N, D)
                                            * (distiller/model.py:155-161, module.py:55-90); 0 otherwise */
    /* S3ENC_MULTIRES only (MultiresHubertConfig, multires_hubert/hubert_model.py:97-148); encoder_layers = sum(mr_layers) */
    int32_t mr_pairs;                               /* rate pairs = resolutions - 1 (label_rate_ratios has 2 * mr_pairs entries) */
    int32_t mr_ratios[2 * (S3ENC_MAX_RES - 1)];     /* label_rate_ratios: up_0, down_0, up_1, down_1, ... */
    int32_t mr_layers[2 * S3ENC_MAX_RES - 1];       /* layers per block in execution order: encoders..., middle, decoders... */
    int32_t mr_kernel;                              /* conv_adapator_kernal (7): odd, every rate divides mr_kernel - 1 */
    int32_t mr_plain;                               /* use_plain_updownsample: ConvDownsampler / ConvUpsampler, else ConvAdapter */
    /* ABI 8: wav2vec 2.0 Conformer encoders (ConformerEncoder / ConformerEncoderLayer, wav2vec2_model.py:440-578,3132-3211),
     * family S3ENC_WAV2VEC2 only, compute_dtype S3ENC_F32 only (s3enc_create refuses the other modes by name).  Per layer:
     *   x += 0.5 * FFN1(x);  x += MHA(LN(x));  x += Conv(x);  x += 0.5 * FFN2(x);  x = LN_final(x)
     * FFN(x) = w_2 . swish(w_1 . LN(x) + b_1) + b_2;  Conv(x) = PW2 . swish(BN(DW(GLU(PW1 . LN(x)))));  no positional conv (its
     * checkpoint weights are accepted and ignored).  Checkpoint tensors per layer "encoder.layers.N." + the reference state_dict
     * names: ffn1.layer_norm.{weight,bias}, ffn1.w_1.{weight,bias}, ffn1.w_2.{weight,bias}, self_attn_layer_norm.{weight,bias},
     * self_attn.linear_{q,k,v,out}.{weight,bias}, [rel_pos: self_attn.linear_pos.weight, self_attn.pos_bias_u, self_attn.pos_bias_v
     * (H, 64)], conv_module.layer_norm.{weight,bias}, conv_module.pointwise_conv1.weight (2D, D, 1),
     * conv_module.depthwise_conv.weight (D, 1, dw_kernel), conv_module.batch_norm.{weight,bias,running_mean,running_var},
     * conv_module.pointwise_conv2.weight (D, D, 1), ffn2.* as ffn1, final_layer_norm.{weight,bias}; plus encoder.layer_norm.
     * Measured (Conformer-large, 32 x 10 s, one MI355X): 157.8 ms per batch with rope, 162.1 ms with rel_pos. */
    int32_t layer_type;                             /* 0 transformer, 1 conformer */
    int32_t pos_enc_type;                           /* conformer: 1 rel_pos (Transformer-XL relative attention), 2 rope */
    int32_t dw_kernel;                              /* conformer: depthwise_conv_kernel_size (odd, <= 63; 31) */
} s3enc_config;

/* S3ENC_WAV2VEC only (Wav2VecConfig, upstream/wav2vec/wav2vec_model.py:289-410): the second configuration block of
 * s3enc_create_ex.  s3enc_config and S3ENC_VERSION stay what ABI 8 binders were built against: the extractor is its n_conv / conv_dim /
 * conv_kernel / conv_stride (conv0: kernel 10); encoder_layers = n_agg and embed_dim = conv_dim; its Transformer fields
 * are ignored.  Every block is Conv1d -> Fp32GroupNorm(1, C) over all C x L values of the utterance, the zero-padded time
 * included -> ReLU (:235-286, :59-114).  Checkpoint tensors, reference state_dict names: feature_extractor.conv_layers.N.0.weight,
 * .N.2.{weight,bias}; feature_aggregator.conv_layers.N.1.{weight,bias}, .N.3.{weight,bias}; gumbel: vector_quantizer.vars (1, Gt * V, Dv),
 * vector_quantizer.weight_proj.{weight,bias} (vq_depth 1) or .weight_proj.I.0.{weight,bias} and .weight_proj.<depth-1>.{weight,bias};
 * k-means: vector_quantizer.embedding (V, Gt, Dv), .projection.0.weight (C, C / G, 1), .projection.1.{weight,bias}; Gt = 1 with
 * combine_groups, else G; wav2vec_predictions.* and project_features.* are not read.  s3enc_create_ex refuses by name what is not
 * built: every compute dtype but fp32, the GRU aggregator, activation gelu, skip_connections_feat, layers of unequal width
 * (residual_proj), aggregator strides other than 1, vq_dim != conv_dim. */
typedef struct s3enc_wav2vec_config {
    int32_t n_agg;                                  /* aggregator layers (12) */
    int32_t agg_dim[S3ENC_MAX_CONV];                /* their widths: all equal to conv_dim */
    int32_t agg_kernel[S3ENC_MAX_CONV];             /* (2..13); each layer pads kernel - 1 frames on the left */
    int32_t agg_stride[S3ENC_MAX_CONV];             /* all 1 */
    int32_t w2v_aggregator;                         /* 0 "cnn", 1 "gru" (refused) */
    int32_t w2v_activation;                         /* 0 "relu", 1 "gelu" (refused) */
    int32_t w2v_skip_feat;                          /* skip_connections_feat (refused) */
    int32_t log_compression;                        /* log(|x| + 1) behind the extractor */
    int32_t skip_connections_agg;                   /* x = (block(x) + x) * sqrt(residual_scale) */
    float residual_scale;
    int32_t non_affine_group_norm;
    int32_t no_conv_bias;                           /* the aggregator's convolutions have no bias */
    int32_t agg_zero_pad;                           /* ZeroPad1d instead of ReplicationPad1d */
    int32_t vq_type;                                /* 0 none, 1 gumbel (wav2vec2_model.py:1591-1782, eval: argmax), 2 kmeans (:117-232) */
    int32_t vq_vars;                                /* V: variables per group (320) */
    int32_t vq_groups;                              /* G (2) */
    int32_t vq_dim;                                 /* width of the codewords: conv_dim */
    int32_t vq_depth;                               /* gumbel: Linear layers of weight_proj (inner width 2 C, ReLU between) */
    int32_t combine_groups;                         /* the groups share one set of variables */
} s3enc_wav2vec_config;

/* S3ENC_CPC only (cpc_default_config.py, cpc/model.py:62-104,146-191): the second configuration block of s3enc_create_cpc.
 * s3enc_config carries the extractor as for every family (n_conv, conv_dim, conv_kernel (10,8,4,4,4), conv_stride (5,4,2,2,2));
 * encoder_layers = 1 and embed_dim = conv_dim; its Transformer fields are ignored.  Every convolution has a bias and `conv_pad`
 * zero frames on both sides (L_out = floor((L_in + 2 pad - k) / stride) + 1) and is followed by ChannelNorm — per frame over the
 * C channels, (x - mean) * rsqrt(var + 1e-5) * weight + bias with the UNBIASED variance (divide by C - 1) — and ReLU.  The
 * recurrent network is torch's nn.LSTM (gates i, f, g, o) or nn.GRU (gates r, z, n; b_hn inside the product with r), batch_first,
 * zero initial state, run over the padded time axis.  Checkpoint tensors, reference state_dict names: gEncoder.convN.{weight,bias},
 * gEncoder.batchNormN.{weight,bias} (1, C, 1), gAR.baseNet.{weight_ih,weight_hh,bias_ih,bias_hh}_lN; every one of them is
 * required (the reference's load_state_dict(strict=False) would keep a random initialisation instead).  s3enc_create_cpc refuses
 * by name what is not built: every compute dtype but fp32, norm_mode other than layerNorm, arMode RNN / transformer / no_ar,
 * cpc_mode "reverse", samplingType "sequential" (keep_hidden: state carried between forwards), hiddenGar != hiddenEncoder,
 * widths that are not a multiple of 64 or above 512, more than 4 recurrent layers. */
typedef struct s3enc_cpc_config {
    int32_t conv_pad[S3ENC_MAX_CONV];               /* (3,2,1,1,1) */
    int32_t norm_mode;                              /* 0 layerNorm (ChannelNorm); 1 instanceNorm, 2 ID, 3 batchNorm (refused) */
    int32_t ar_mode;                                /* 0 LSTM, 1 GRU; 2 RNN, 3 transformer, 4 no_ar (refused) */
    int32_t ar_layers;                              /* nLevelsGRU: 1..4 */
    int32_t ar_hidden;                              /* hiddenGar: equal to conv_dim */
    int32_t reverse;                                /* cpc_mode == "reverse" (refused) */
    int32_t keep_hidden;                            /* samplingType == "sequential" (refused) */
} s3enc_cpc_config;

/* S3ENC_APC only (apc/apc.py:26-71, apc/audio.py:53-115): the second configuration block of s3enc_create_apc.  s3enc_config
 * carries the frame geometry as a one-layer "conv stack": n_conv = 1, conv_kernel[0] / conv_stride[0] = the analysis window / the
 * frame shift in samples (400 / 160; both multiples of 4), conv_dim = embed_dim = hidden, encoder_layers = 2 (three states).
 * Front end: torchaudio.compliance.kaldi.fbank(num_mel_bins, frame_length, frame_shift, window_type) at 16 kHz -> CMVN over time
 * (unbiased std, eps 1e-10 added to the std) when `cmvn`.  Model: num_layers nn.GRU(batch_first) layers on packed sequences,
 * layer i > 0 adding its own input to its output when `residual`.  Checkpoint tensors, reference state_dict names:
 * rnn_layers.N.{weight_ih,weight_hh,bias_ih,bias_hh}_l0, every one of them required; vq_layers.* and postnet.* (VQ-APC's
 * quantizer and the regression head) feed only the prediction the upstream discards: accepted and not uploaded.
 * s3enc_create_apc refuses by name: every compute dtype but fp32, num_layers below 3 (the reference's hooks index rnn_layers[2])
 * or above 4, hidden not a multiple of 64 or above 512, window / shift that are not multiples of 4 samples. */
typedef struct s3enc_apc_config {
    int32_t num_mel_bins;                           /* feat_dim: 80 */
    float frame_length_ms;                          /* 25 */
    float frame_shift_ms;                           /* 10 */
    int32_t window;                                 /* 0 povey, 1 hamming (the reference's WINDOW_TYPE) */
    int32_t cmvn;                                   /* apply_cmvn */
    int32_t hidden;                                 /* hidden_size */
    int32_t num_layers;                             /* 3 or 4 */
    int32_t residual;                               /* rnn_residual */
} s3enc_apc_config;

/* S3ENC_MOCKINGJAY only: the second configuration block of s3enc_create_mockingjay.  s3enc_config carries embed_dim (hidden_size),
 * ffn_dim (intermediate_size), heads, encoder_layers (num_hidden_layers) and the frame geometry as a one-layer "conv stack":
 * n_conv = 1, conv_stride[0] = 160, conv_kernel[0] = 0 for the mel front end (centred frames: T = 1 + n / 160) or the analysis
 * window (400) for the kaldi one; conv_dim = embed_dim.  Checkpoint tensors, reference state_dict names of `Transformer`:
 * input_representations.{spec_transform,LayerNorm}.{weight,bias}, encoder.layer.N.attention.self.{query,key,value}.{weight,bias},
 * encoder.layer.N.attention.output.{dense,LayerNorm}.{weight,bias}, encoder.layer.N.intermediate.dense.{weight,bias},
 * encoder.layer.N.output.{dense,LayerNorm}.{weight,bias}; with share_layer only N = 0 is read (and uploaded once).
 * Refused by name: every compute dtype but fp32, pre_layer_norm, hidden_act other than gelu, embed_dim / heads != 64,
 * input_dim not a multiple of 4. */
typedef struct s3enc_mockingjay_config {
    int32_t input_dim;        /* width of a feature row: n_mels, or num_mel_bins * (delta_order + 1) */
    float layer_norm_eps;     /* 1e-12: EVERY LayerNorm of the family */
    int32_t share_layer;      /* AudioALBERT: layer 0's weights run encoder_layers times */
    int32_t sequence_length;  /* task.sequence_length: 0 = never chunk; T > it: torch.chunk(x, ceil(T / it), dim = 1) */
    int32_t frontend;         /* 0 = kaldi (`fbank`), 1 = mel (OnlinePreprocessor, feat_type mel, log, delta 0) */
    int32_t n_mels;           /* mel */
    float target_level;       /* mel: -25 dB */
    int32_t cmvn;             /* mel */
    int32_t pre_layer_norm;   /* refused */
    int32_t hidden_act;       /* 0 gelu; anything else is refused */
    /* kaldi: what the `fbank` baseline's configuration block carries, at a sample rate of 16000 */
    int32_t fbank_num_mel_bins;
    float fbank_frame_length_ms;
    float fbank_frame_shift_ms;
    float fbank_preemphasis;
    int32_t fbank_delta_order;
    int32_t fbank_delta_win_length;
    int32_t fbank_use_cmvn;
    float fbank_cmvn_eps;
} s3enc_mockingjay_config;

/* S3ENC_DECOAR only (decoar/decoar.py:9-83, decoar/audio.py:41-97, decoar_layers/decoar.py): the second configuration block of
 * s3enc_create_decoar.  s3enc_config carries the frame geometry as a one-layer "conv stack": n_conv = 1, conv_kernel[0] /
 * conv_stride[0] = the analysis window / the frame shift in samples (400 / 160; both multiples of 4), conv_dim = embed_dim =
 * 2 hidden (the width of a state), encoder_layers = the number of states - 1 (0, or num_layers - 1 with per_layer_states).
 * Front end: torchaudio.compliance.kaldi.fbank(num_mel_bins, window_type = hamming) at 16 kHz -> CMVN over time (unbiased std, eps
 * 1e-10 added to the std), then every `subsample`-th frame: f fbank frames give ceil(f / subsample) model frames.  The reference's
 * decoar / decoar_layers front end keeps every frame (subsample 1); 2 is the front end of DeCoAR 2.0 (decoar2/audio.py:84; served
 * by S3ENC_DECOAR2 on the batch-wide pass) and costs nothing here: the projection reads its rows at twice the stride.  Model: post_extract_proj (Linear), then per layer and
 * direction an nn.LSTM layer on packed sequences — the backward stack on every utterance's own rows in reverse — and the two
 * outputs side by side.  Checkpoint tensors, reference state_dict names: post_extract_proj.{weight,bias},
 * {forward,backward}_lstm.{weight_ih,weight_hh,bias_ih,bias_hh}_lN, every one of them required.  Refused by name: every compute
 * dtype but fp32, num_layers outside 1..4, hidden not a multiple of 64 or above 1024, subsample other than 1 or 2, window / shift
 * that are not multiples of 4 samples. */
typedef struct s3enc_decoar_config {
    int32_t num_mel_bins;                           /* 80 */
    int32_t hidden;                                 /* 1024 */
    int32_t num_layers;                             /* 4 */
    float frame_length_ms;                          /* 25 */
    float frame_shift_ms;                           /* 10 */
    int32_t subsample;                              /* 1 (decoar, decoar_layers) or 2 */
    int32_t per_layer_states;                       /* 0: one state, the last layer (decoar); 1: one per layer (decoar_layers) */
} s3enc_decoar_config;

/* S3ENC_NPC only (npc/npc.py:21-248, npc/audio.py:53-115, npc/expert.py:18-53): the second configuration block of
 * s3enc_create_npc.  s3enc_config carries the frame geometry as APC does: n_conv = 1, conv_kernel[0] / conv_stride[0] = the
 * analysis window / the frame shift in samples (400 / 160; both multiples of 4), conv_dim = embed_dim = hidden, encoder_layers =
 * the number of states - 1 (2 n_blocks, or n_blocks + 1 with disable_cross_layer).  Front end: APC's (s3enc_apc_config).
 * Model, eval mode: block i is x' = act(BN2(Conv1d_1(act(BN1(Conv1d_3(x))))) [+ x when residual and i > 0]) with BatchNorm on its
 * running statistics (eps 1e-5) when `batch_norm`, folded into the convolutions at load; masked conv i is
 * tanh(Conv1d(hidden, hidden, kernel_size, padding = (kernel_size - 1) / 2)) with taps [head, head + m_i) zeroed, m_i = mask_size
 * + 2 (i + 1), head = (kernel_size - m_i) / 2 — those taps are never read; the running sum of the masked outputs is the last
 * state.  With disable_cross_layer only the last block has a masked conv.  States in the reference's hook order: blocks[0],
 * masked_convs[0], blocks[1], masked_convs[1], ..., the sum (disable_cross_layer: the blocks, the last masked conv, and that
 * tensor again).  Checkpoint tensors, reference state_dict names: blocks.N.{conv,linear}.{weight,bias},
 * blocks.N.{bn1,bn2}.{weight,bias,running_mean,running_var} (batch_norm), masked_convs.N.conv.{weight,bias}, every one required;
 * masked_convs.N.conv_mask is optional and, when given, must equal the mask computed from this block; vq_layers.* and postnet.*
 * feed only the prediction the upstream discards: accepted and not uploaded.  s3enc_create_npc refuses by name: every compute
 * dtype but fp32, even kernel_size or mask_size, a mask that leaves no tap in some block, n_blocks outside 1..8, hidden not a
 * multiple of 64 or above 1024, num_mel_bins not a multiple of 16, activate other than 0 / 1, window / shift that are not
 * multiples of 4 samples, dim_bottleneck (a last state of another width). */
typedef struct s3enc_npc_config {
    int32_t num_mel_bins;                           /* feat_dim: 80 */
    float frame_length_ms;                          /* 25 */
    float frame_shift_ms;                           /* 10 */
    int32_t window;                                 /* 0 povey, 1 hamming (the reference's WINDOW_TYPE) */
    int32_t cmvn;                                   /* apply_cmvn */
    int32_t hidden;                                 /* hidden_size: 512 */
    int32_t n_blocks;                               /* 4 */
    int32_t kernel_size;                            /* 15 */
    int32_t mask_size;                              /* 5 */
    int32_t residual;                               /* 1 */
    int32_t batch_norm;                             /* 1 */
    int32_t activate;                               /* 0 relu, 1 tanh */
    int32_t disable_cross_layer;                    /* 0 */
    int32_t dim_bottleneck;                         /* 0: none; the auto-encoder bottleneck gives the last state another width (refused) */
} s3enc_npc_config;

/* S3ENC_VGGISH only (vggish/audio.py:30-84,256-294, vggish/vggish.py:18-133, vggish/expert.py:16-40): the second configuration
 * block of s3enc_create_vggish.  s3enc_config carries the frame geometry as APC does: n_conv = 1, conv_kernel[0] / conv_stride[0]
 * = window / shift in samples (400 / 160; both multiples of 4), conv_dim = embed_dim = fc[2], encoder_layers = 0 (one state).
 * Front end, 16 kHz input: frames of `window` samples every `shift` samples with NO padding, F = 1 + (n - window) / shift; each
 * times the periodic Hann window; |rfft(., n_fft)|; the (n_fft / 2 + 1) x num_mel_bins HTK mel matrix (edges linear in mel = 1127
 * ln(1 + f / 700) between mel_min_hz and mel_max_hz, DC row zero); log(. + log_offset); examples of example_frames frames every
 * example_hop frames, incomplete tails dropped: E = 1 + (F - example_frames) / example_hop for F >= example_frames, else 0.
 * Model: n_layers times Conv2d(3 x 3, padding 1) + ReLU, layer i followed by MaxPool2d(2, 2) when pool_after[i]; the last map is
 * flattened in (frames, bands, channels) order; Linear + ReLU three times (widths fc[0..2]); with `postprocess`
 * q = rint((clamp(P (y - m), quant_min, quant_max) - quant_min) * (255 / (quant_max - quant_min))), rint half to even.
 * Checkpoint tensors, reference state_dict names: features.K.{weight,bias} with K the layer's index in the reference's
 * nn.Sequential (a conv + its ReLU count two, a pool one: 0, 3, 6, 8, 11, 13 at the released shape), embeddings.{0,2,4}.
 * {weight,bias}, and with postprocess pca_eigen_vectors (D, D) and pca_means (D) or (D, 1), D = fc[2].  s3enc_create_vggish
 * refuses by name: every compute dtype but fp32, n_layers outside 1..8, channels that are not a multiple of 16, example_frames or
 * num_mel_bins not divisible by 2^pools, example_hop other than example_frames, window / shift that are not multiples of 4
 * samples, an n_fft that is not the power of two at or above window, Linear widths that are not multiples of 4. */
#define S3ENC_VGGISH_MAX_LAYERS 8
typedef struct s3enc_vggish_config {
    int32_t num_mel_bins;                           /* 64 */
    int32_t window;                                 /* samples: 400 */
    int32_t shift;                                  /* samples: 160 */
    int32_t n_fft;                                  /* 512 */
    float mel_min_hz;                               /* 125 */
    float mel_max_hz;                               /* 7500 */
    float log_offset;                               /* 0.01 */
    int32_t example_frames;                         /* 96 */
    int32_t example_hop;                            /* 96: must equal example_frames */
    int32_t n_layers;                               /* 6 */
    int32_t channels[S3ENC_VGGISH_MAX_LAYERS];      /* 64, 128, 256, 256, 512, 512 */
    int32_t pool_after[S3ENC_VGGISH_MAX_LAYERS];    /* 1, 1, 0, 1, 0, 1 */
    int32_t fc[3];                                  /* 4096, 4096, 128 */
    int32_t postprocess;                            /* 1 */
    float quant_min;                                /* -2 */
    float quant_max;                                /* +2 */
} s3enc_vggish_config;

/* S3ENC_BYOL_A only (byol_a/expert.py:27-125, byol_a.py:36-137, config.yaml): the second configuration block of
 * s3enc_create_byol_a.  s3enc_config carries the segment geometry: n_conv = 1, conv_kernel[0] / conv_stride[0] = window / stride in
 * samples, conv_dim = embed_dim = feature_d, encoder_layers = 0 (one state).  The caller computes window = int(window_secs * 16000)
 * and stride = int(stride_secs * 16000) exactly as the reference does.  Segments: starts = range(0, n_max, stride); every utterance
 * zero-padded to starts[-1] + window; segment (b, s) = padded[b][starts[s] : starts[s] + window].  Front end per segment, fixed:
 * n_fft = win_length = 1024, hop 160, center = True with reflect padding about the segment's own ends, periodic hann, power 2,
 * 1 + window / 160 frames; 64 HTK mel triangles between 60 and 7800 Hz over linspace(0, 8000, 513), norm = None; (log(mel +
 * FLT_EPSILON) - norm_mean) / norm_std.  Checkpoint tensors, reference state_dict names after the prefix rule of byol_a.py:66-74:
 * features.{0,4,8}.{weight,bias} (Conv2d(., 64, 3)), features.{1,5,9}.{weight,bias,running_mean,running_var} (BatchNorm2d),
 * fc.0.{weight,bias} (feature_d, 512), fc.3.{weight,bias} (feature_d, feature_d).  s3enc_create_byol_a refuses by name: every
 * compute dtype but fp32, a window of at most 512 samples (the reflection is undefined), a window below 1120 samples (fewer than 8
 * frames: nothing survives three pools), a feature_d that is not a multiple of 4. */
typedef struct s3enc_byol_a_config {
    int32_t feature_d;                              /* 512 / 1024 / 2048 */
    int32_t window;                                 /* samples per segment: 16000 */
    int32_t stride;                                 /* samples between two segment starts: 16000 */
    float norm_mean;                                /* -5.4919195 */
    float norm_std;                                 /* 5.0389895 */
    float bn_eps;                                   /* 1e-5 */
} s3enc_byol_a_config;

/* S3ENC_MAE_AST only (mae_ast/expert.py:24-100, mae_ast.py:202-281,305-325,400-481,613-821): the second configuration block of
 * s3enc_create_mae_ast.  s3enc_config carries embed_dim = D, heads, ffn_dim, encoder_layers and layer_norm_first; its conv fields
 * are not read.  Patches: kernel = stride = (kt, kc) on both axes; Tt = F_max / kt time steps, V = 128 / kc tokens per step, Ttok =
 * Tt * V tokens; frames Tt * kt .. F_max are never read.  Key padding (forward_padding_mask): utterance b keeps kv_b =
 * min(ceil(F_b / kt) * V, Ttok) leading tokens as keys — a patch that is only partly real counts as real.  The eval BatchNorm is
 * folded into the Linear once, on the host, in float64: s = 0.5 / sqrt(bn_var + bn_eps), W' = s W, b' = b - s bn_mean rowsum(W); the
 * image stays raw log-mel and the rows behind an utterance's frames stay zeros.  Checkpoint tensors, reference state_dict names:
 * post_extract_proj.{weight,bias} (D, kt * kc); enc_sine_pos_embed.pe: the LEADING pos_rows rows of the file's table, (pos_rows, D) —
 * the table in the file is the reference's operand, it is not recomputed; encoder.layer_norm.{weight,bias} (read only without
 * layer_norm_first: with it the final LayerNorm reaches no returned state and is not computed); encoder.layers.N.self_attn.{q,k,v,
 * out}_proj.{weight,bias}, .self_attn_layer_norm, .fc1, .fc2, .final_layer_norm.  A batch with more than pos_rows tokens is refused
 * by message, with the count.  s3enc_create_mae_ast refuses by name: every compute dtype but fp32, feature_dim != 128 (the
 * reference's mask rule hard-codes 128), kc outside {16, 32, 64, 128}, kt outside 1..32, embed_dim / heads != 64. */
typedef struct s3enc_mae_ast_config {
    int32_t kt;                                     /* ast_kernel_size_time = ast_kernel_stride_time: 16 (patch), 2 (frame) */
    int32_t kc;                                     /* ast_kernel_size_chan = ast_kernel_stride_chan: 16 (patch), 128 (frame) */
    int32_t feature_dim;                            /* task.feature_dim: 128 */
    float bn_mean;                                  /* batch_norm.running_mean[0] */
    float bn_var;                                   /* batch_norm.running_var[0] */
    float bn_eps;                                   /* 1e-5 */
    int32_t pos_rows;                               /* rows of enc_sine_pos_embed.pe handed over: min(max_token_length, 8192) */
} s3enc_mae_ast_config;

/* S3ENC_SSAST only (ssast/expert.py:24-133, ast_models.py:263-393, audio.py:88-116): the second configuration block of
 * s3enc_create_ssast.  s3enc_config carries embed_dim = D, heads, ffn_dim and encoder_layers; layer_norm_first must be 1; its conv fields
 * are not read.  f_dim = (128 - fshape) / fstride + 1, t_dim = (target_length - tshape) / tstride + 1, 2 + f_dim * t_dim tokens per
 * window.  Inside the handle the patch tokens of a window are TIME-major (token 2 + ti * f_dim + fi; the reference's order is f-major):
 * with neither a mask nor a relative position the model is equivariant under the permutation, and every f_dim-row group of a sequence
 * is one state row.  Tensors, prepared by the binder from the released file's module.v.* (s3prl_amd/ckpt.py: ssast_hot_path):
 * patch.weight (D, tshape * fshape), the conv weight summed over its input channel and permuted to [n][t][f]; patch.bias (D); prefix
 * (2, D) = cls_token + pos_embed[0], dist_token + pos_embed[1]; pos (pos_rows, D), pos_rows = f_dim * t_dim, the position rows of the
 * patch tokens after the reference's cut / bilinear interpolation, in the time-major order; blocks.N.{norm1,attn.qkv,attn.proj,norm2,
 * mlp.fc1,mlp.fc2}.{weight,bias} as stored (attn.qkv rows q | k | v; the q rows are scaled by head_dim^-0.5 = 0.125 at create).  v.norm
 * reaches no returned state and is not read.  s3enc_create_ssast refuses by name: every compute dtype but fp32, layer_norm_first = 0,
 * embed_dim / heads != 64, a geometry patchstrided.hip does not take (fshape outside {16, 32, 64, 128}, tshape outside 1..32, an odd
 * fstride), window_samples < 400 or not a multiple of 4, target_length < tshape or below the window's own frame count, pos_rows !=
 * f_dim * t_dim. */
typedef struct s3enc_ssast_config {
    int32_t fshape;                                 /* patch extent in mel bins: 16 (patch), 128 (frame) */
    int32_t tshape;                                 /* patch extent in frames: 16 (patch), 2 (frame) */
    int32_t fstride;                                /* 10 (patch), 128 (frame) */
    int32_t tstride;                                /* 10 (patch), 1 (frame) */
    int32_t window_samples;                         /* int(window_secs * 16000) */
    int32_t target_length;                          /* int(window_secs * 16000 / 160): image rows per window */
    float ln_eps;                                   /* the blocks' LayerNorm eps: 1e-6 */
    int32_t pos_rows;                               /* f_dim * t_dim */
} s3enc_ssast_config;

/* S3ENC_BYOL_S only: the second configuration block of s3enc_create_byol_s.  s3enc_config carries the window geometry as n_conv = 1,
 * conv_kernel[0] / conv_stride[0] = window / step in samples, conv_dim = embed_dim = 2048, encoder_layers = 0 (one state).  The
 * caller computes window = int(window_secs * 1000 / 1000 * 16000) and step = int(hop_secs * 1000 / 1000.0 * 16000) with the
 * reference's own expressions (expert.py:22-23, serab.py:151-153, utils.py:79).  Checkpoint tensors, the reference's plain state_dict:
 * default: features.{0,4,8}.{weight,bias}, features.{1,5,9}.{weight,bias,running_mean,running_var}, fc.0 (2048, 512), fc.3 (2048,
 * 2048); resnetish: conv1.weight (64, 1, 7, 7), bn1.*, layerL.B.{conv1,conv2}.weight, layerL.B.{bn1,bn2}.*, and for the first block
 * of layers 2-4 layerL.0.downsample.0.weight (planes, inplanes, 1, 1) and layerL.0.downsample.1.*; no convolution has a bias.
 * s3enc_create_byol_s refuses by name: every compute dtype but fp32, the networks cvt and clstm, Bottleneck blocks, a block count
 * outside 1..64, a window of at most 512 samples (the reflection is undefined), for `default` a window below 1120 samples, a step
 * below one sample. */
enum { S3ENC_BYOL_S_DEFAULT = 0, S3ENC_BYOL_S_RESNETISH = 1, S3ENC_BYOL_S_CVT = 2, S3ENC_BYOL_S_CLSTM = 3 };
typedef struct s3enc_byol_s_config {
    int32_t network;                                /* S3ENC_BYOL_S_DEFAULT / _RESNETISH (the other two are refused by name) */
    int32_t blocks[4];                              /* resnetish: BasicBlocks per layer, 3 4 6 3 (resnetish34) */
    int32_t bottleneck;                             /* 1: Bottleneck blocks (resnetish50): refused by name */
    int32_t window;                                 /* samples per window: 16000 */
    int32_t step;                                   /* samples between two window starts: 800 */
    float bn_eps;                                   /* 1e-5 */
} s3enc_byol_s_config;

/* A named fp32 host tensor of the checkpoint, named exactly like the reference state_dict entry
 * ("encoder.layers.3.fc1.weight", ...).  Replaces model.load_state_dict(...)
 * (upstream/hubert/convert.py:37-56, wav2vec2/convert.py:26-39, wavlm/expert.py:37-40). */
typedef struct s3enc_tensor {
    const char* name;
    const float* data;  /* host, contiguous, row-major */
    int32_t ndim;
    int64_t shape[4];
} s3enc_tensor;

int s3enc_version(void);
const char* s3enc_last_error(void);

/* Build an encoder on GPU `device`: packs the weights (folds weight-norm, concatenates q/k/v, folds the
 * 1/sqrt(head_dim) query scale, re-lays conv weights tap-major, converts to the compute dtype) and uploads them.
 * Replaces UpstreamExpert.__init__ (hubert/expert.py:27-51, wav2vec2/expert.py:21-56, wavlm/expert.py:34-54). */
int s3enc_create(const s3enc_config* cfg, const s3enc_tensor* tensors, int32_t n_tensors, int32_t device,
                 s3enc_handle* out);
/* s3enc_create with the family's second configuration block: `w2v` is required for S3ENC_WAV2VEC (s3enc_create refuses that family:
 * it has no place for the aggregator / quantizer parameters) and must be NULL for every other family.
 * Replaces UpstreamExpert.__init__ of upstream/wav2vec/expert.py:16-34 (load_converted_model, wav2vec/convert.py:24-37). */
int s3enc_create_ex(const s3enc_config* cfg, const s3enc_wav2vec_config* w2v, const s3enc_tensor* tensors, int32_t n_tensors,
                    int32_t device, s3enc_handle* out);
/* The S3ENC_CPC family: s3enc_config beside its own block (s3enc_create and s3enc_create_ex refuse that family by name: they have no
 * place for the paddings and the recurrent network).  Replaces UpstreamExpert.__init__ of upstream/cpc/expert.py:26-42.  On the
 * handle: s3enc_num_frames / _num_output_frames count with the paddings (159 samples give one frame, fewer give 0 and the forward
 * refuses them), s3enc_valid_frames follows the wav2vec convention (the frames the utterance's own samples reach),
 * s3enc_num_states is 2 for S3ENC_SEL_HIDDEN (the other selections are refused), out_dtype must be S3ENC_F32. */
int s3enc_create_cpc(const s3enc_config* cfg, const s3enc_cpc_config* cpc, const s3enc_tensor* tensors, int32_t n_tensors,
                     int32_t device, s3enc_handle* out);
/* The S3ENC_APC family: s3enc_config beside its own block (s3enc_create, s3enc_create_ex and s3enc_create_cpc refuse that family
 * by name).  Replaces UpstreamExpert.__init__ of upstream/apc/expert.py:19-42.  On the handle: s3enc_num_frames counts whole
 * analysis windows (snip_edges: 400 samples give one frame, fewer give 0 and the forward refuses such an utterance),
 * s3enc_valid_frames is the utterance's own frame count, s3enc_num_states is 3 for S3ENC_SEL_HIDDEN (the other selections are
 * refused), out_dtype must be S3ENC_F32.  Every state row behind an utterance's frame count is exactly 0. */
int s3enc_create_apc(const s3enc_config* cfg, const s3enc_apc_config* apc, const s3enc_tensor* tensors, int32_t n_tensors,
                     int32_t device, s3enc_handle* out);
/* The S3ENC_MOCKINGJAY family: s3enc_config beside its own block (the other create entries refuse the family by name).  Replaces
 * PretrainedTransformer.__init__ / forward of upstream/mockingjay/builder.py.  On the handle: s3enc_num_frames is the STAND-ALONE
 * frame count (mel: 1 + n / 160); s3enc_valid_frames(length, n_max) is the utterance's frame count INSIDE a batch padded to n_max
 * — for the mel front end with CMVN round(length / (n_max / T)), which can be one less than the stand-alone count (8000 samples
 * beside 16000: 50, alone 51); without CMVN every row is live (T).  States: the input representation, then every layer's output.
 * Rows at or behind an utterance's frame count are padding: what the kernels compute there (the zero feature rows run through
 * the model, attention over the chunk's live keys, or over key 0 alone in a chunk without a live key) — finite, deterministic,
 * inside the buffer, and not the reference's values. */
int s3enc_create_mockingjay(const s3enc_config* cfg, const s3enc_mockingjay_config* mj, const s3enc_tensor* tensors, int32_t n_tensors,
                            int32_t device, s3enc_handle* out);
/* The S3ENC_DECOAR family: s3enc_config beside its own block (the other create entries refuse the family by name).  Replaces
 * UpstreamExpert.__init__ of upstream/decoar/expert.py and upstream/decoar_layers/expert.py (same checkpoint file and tensor names;
 * the latter only renames them).  On the handle: s3enc_num_frames is ceil(fbank frames / subsample); an utterance with fewer than
 * 2 fbank frames is refused by the forward (the reference's unbiased std over one frame is NaN); s3enc_downsample_rate is the
 * frame shift in samples, 160, what the reference's get_downsample_rates returns whatever `subsample` is; s3enc_num_states is 1 or
 * num_layers for S3ENC_SEL_HIDDEN (the other selections are refused), out_dtype must be S3ENC_F32, B <= 128.  Every state row
 * behind an utterance's frame count is exactly 0. */
int s3enc_create_decoar(const s3enc_config* cfg, const s3enc_decoar_config* decoar, const s3enc_tensor* tensors, int32_t n_tensors,
                        int32_t device, s3enc_handle* out);
/* The S3ENC_NPC family: s3enc_config beside its own block (the other create entries refuse the family by name).  Replaces
 * UpstreamExpert.__init__ of upstream/npc/expert.py.  On the handle: s3enc_num_frames is the fbank frame count; an utterance
 * shorter than one window is refused by the forward; s3enc_downsample_rate is the frame shift in samples, 160;
 * s3enc_num_states is encoder_layers + 1 for S3ENC_SEL_HIDDEN (the other selections are refused), out_dtype must be S3ENC_F32.
 * s3enc_valid_frames is the utterance's own frame count, BUT — the one place this family differs from APC — the rows behind it
 * are NOT zeros: the reference runs its convolutions over all T rows of the padded batch, bias and BatchNorm make the padded
 * rows loud from the first block on, and they reach the utterance's last valid frames.  Every row of every state is the
 * reference's value for this T; an utterance's rows depend on T and on nothing else of the batch. */
int s3enc_create_npc(const s3enc_config* cfg, const s3enc_npc_config* npc, const s3enc_tensor* tensors, int32_t n_tensors,
                     int32_t device, s3enc_handle* out);
/* The S3ENC_VGGISH family: s3enc_config beside its own block (the other create entries refuse the family by name).  Replaces
 * UpstreamExpert.__init__ of upstream/vggish/expert.py.  On the handle: s3enc_num_frames(n) is the number of examples E (0 below
 * window + (example_frames - 1) * shift samples = 15600, and the forward refuses such an utterance by index and length);
 * s3enc_valid_frames is the utterance's own E, the rows behind it are exact zeros (also in the quantised form);
 * s3enc_downsample_rate is 16000 (expert.py:21-22, although the examples are 15360 samples apart); s3enc_num_states is 1 for
 * S3ENC_SEL_HIDDEN (the other selections are refused), out_dtype must be S3ENC_F32. */
int s3enc_create_vggish(const s3enc_config* cfg, const s3enc_vggish_config* vggish, const s3enc_tensor* tensors, int32_t n_tensors,
                        int32_t device, s3enc_handle* out);
/* The S3ENC_BYOL_A family: s3enc_config beside its own block (the other create entries refuse the family by name).  Replaces
 * UpstreamExpert.__init__ of upstream/byol_a/expert.py.  On the handle: s3enc_num_frames(n) is the number of segments S =
 * ceil(n / stride); s3enc_valid_frames is the utterance's own S — the rows behind it are NOT zeros but the reference's values for
 * the zero-padded segments; s3enc_downsample_rate is stride; s3enc_num_states is 1 for S3ENC_SEL_HIDDEN (the other selections are
 * refused), out_dtype must be S3ENC_F32.  A row (b, s) depends on segment (b, s)'s own `window` samples and on nothing else. */
int s3enc_create_byol_a(const s3enc_config* cfg, const s3enc_byol_a_config* byol_a, const s3enc_tensor* tensors, int32_t n_tensors,
                        int32_t device, s3enc_handle* out);
/* The S3ENC_MAE_AST family: s3enc_config beside its own block (the other create entries refuse the family by name).  Replaces
 * UpstreamExpert.__init__ of upstream/mae_ast/expert.py.  On the handle: s3enc_num_frames(n) is F(n) / kt time steps, F(n) = 1 +
 * (n - 400) / 160; s3enc_valid_frames(length, n_max) is min(ceil(F(length) / kt), F(n_max) / kt); s3enc_downsample_rate is kt * 160;
 * s3enc_num_states is encoder_layers for S3ENC_SEL_HIDDEN (the layer outputs, not the embedding; the other selections are refused);
 * a state row is V * D wide (layer_stride counts B * F_max / kt * V * D elements); out_dtype must be S3ENC_F32; featurize is
 * elementwise over the same slab (feat_normalize is refused when V > 1: the reference would normalise rows of V * D).  Rows at or
 * behind an utterance's valid count are the reference's values (see S3ENC_MAE_AST): the attention kernel computes padded query
 * rows over the live keys, as for the Mockingjay family.  s3enc_forward refuses by message: an utterance under 400 samples (by index
 * and length), a batch with F_max < kt, a batch with more tokens than pos_rows (with the count).  Tuning key patch_embed_fused. */
int s3enc_create_mae_ast(const s3enc_config* cfg, const s3enc_mae_ast_config* mae_ast, const s3enc_tensor* tensors, int32_t n_tensors,
                         int32_t device, s3enc_handle* out);
/* The S3ENC_BYOL_S family: s3enc_config beside its own block (the other create entries refuse the family by name).  Replaces
 * UpstreamExpert.__init__ of upstream/byol_s/expert.py.  On the handle: s3enc_num_frames(n) is the number of windows S = n / step +
 * 1; s3enc_valid_frames is the utterance's own len / step + 1 — the rows behind it are NOT zeros but the reference's values;
 * s3enc_downsample_rate is step; s3enc_num_states is 1 for S3ENC_SEL_HIDDEN (the other selections are refused), out_dtype must be
 * S3ENC_F32.  A row depends on the whole batch (the two statistics): a batch must not be split.  Debug taps of the last forward:
 * "logmel" (B S, frames, 64) un-normalised, "stats" the two statistics {mean / (B S), std / (B S)}.  Tuning keys byol_s_chunk,
 * stem_fused, conv2d_n64. */
int s3enc_create_byol_s(const s3enc_config* cfg, const s3enc_byol_s_config* byol_s, const s3enc_tensor* tensors, int32_t n_tensors,
                        int32_t device, s3enc_handle* out);
/* The S3ENC_SSAST family: s3enc_config beside its own block (the other create entries refuse the family by name).  Replaces
 * UpstreamExpert.__init__ of upstream/ssast/expert.py.  On the handle: s3enc_num_frames(n) is T_out(n) = min(ceil(n / W) * t_dim,
 * ceil(n / (160 * tstride))), W = window_samples; s3enc_valid_frames(length, n_max) is min(ceil(length / (160 * tstride)), T_out(n_max)),
 * the wrapper's rule (the rows behind it are the reference's values, not zeros); s3enc_downsample_rate is 160 * tstride;
 * s3enc_num_states is encoder_layers for S3ENC_SEL_HIDDEN (the layer outputs; the other selections are refused); a state row is f_dim * D
 * wide (layer_stride counts B * T_out * f_dim * D elements); out_dtype must be S3ENC_F32; featurize is the elementwise weighted sum
 * (feat_normalize is refused).  There is no minimum length: a window wholly behind an utterance's end is embedded and encoded like any
 * other.  The forward status word is not fed by this family's LayerNorms.  Tuning keys patch_strided_fused, ssast_chunk. */
int s3enc_create_ssast(const s3enc_config* cfg, const s3enc_ssast_config* ssast, const s3enc_tensor* tensors, int32_t n_tensors,
                       int32_t device, s3enc_handle* out);
int s3enc_destroy(s3enc_handle h);

/* T = frames produced for an n-sample input: floor((L-k)/s)+1 through the conv stack
 * (wav2vec2_model.py:2610-2624).  get_downsample_rates() is the product of the strides (320). */
int s3enc_num_frames(s3enc_handle h, int64_t n_samples, int32_t* T);
/* T of the states the forward writes for a batch padded to n_samples: s3enc_num_frames, except for S3ENC_MULTIRES
 * where every state is cut to the common length of the upsampled blocks (multires_hubert/expert.py:93-101). */
int s3enc_num_output_frames(s3enc_handle h, int64_t n_samples, int32_t* T);
int s3enc_downsample_rate(s3enc_handle h, int32_t* rate);
/* Un-masked frames of an utterance of `length` samples in a batch padded to `n_max`:
 * HuBERT/WavLM forward_padding_mask (hubert_model.py:454-464, WavLM.py:339-349), wav2vec2 conv-length rule
 * (wav2vec2_model.py:2652-2669). */
int s3enc_valid_frames(s3enc_handle h, int64_t length, int64_t n_max, int32_t* valid);

/* The forward.  Replaces UpstreamExpert.forward + the hook capture of UpstreamBase.__call__
 * (hubert/expert.py:56-72, upstream/interfaces.py:100-131).
 *   wavs      host array of B device pointers, wavs[b] -> lengths[b] fp32 samples (borrowed, read-only)
 *   lengths   host array of B sample counts
 *   n_max     pad-to length; 0 = max(lengths).  A data-parallel shard passes the GLOBAL batch maximum.
 *   out       device fp32; hidden_states[l] is the contiguous (B, T, D) block at out + l*layer_stride,
 *             l = 0..encoder_layers (layer inputs, then the encoder output)
 *   layer_stride  in elements, >= B*T*D
 */
int s3enc_forward(s3enc_handle h, const float* const* wavs, const int64_t* lengths, int32_t B, int64_t n_max,
                  float* out, int64_t layer_stride, void* stream);

/* Which tensors of the forward are "the states", and how they leave the library.
 * Replaces: the hook selection of the experts (hubert/expert.py:36-43: layer inputs + encoder output), wav2vec2's
 * feature_selection (wav2vec2/expert.py:81-93: layer_results[i][0] / [i][2]), the DistilHuBERT list
 * (distiller/expert.py:43-52), and — with `featurize` — Featurizer._weighted_sum applied as the encoder's epilogue
 * (nn/upstream.py:312-328, upstream/interfaces.py:221-249). */
enum { S3ENC_SEL_HIDDEN = 0,     /* default list: encoder_layers+1 states (DistilHuBERT: 1 + layers + pred_heads) */
       S3ENC_SEL_LAYER_OUT = 1,  /* "fairseq_layers": every layer's output (encoder_layers states) */
       S3ENC_SEL_FFN_OUT = 2 };  /* "fairseq_layers_before_residual": every layer's fc2 output before the residual */
typedef struct s3enc_forward_opts {
    int32_t selection;       /* S3ENC_SEL_* */
    int32_t out_dtype;       /* S3ENC_F32, or the handle's own 16-bit compute dtype: states are then written as 16-bit
                              * values (half the slab bytes and half the data-parallel all-gather); ignored with featurize */
    int32_t featurize;       /* 1: write ONLY  out[b][t][:] = sum_i feat_w[i] * (feat_normalize ? layer_norm(state_i) : state_i)
                              * as one fp32 (B, T, D) block — the states themselves never leave the workspace */
    int32_t feat_normalize;  /* F.layer_norm(state, (D,)) (no affine, eps 1e-5) before the sum */
    const float* feat_w;     /* host, one weight per state of the selection (softmax already applied; 0 = unselected) */
} s3enc_forward_opts;
/* number of states of a selection (the leading extent of `out` when not featurizing) */
int s3enc_num_states(s3enc_handle h, int32_t selection, int32_t* n);
/* s3enc_forward with options; opts == NULL is s3enc_forward.  out: device; state i is the contiguous (B, T, D) block at
 * out + i*layer_stride ELEMENTS of out_dtype (featurize: one fp32 (B, T, D) block, layer_stride ignored). */
int s3enc_forward_ex(s3enc_handle h, const float* const* wavs, const int64_t* lengths, int32_t B, int64_t n_max,
                     const s3enc_forward_opts* opts, void* out, int64_t layer_stride, void* stream);

/* s3enc_forward_ex plus the quantizer's outputs of an S3ENC_WAV2VEC handle with vq_type != 0 (wav2vec family).  Replaces result["codewords"]
 * and result["codeids"] of wav2vec/expert.py:49-53 (vector_quantizer(features, produce_targets=True)): codewords: device fp32
 * (B, T, vq_dim), 16-byte aligned; codeids: device int64 (B, T, vq_groups), per (frame, group) the index of the chosen variable
 * (ties: the lowest index); either may be NULL.  Other handles: both must be NULL. */
int s3enc_forward_aux(s3enc_handle h, const float* const* wavs, const int64_t* lengths, int32_t B, int64_t n_max,
                      const s3enc_forward_opts* opts, void* out, int64_t layer_stride, float* codewords, int64_t* codeids,
                      void* stream);

/* Numerical health of the forwards of this handle (ABI 6).  Replaces: nothing the reference has as a call — its
 * experts return whatever ATen computed and the regression test inspects the tensors (test/test_upstream.py:118-136);
 * a 16-bit compute mode can overflow where fp32 cannot (fp16: |x| > 65504), so the library reports it instead of leaving
 * the caller to scan (NS, B, T, D) states.  `*status` = OR of S3ENC_STATUS_* over every FINISHED forward since the last
 * call; reading clears.  S3ENC_STATUS_NONFINITE: some row LayerNorm met a non-finite mean / variance — every hidden state
 * is a LayerNorm output (post-LN models) or the next LayerNorm's input (pre-LN residual streams), so an inf / NaN that
 * reaches the states is seen; the states of that forward must not be trusted.  wait != 0: block until every forward
 * enqueued so far has finished on its stream; wait == 0: never blocks — forwards still running are reported by the bit
 * S3ENC_STATUS_PENDING and their own bits by a later call (host-side cost of a poll: a few hipEventQuery; each forward
 * copies its word to a pinned ring of 8 slots, so nothing here touches the device). */
enum { S3ENC_STATUS_NONFINITE = 1, S3ENC_STATUS_PENDING = 1 << 30 };
int s3enc_forward_status(s3enc_handle h, int32_t wait, int32_t* status);

/* Optional: `n` = encoder_layers+1 hipEvent_t handles (as void*); the following forwards record events[l] on the
 * launch stream as soon as hidden_states[l] is final, so a communication stream can start the all-gather of layer l
 * while later layers are still computing.  n = 0 clears.  The events stay owned by the caller. */
int s3enc_set_layer_events(s3enc_handle h, void* const* events, int32_t n);

/* ---- multi-GPU: the exchange step of the data-parallel path ---------------------------------------
 * One rank per GPU (process or thread).  Rank r encodes its contiguous block of the batch padded to the GLOBAL n_max
 * (s3enc_forward's n_max argument — the only coupling between utterances) into a (states, shard, T, D) slab; the slabs are
 * re-assembled into (states, world * shard, T, D), rank order = input order, with one RCCL all-gather per state over xGMI.
 * Replaces: nothing in the reference's upstream path (run_downstream.py:166-168 only wraps trainable upstreams in DDP);
 * it is what torch.distributed.all_gather_into_tensor does for the Python binding (s3prl_amd/parallel.py).
 *   s3enc_comm_unique_id   rank 0 draws the 128-byte RCCL id and hands it to the other ranks by any side channel
 *   s3enc_comm_init_rank   collective over all ranks; `device` = the rank's GPU.  world = 1 is valid (gathers are copies).
 *   s3enc_comm_allgather_states
 *       send / recv: device; state l is `bytes_per_state` bytes at send + l * send_state_stride, and lands as rank r's block
 *       at recv + l * recv_state_stride + r * bytes_per_state (strides in BYTES; recv_state_stride >= world * bytes_per_state).
 *       ready_events: NULL, or n_states hipEvent_t (as void*) — the events given to s3enc_set_layer_events: the gather of
 *       state l then starts as soon as the encoder has recorded event l, on the communicator's own stream, while the
 *       remaining layers still compute.  On return the gathers are enqueued and `stream` is ordered after the last of them. */
typedef struct s3enc_comm_s* s3enc_comm;
int s3enc_comm_version(int32_t* version); /* RCCL's version code; fails (with the reason) when librccl cannot be loaded */
int s3enc_comm_unique_id(void* id128);
int s3enc_comm_init_rank(const void* id128, int32_t world, int32_t rank, int32_t device, s3enc_comm* out);
int s3enc_comm_info(s3enc_comm c, int32_t* world, int32_t* rank);
int s3enc_comm_allgather_states(s3enc_comm c, const void* send, int64_t send_state_stride, void* recv, int64_t recv_state_stride,
                                int32_t n_states, int64_t bytes_per_state, void* const* ready_events, void* stream);
/* The same exchange with the algorithm chosen by the caller (ABI 5):
 *   S3ENC_EXCHANGE_COLLECTIVE  one ncclAllGather per state — what s3enc_comm_allgather_states issues; RCCL picks ring / direct;
 *   S3ENC_EXCHANGE_DIRECT      per state one group of world-1 ncclSend / ncclRecv pairs (peer = rank +- p): xGMI is
 *                              point-to-point, every pair of GPUs has its own link, all 7 are driven at once.
 * Identical result bytes; replaces nothing in the reference (see above).  With world = 1 both are one device copy. */
#define S3ENC_EXCHANGE_COLLECTIVE 0
#define S3ENC_EXCHANGE_DIRECT 1
/* S3ENC_EXCHANGE_COPY (ABI 7): the same bytes in the same places moved by the COPY ENGINES — no RCCL kernel, no compute unit beside
 * the encoder's GEMMs.  Every rank registers ONE receive slab (s3enc_comm_copy_export: the `recv` of every later exchange), the ranks
 * swap the S3ENC_COPY_HANDLE_BYTES blobs by any side channel (hipIpcGetMemHandle inside: one PROCESS per GPU) and map each other's slab
 * and mailbox (s3enc_comm_copy_attach).  Per exchange and peer: one hipMemcpyAsync per state into the peer's slab, on that peer's own
 * stream (all xGMI links at once) and behind the encoder's "state l final" event; two 64-bit sequence numbers per pair order the
 * exchange (ready-to-receive, data-has-landed; csrc/comm.hip).  The waits are one-wave polls with a deadline (S3ENC_COPY_DEADLINE_MS,
 * default 5000): s3enc_comm_copy_status reports a missed one instead of a hung GPU.  A communicator for this form alone needs no RCCL:
 * s3enc_comm_init_local. */
#define S3ENC_EXCHANGE_COPY 2
#define S3ENC_COPY_HANDLE_BYTES 256
int s3enc_comm_init_local(int32_t world, int32_t rank, int32_t device, s3enc_comm* out);
int s3enc_comm_copy_export(s3enc_comm c, void* recv_slab, int64_t bytes, void* handle_out);
int s3enc_comm_copy_attach(s3enc_comm c, const void* handles /* world x S3ENC_COPY_HANDLE_BYTES, in rank order */);
int s3enc_comm_copy_status(s3enc_comm c, int32_t* status);
/* optional: marks, on `stream`, the point behind which nobody reads the slab's current contents any more — call it before enqueueing
 * the next forward, and that forward's per-state pushes overlap it (without it the next exchange counts from its own call) */
int s3enc_comm_copy_release(s3enc_comm c, void* stream);
int s3enc_comm_exchange_states(s3enc_comm c, int32_t algo, const void* send, int64_t send_state_stride, void* recv,
                               int64_t recv_state_stride, int32_t n_states, int64_t bytes_per_state, void* const* ready_events,
                               void* stream);
int s3enc_comm_destroy(s3enc_comm c);

/* Same, for a zero-padded (B, row_stride) device buffer (what pad_sequence builds, hubert/expert.py:66). */
int s3enc_forward_padded(s3enc_handle h, const float* pcm, int64_t row_stride, const int64_t* lengths, int32_t B,
                         int64_t n_max, float* out, int64_t layer_stride, void* stream);

/* ---- measurement ------------------------------------------------------------------------------------
 * With profiling on, the kernel launches of the next forwards are bracketed by HIP events on the launch stream
 * (on = 1: every kernel; on = 2: only the GEMM launches — two events cost ~2.6 us, which for ~290 launches per forward
 * is 2 % of an fp32 and 10 % of a bf16 batch, so a TIMED region profiles only its dominant kernel);
 * s3enc_profile_read synchronises and returns per-kernel-kind totals. */
int s3enc_profile_enable(s3enc_handle h, int32_t on);
int s3enc_profile_reset(s3enc_handle h);
typedef struct s3enc_profile_entry {
    char name[48];
    int64_t launches;
    double ms;     /* summed event time */
    double flops;  /* algorithmic FLOPs of those launches (2*M*N*K etc.; 0 for byte-bound kernels) */
    double bytes;  /* algorithmic HBM bytes of those launches (operands read once + outputs written once) */
} s3enc_profile_entry;
int s3enc_profile_read(s3enc_handle h, s3enc_profile_entry* entries, int32_t max_entries, int32_t* n_entries);

/* Copy an intermediate of the LAST forward to the host as fp32 (test hook): the last three conv layers
 * ("conv4".."conv6" for the 7-layer stack), "feat_ln", "proj", "posconv", "qkv0", "attn0" ("qkv0" / "attn0" name the buffers: after a
 * whole forward they hold the LAST layer's contents).  Synchronises.
 * Diagnostic (tools/two_stream_probe.py --taps): with the environment variable S3ENC_DEBUG_STOP = k set when the library loads, every
 * forward ends behind stage k — 1 + i: conv layer i, 20: the feature LayerNorm, 21: post_extract_proj, 22: the positional conv, 30 .. 34:
 * layer 0's q|k|v / attention / out_proj / LayerNorm / fc1, 40 + l: in front of layer l — writes NO states, and keeps "conv0" .. as taps
 * too (a conv tap is whole only for the last two conv layers that ran: the stack ping-pongs between two buffers).  Conformer
 * handles: "ffn1_0" (layer 0 after x + 0.5 FFN1), "attn0", "conv0_mod" (the conv module's pointwise_conv2 operand), "ffn2_0"
 * (before final_layer_norm) — buffers later layers reuse: whole for a one-layer model or with S3ENC_DEBUG_STOP = 41. */
int s3enc_debug_tap(s3enc_handle h, const char* name, float* host_out, int64_t max_elems, int64_t* n_elems);
/* Measurement hook (no reference counterpart): `workgroups` x `threads` idle threads that hold their CU slots for `milliseconds` on
 * `stream` — a stand-in for a collective's channel kernels running beside the encoder (bench.py --steal-cus). */
int s3enc_debug_occupy_cus(int32_t workgroups, int32_t threads, double milliseconds, void* stream);  /* milliseconds <= 10000 */
/* Measurement hook (no reference counterpart): writes {shader-clock counter, reference-clock counter, reference rate in kHz} of XCD 0
 * to three device uint64 on `stream`.  Two samples around a region give its average shader clock: d(out[0]) / d(out[1]) x out[2]
 * (hipDeviceAttributeWallClockRate, 100 MHz) — bench.py's `clock_ghz`, so that a slow box reads as a slow box. */
int s3enc_debug_clock_sample(uint64_t* out3_device, void* stream);
/* Test hook (no reference counterpart, touches no device): the workgroups of one exact-fp32 tile-GEMM launch (gemmt.hip) in blockIdx
 * order, through the kernel's own block -> tile map: M x N per batch, bulk tiles of 64 tm rows (tm 1..4), `tail` as the "gemm32_tail"
 * key below, on a part of `cus` CUs.  Writes *n_items = the launch's grid, and — when items4_host holds max_items >= *n_items entries —
 * four host int32 per workgroup: batch, first row, rows, first column. */
int s3enc_debug_gemm_schedule(int32_t M, int32_t N, int32_t batches, int32_t tm, int32_t tail, int32_t cus, int32_t* items4_host,
                              int64_t max_items, int64_t* n_items);

/* Process-wide tuning knobs (kernel-variant selection for A/B measurements; results are unchanged, except "gelu32"):
 *   "gemm_variant": gemm.hip's 128x128 kernel: bit 0 = 64-byte K stages (else 128), bit 1 = LDS-DMA staging, bit 2 = no
 *                   XCD-aware tile order;
 *   "gemm32_big":   exact-fp32 tile kernel (gemmt.hip): 0 off (gemm.hip), 1 = tile height by shape (default), 2 / 3 / 4 / 5 =
 *                   force 256 / 192 / 128 / 64 rows;  "gemm_x3_tile": the same for S3ENC_F32X3 (1 = only small shapes);
 *   "gemm32_tail":  exact-fp32 tile kernel: a launch of 256 / 192 / 128-row tiles may end with a tail region of 64-row tiles, the last
 *                   workgroups dispatched, so that the last round of co-resident workgroups is not nearly empty (every height
 *                   gives the same bits): 0 = never, 1 (default) = where the round model of gemmt.hip says it pays, 2 = every
 *                   such launch, with the largest tail its M allows (one bulk tile when M exceeds the height, else none);
 *   "gemm32_tail_units": lab probe under "gemm32_tail" = 1: 0 (default) = the model's tail, n = a tail of n 64-row units of every
 *                   batch's M (clamped to M) on every such launch;
 *   "gemm16_big":   large-tile kernel of the 16-bit modes: 0 off, 1 = one workgroup per CU (256x256 or 192x256 tiles by CU
 *                   utilisation; 5 / 6 force either), 2 = 128x256, 4 = 128x256 with a 3-stage ring (two workgroups per
 *                   CU), 7 = mode 1's tiles walked by one persistent workgroup per CU, 8 = 7 with the epilogue's stores left
 *                   draining under the next tile's first K steps (profiles/r04_gemm16_overlap.md), 9 / 10 = 7 / 8 with the
 *                   row-per-lane epilogue (no LDS transpose) wherever it is legal, 3 = chosen by shape (default: 7);
 *   "gemm16_rows":  1 (default) = under mode 7 the GELU epilogues with a 16-bit output (conv1-5, fc1) take the row-per-lane form
 *                   (profiles/r04_gemm16_epilogue.md), 0 = never;
 *   "gemm16_pp":    under mode 7 / 9, which fragment steps of a K step carry a wave's LDS-DMA pieces: 0 (default) = steps 0 / 1 for
 *                   every wave, non-zero = waves 4-7 (the SIMD partners of waves 0-3) steps 1 / 2 instead — a schedule change only,
 *                   measured within 1-3 % of the default (profiles/r05_gemm16_loop_probe.md);
 *   "gemm16_mx":    S3ENC_F16X2 only, bit mask: which GEMMs take their second weight term as an MX-fp4 image on the scaled-MFMA pipe
 *                   (gemm16.hip MXW: 4.8e-5 of weight error per GEMM instead of 5e-7) where the shape allows — 1 conv1, 2 q|k|v, 4 fc1,
 *                   8 fc2, 16 = (read at s3enc_create) also weights whose 256-row tiling needs fewer CU-rounds at the reference batch — which weights
 *                   take it is decided per weight, never per batch; default 14; 0 = two fp16 terms everywhere.  Results
 *                   differ at the 1e-5 ... 1e-4 level (profiles/r05_mx_second_term.md);
 *                   The mask is read at s3enc_create: only the kinds it names get an image (narrowing it on a live handle works,
 *                   widening needs a new handle);
 *   "forward_chain": 1 (default) = a forward of a 16-bit / split-precision handle (S3ENC_BF16, S3ENC_F16, S3ENC_F16X2, S3ENC_F32X3) starts, on the
 *                   device, behind the previous such forward of ANY handle of the process on that device (hipStreamWaitEvent on one event per
 *                   device; no host wait; with one handle on one stream it adds nothing to stream order).  Forwards of several handles
 *                   overlapping on four or more streams were measured NOT bit-stable in those modes — rare rows a few 16-bit ulps off, never
 *                   with two streams, never in S3ENC_F32 (profiles/r06c_concurrent_forwards.md; round 6's fourth session traced every such row to the first
 *                   conv layer's kernel computing single frames wrong while waves that issue the double-rate 16-bit MFMA (v_mfma_f32_32x32x16) share its SIMD —
 *                   a cross-wave effect; the 16-bit tile-GEMM kernels therefore claim their SIMD's whole register file, r06d) — so a
 *                   serving process that keeps one encoder per model or per worker thread gets every utterance's own bits by default.
 *                   0 = such forwards may overlap (small batches then fill the chip together: four 8 x 10 s forwards 12.1 -> 8.5 ms);
 *                   (round 6, fourth session: the differing rows originate in the first conv layer's kernel of the 16-bit modes and nowhere
 *                   else — profiles/r06d_concurrent_forwards_exclusions.md);
 *   "conv0_fast":   16-bit outputs of the first conv layer: 1 (default) = packed fp32 taps and the packed one-transcendental GELU, 0 = scalar taps
 *                   and libm erff (about twice that kernel's time; results a few 16-bit ulps apart).  With 0 — and forward_chain = 0 — 32 of 32
 *                   measured runs of four / eight overlapping forwards kept their bits; why is not understood, so this is a diagnostic
 *                   switch and the forward chain stays the protection;
 *   "comm_self_p2p": S3ENC_EXCHANGE_DIRECT test hook: 1 = a rank's own block travels as an ncclSend-to-self / ncclRecv-from-self pair
 *                   inside the state's group instead of a device copy (how the all-pairs code executes on a one-GPU box); default 0;
 *   "fp16x2_conv1_f32": S3ENC_F16X2, read at s3enc_create: 1 = conv0 writes fp32 activations and conv1 reads them through the three-term
 *                   GEMM like conv2.. already do (removes the mode's last fp16 rounding inside the conv stack: the worst weight seed of
 *                   profiles/r06_parity_seeds.md moves from 8.3e-4 to ~7e-4, for conv1 at the three-term rate); default 0;
 *   "attn_persist": 1 = the attention kernels run as persistent workgroups that fetch the next (batch, head, query block) item's
 *                   operands under the current item's last key tile, 0 (default) = the one-shot grid; bit-identical results; a measured
 *                   prototype that lost (profiles/r06_attention_persist.md), kept for re-measurement;
 *   "reserve_cus":  CUs the persistent one-workgroup-per-CU GEMM of the 16-bit modes leaves out of its grid (default 0; a measurement
 *                   knob — leaving CUs to a collective's channel kernels costs more than sharing them: profiles/r05_cu_contention.md;
 *                   tests/test_col_edges_gpu.py sets 128 to make the persistent grid walk several tiles per workgroup on small shapes);
 *   "rnn_split":    the length-aware recurrence (s3enc_op_rnn_len, S3ENC_APC handles): 0 = one launch per layer runs all steps, one
 *                   workgroup per utterance; 1 / 2 / 4 / 8 = the step-split form: one launch per time step on a (S, B) grid, workgroup
 *                   (s, b) owning hidden / S units of utterance b (hidden / S a multiple of 64, S * B <= 256; refused otherwise) —
 *                   the same bits for every S; -1 (default) = S = 8 for a GRU at hidden = 512 with 8 B <= 256, where it was measured
 *                   to win (27.0 against 88.8 ms per 32 x 10 s apc_360hr forward, profiles/apc_360hr_fp32.md), one launch elsewhere;
 *   "npc_skip_taps": S3ENC_NPC handles: 1 (default) = the masked convolutions walk their two runs of live taps only (convtaps.hip: the
 *                   masked taps are neither fetched nor multiplied), 0 = the same kernel over all kernel_size taps on weights whose
 *                   masked taps are stored as zeros — equal values; measured 6.13 against 10.55 ms per 32 x 10 s npc_360hr forward
 *                   (profiles/npc_360hr_fp32.md);
 *   "melspec_fft":  S3ENC_BYOL_A handles and s3enc_op_melspec1024: 1 (default) = the 1024-point STFT as a real FFT in LDS, one
 *                   workgroup per frame (melspec.hip), 0 = the overlapping-row GEMM against the folded hann x DFT matrix — the
 *                   yardstick and the fallback; results differ in the last bits; measured 1.04 against 1.75 ms per 32 x 10 s
 *                   byol_a_2048 forward (profiles/byol_a_fp32.md);
 *   "conv2d_n64":   S3ENC_BYOL_A handles and s3enc_op_conv2d3x3_affine: 1 (default) = Cout <= 64 runs on the 64-wide n-tile of
 *                   conv2d.hip, 0 = on the 128-wide one, half of whose MFMA columns are then padding — the same bits; measured 1.04
 *                   against 1.28 ms per forward (profiles/byol_a_fp32.md);
 *   "patch_embed_fused": S3ENC_MAE_AST handles and s3enc_op_patch_embed: 1 (default) = the patch embedding as one implicit GEMM that reads
 *                   the image in place (patchembed.hip), 0 = a gather kernel that writes the (B * tokens, kt * kc) rows, the tile GEMM
 *                   and a position add — the yardstick and a second implementation, held to the fixture bound; measured 0.0625
 *                   against 0.0798 ms per 32 x 10 s mae_ast_patch embedding, the forwards indistinguishable (profiles/mae_ast_fp32.md);
 *   "patch_strided_fused": S3ENC_SSAST handles and s3enc_op_patch_embed_strided: 1 (default) = the overlapping patch embedding as one
 *                   implicit GEMM that reads the image in place (patchstrided.hip), 0 = a gather kernel that writes the (windows *
 *                   tokens, tshape * fshape) rows, the tile GEMM and a position add — the yardstick and a second implementation, held
 *                   to the same bound; measured 0.147 against 0.187 ms per 32 x 10 s ssast_patch_base embedding, the forwards
 *                   indistinguishable and the states bit-equal (profiles/ssast_fp32.md);
 *   "ssast_chunk": S3ENC_SSAST handles: tokens per pass of the embedding and the layers (default 65536, 1..4194304; whole windows, at
 *                   least one): the workspace is bounded by it and does not grow with B x nseg; a row's bits do not depend on it;
 *   "stem_fused":   S3ENC_BYOL_S resnetish handles: 1 = the stem's 7 x 7 convolution, affine, ReLU and 3 x 3 / stride-2 max-pool in one
 *                   kernel (2.25 x the multiply-adds, no un-pooled map), 0 (default) = the un-pooled map written once and pooled by
 *                   a second kernel — the same bits; measured 223.0 against 222.2 ms per forward (profiles/byol_s_fp32.md);
 *   "byol_s_chunk": S3ENC_BYOL_S handles: windows per pass of the network (default 1024, 1..4096): the workspace is bounded by it
 *                   (about 6.2 MB per window) and does not grow with B x S; a window's bits do not depend on it; measured 246.9 /
 *                   222.2 / 207.5 / 193.2 ms per 32 x 10 s byol_s_resnetish34 forward at 128 / 256 / 512 / 1024;
 *   "conv_f22":     S3ENC_F32: 1 (default) = conv layers 1.. with kernel 3 and stride 2 (conv1-4 of every extractor) run in the
 *                   two-output form (convf22.hip: 5 block products per pair of outputs instead of 6, fp32 operands and accumulation,
 *                   a different association — results differ in the last bits), 0 = the implicit GEMM;
 *   "conv0_nt":     1 (default) = the fp32 conv0 kernel writes its activation with non-temporal stores, 0 = plain stores;
 *   "ws_inplace":   1 (default) = post-LN layers run LayerNorm 1 and fc2 in place on one fp32 workspace buffer, 0 = two buffers;
 *   "ln1_fold":     16-bit modes, post-LN layers: 1 (default) = LayerNorm 1 writes its 16-bit output and the rows' (mean, rstd) only and
 *                   fc2's epilogue rebuilds the fp32 rows it adds from the row it normalised; 0 = LayerNorm 1 writes them; same bits;
 *   "ln_preload":   1 (default) = the row LayerNorm fetches gamma / beta together with the row instead of behind the reductions; same bits;
 *   "ln_rows":      rows per wave of the row LayerNorm: 1 (default), 2 = two rows' loads in flight (launches of >= 8192 rows); same
 *                   bits; measured 2-3 % slower, kept for re-measurement;
 *   "gn_lag_one_block": 1 (default) = the GroupNorm lag sums of the waveform come from one workgroup per (4096-frame chunk,
 *                   utterance) over an LDS-staged window, 0 = the earlier k0-workgroups kernel; same bits
 *                   (profiles/r06b_gn_stats.md);
 *   "gelu32":       S3ENC_F32 only: 1 = the one-transcendental erf-GELU every mode uses (default; csrc/common.h gelu_fast: as
 *                   close to an fp64 erf-GELU as 0.5 x (1 + erff(x / sqrt 2)) evaluated in fp32), 0 = libm erff — results
 *                   differ in the last bits. */
int s3enc_set_tuning(const char* key, int32_t value);
/* The same keys for ONE handle: the handle starts from the process-wide values as they are at the first call and keeps its own
 * copy from then on; its forwards use that copy (per calling thread), other handles and the s3enc_op_* entry points do not. */
int s3enc_set_handle_tuning(s3enc_handle h, const char* key, int32_t value);

/* ---- single-kernel entry points (parity tests of each HIP kernel against the oracle) -------------------
 * All pointers are device pointers; dtype is S3ENC_F32/BF16/F16 for the 16-bit-capable operands
 * (16-bit data are raw uint16). */

/* out[b][m][n] = epilogue( sum_k A[b][m][k] * W[n][k] ):  A rows start at A + b*a_batch_stride + m*lda
 * (elements; lda < K expresses an overlapping strided-conv window), W is (N, K) row-major.
 * epilogue: + bias[n]; GELU if act; + residual (fp32, same indexing as out32); rows m >= row_limit[b] -> 0.
 * Writes out32 (fp32) and/or out16 (dtype) when non-NULL.  dtype S3ENC_F32X3: fp32 A / W / out32, three bf16 MFMAs per
 * product (K % 32 == 0, M, N >= 128; synchronises).  dtype S3ENC_F16X2: fp16 A and out16, W is the (N, 2K) fp16 image
 * [hi(K) | lo(K)] per row with w = hi + lo (K % 64 == 0, else only the hi half is used). */
int s3enc_op_gemm(int32_t dtype, const void* A, int64_t lda, int64_t a_batch_stride, const void* W,
                  const float* bias, int32_t M, int32_t N, int32_t K, int32_t batches, int32_t act,
                  const float* residual, const int32_t* row_limit, float* out32, void* out16, int64_t ldo,
                  int64_t o_batch_stride, void* stream);

/* conv0 of the feature extractor with its normalisation and GELU (wav2vec2_model.py:2879-2906) on raw waveforms:
 * per-utterance waveform layer-norm if `normalize`; GroupNorm(C, C) over all L0 frames incl. the zero padding when
 * gn_gamma != NULL (statistics from the waveform's lag sums), else LayerNorm(C) per frame when ln_gamma != NULL.
 * wavs / lengths as in s3enc_forward; w0 (C, 10), bias (C or NULL), gamma / beta: device fp32; out: device
 * (B, L0, C) of `dtype`, L0 = (n_max - 10) / stride + 1. */
int s3enc_op_conv0(int32_t dtype, const float* const* wavs, const int64_t* lengths, int32_t B, int64_t n_max,
                   int32_t normalize, const float* w0, const float* bias, const float* gn_gamma, const float* gn_beta,
                   const float* ln_gamma, const float* ln_beta, int32_t C, int32_t stride, void* out, void* stream);
/* WavLM gate (wavlm/modules.py:535-549) from the attention input x (device fp32 (B, T, H*64)):
 * gate[b][h][t] = a * (b * grep_a[h] - 1) + 2,  a|b = sigmoid(sum4(grep_linear(x_head))).  grep_w (8, 64), grep_b (8),
 * grep_a (H): device fp32. */
int s3enc_op_wavlm_gate(const float* x, const float* grep_w, const float* grep_b, const float* grep_a, int32_t B, int32_t T,
                        int32_t H, float* gate, void* stream);

/* Row LayerNorm over C (eps 1e-5, biased variance), optional erf-GELU, fp32 in, fp32 and/or dtype out. */
int s3enc_op_layernorm(int32_t dtype, const float* x, const float* gamma, const float* beta, int32_t rows,
                       int32_t C, int32_t act, float* out32, void* out16, void* stream);

/* Multi-head self-attention on a fused (B*T, 3D) q|k|v buffer, head_dim 64, keys >= valid[b] masked.  q arrives
 * pre-scaled by head_dim^-0.5 — for dtype S3ENC_BF16 / S3ENC_F16 by head_dim^-0.5 * log2(e): the 16-bit kernels
 * work on base-2 scores, the engine folds either factor into W_q at s3enc_create; optional WavLM gated relative-position bias: score += gate[b][h][i] * table[h][clamp(j-i, -R, R) + R]
 * with a (H, 2R+1) table (the bucket of wavlm/modules.py:418-446 is constant for |j-i| >= max_distance, so
 * R = max_distance serves every T).  table_R = 0 is accepted: a (H, 1) table adds one constant per query, which the softmax
 * ignores — the result is the bias-free one to rounding.  Every query row of the T is computed, the padded ones (t >= valid[b])
 * like the rest.  valid[b] must be at least 1: with valid[b] = 0 the key loop runs zero tiles and the utterance's rows are
 * 0 * (1 / 0) = NaN (nothing is read or written out of bounds).  The engine never passes 0: every forward refuses an utterance
 * without a valid frame before it launches anything ("too short to produce a valid frame"), the chunked Mockingjay path clamps a
 * chunk's key count to 1, and s3enc_valid_frames, which does answer 0 for such an utterance, is a query and launches nothing. */
int s3enc_op_attention(int32_t dtype, const void* qkv, void* out, const int32_t* valid, int32_t B, int32_t T,
                       int32_t H, const float* bias_table, int32_t table_R, const float* gate, void* stream);

/* Conformer convolution module after pointwise_conv1 (wav2vec2_model.py:313-393): out = swish(DW(GLU(x)) * scale + shift) with
 * GLU(a | g) = a * sigmoid(g) over the channel halves of x, DW the depthwise Conv1d of kernel K (odd, <= 63) with zero padding
 * (K-1)/2 inside each utterance's T-row block (the batch-padded time axis), scale / shift the eval BatchNorm folded by the caller.
 * x: device fp32 (B*T, 2D); taps: device fp32 (D, K) (depthwise weight already times scale); shift: device fp32 (D);
 * out: device fp32 (B*T, D).  D % 64 == 0. */
/* (measured 51.5 us at B*T = 32 x 499, D = 1024: 196 MB at 3.81 TB/s) */
int s3enc_op_conformer_conv(const float* x, const float* taps, const float* shift, int32_t B, int32_t T, int32_t D, int32_t K,
                            float* out, void* stream);
/* Conformer rel_pos self-attention (RelPositionMultiHeadedAttention, wav2vec2_model.py:165-252), fp32, head_dim 64, keys >=
 * valid[b] masked:  score(i, j) = q_i . k_j + (q_i + qadd_h) . P[(j - i) + T - 1][h*64 ...]  with q the (B*T, 3D) buffer's q
 * columns (the engine passes (q + pos_bias_u) / 8), P (2T-1, D) = linear_pos(pe) for this T, qadd (H, 64) = (pos_bias_v -
 * pos_bias_u) / 8.  Neither a (B, H, T, 2T-1) tensor nor the score matrix is stored.  (1.62x the plain fp32 attention's time at
 * B = 32, H = 16, T = 499.) */
int s3enc_op_relpos_attention(const float* qkv, float* out, const int32_t* valid, int32_t B, int32_t T, int32_t H, const float* P,
                              const float* qadd, void* stream);

/* wav2vec: the row pass behind a convolution (wav2vec_model.py:25-56,83-113,248-286): Fp32GroupNorm(1, C) over the `rows` x C values
 * of each utterance (biased variance, eps 1e-5; statistics in double) -> ReLU -> [(y + res) * scale] -> [log(|y| + 1)].
 * x: device fp32 (B, rows, C); gamma / beta: device (C) or NULL (non_affine_group_norm); res: device (B, rows, C) or NULL.
 * dst: device (B, pad + rows, C) or NULL: the next convolution's operand, its `pad` leading rows of every utterance filled with
 * frame 0 (ReplicationPad1d) or zeros (pad_zero); state: device (B, rows, C) or NULL; acc: device (B, rows, C) or NULL — the
 * Featurizer term acc (+)= acc_w * (acc_norm ? layer_norm(y) : y), written instead of added when acc_init.  Synchronises. */
int s3enc_op_gn1_apply(const float* x, const float* gamma, const float* beta, const float* res, float scale, int32_t log_compress,
                       int32_t B, int32_t rows, int32_t C, int32_t pad, int32_t pad_zero, float* dst, float* state, float* acc,
                       float acc_w, int32_t acc_norm, int32_t acc_init, void* stream);
/* Hard selection of a quantizer (GumbelVectorQuantizer in eval, wav2vec2_model.py:1733-1775; KmeansVectorQuantizer's argmin on
 * negated distances, wav2vec_model.py:193-204): per (row, group) the index of the largest of V scores (ties: the lowest index),
 * and the gathered variables.  scores: device fp32 (rows, G, V); table: device fp32 (shared ? 1 : G, V, Dv); ids: device int64
 * (rows, G) or NULL; out: device fp32 (rows, G * Dv) or NULL. */
int s3enc_op_argmax_gather(const float* scores, const float* table, int32_t shared, int64_t rows, int32_t G, int32_t V, int32_t Dv,
                           int64_t* ids, float* out, void* stream);

/* modified CPC: the row pass behind a convolution (cpc/model.py:33-59,99-104): per frame over the C channels
 * y = relu((x - mean) * rsqrt(var + 1e-5) * gamma + beta), var unbiased (divided by C - 1).  x: device fp32 (B, rows, C);
 * gamma / beta: device (C) or NULL (1 / 0); dst: device (B, pad + rows + pad, C) or NULL: the next convolution's operand, its
 * `pad` rows in front of and behind every utterance written as zeros; state: device (B, rows, C) or NULL.  C % 4 == 0, C <= 1024. */
int s3enc_op_channelnorm_relu(const float* x, const float* gamma, const float* beta, int32_t B, int32_t rows, int32_t C,
                              int32_t pad, float* dst, float* state, void* stream);
/* The recurrence of nn.LSTM (cell 0) / nn.GRU (cell 1), batch_first, zero initial state, all T steps in one launch, one
 * workgroup per utterance.  gates = 4 (i, f, g, o) / 3 (r, z, n).  pre: device fp32, row (b, t) at pre + (b * T + t) * ld_pre,
 * gates * H values x W_ih^T + b_ih plus the part of b_hh that may be folded (LSTM: all of it; GRU: the r and z parts only).
 * w_hh_host: HOST fp32 (gates * H, H), nn's weight_hh_l*; packed and uploaded inside.  b_hn: device (H), GRU's b_hh[2H:3H], NULL
 * for LSTM.  out: device fp32, row (b, t) at out + (b * T + t) * ldo, H values.  H % 64 == 0, H <= 512.  Synchronises. */
int s3enc_op_rnn(int32_t cell, const float* pre, const float* w_hh_host, const float* b_hn, int32_t B, int32_t T, int32_t H,
                 int64_t ld_pre, float* out, int64_t ldo, void* stream);

/* s3enc_op_rnn with packed-sequence semantics (pack_padded_sequence / pad_packed_sequence): utterance b runs len_host[b] steps
 * (HOST int32 (B), each in 1..T) and its rows [len, T) are written as zeros.  res: device fp32 or NULL, row (b, t) at
 * res + (b * T + t) * ld_res, H values added to the row written (the carried state stays the un-summed h_t).  out must be
 * 16-byte aligned and ldo a multiple of 4.  With every length equal to T and no res the result is bit-identical to
 * s3enc_op_rnn.  Synchronises. */
int s3enc_op_rnn_len(int32_t cell, const float* pre, const float* w_hh_host, const float* b_hn, const int32_t* len_host,
                     const float* res, int64_t ld_res, int32_t B, int32_t T, int32_t H, int64_t ld_pre, float* out, int64_t ldo,
                     void* stream);

/* Stride-1 nn.Conv1d(C, N, k, padding = (k - 1) / 2) on channel-last rows, exact fp32, with `mask` taps in the middle of the
 * kernel zeroed — taps [(k - mask) / 2, (k + mask) / 2), NPC's MaskConvBlock — and never read (convtaps.hip):
 *   v[b][t][:] = act(sum_{j live} W[:, :, j] x[b][t + j - P] + bias [+ res[b][t]]),  P = (k - 1) / 2,  act 0 none / 1 ReLU / 2 tanh.
 * x: device fp32, the BORDERED operand (B, T + 2 P, C): per utterance P zero rows, the T data rows, P zero rows (the caller zeroes
 * the borders).  w_host: HOST fp32 (N, C, k), nn.Conv1d's layout; packed (live taps only, tap-major) and uploaded inside.  bias:
 * device fp32 [N] or null.  mask: 0 or an odd number below k (k odd).  res: optional device fp32, row (b, t) at res + (b * T + t) *
 * ld_res, added BEFORE the activation.  Up to three destinations, at least one: dst, a bordered (B, T + 2 dst_pad, ldo) buffer of
 * which only rows [dst_pad, dst_pad + T) and columns [0, N) of each utterance are written; state, (B, T, N) contiguous; sum, (B, T,
 * N) contiguous: sum = sum_init ? v : sum + v.  dense != 0 runs the same kernel over all k taps on weights whose masked taps are
 * stored as zeros: equal values.  C % 16 == 0, N % 4 == 0, ldo % 4 == 0, ldo >= N, ld_res % 4 == 0, 16-byte aligned pointers.  A
 * row's bits depend neither on B, nor on its place in the batch, nor on T's tiling.  Synchronises. */
int s3enc_op_conv_taps(const float* x, const float* w_host, const float* bias, int32_t B, int32_t T, int32_t C, int32_t N, int32_t k,
                       int32_t mask, int32_t act, const float* res, int64_t ld_res, float* dst, int32_t dst_pad, int64_t ldo,
                       float* state, float* sum, int32_t sum_init, int32_t dense, void* stream);

/* nn.Conv1d(C, C, 3, stride = 2) without padding on channel-last rows, exact fp32, in the two-output form (convf22.hip; conv1-4 of
 * the HuBERT / wav2vec 2.0 / WavLM / data2vec extractors in the S3ENC_F32 mode):
 *   out[b][t][:] = act(W[:, :, 0] x[b][2t] + W[:, :, 1] x[b][2t + 1] + W[:, :, 2] x[b][2t + 2] + bias),  t in [0, M),
 *   act 0 none / 1 GELU (the tuning key "gelu32" chooses its form, as everywhere in the fp32 mode).
 * x: device fp32, utterance b's frames at x + b * x_bs; frames [0, 2M] are read and nothing behind frame 2M is.  w_host: HOST fp32
 * (C, C, 3), nn.Conv1d's layout; packed tap-major, with the (C, C) sum of taps 0 and 2 beside it, by the code s3enc_create uses,
 * and uploaded inside.  bias: device fp32 [C] or null.  row_limit: device int32 [B] or null: rows [row_limit[b], M) of utterance b
 * are written as +0.0.  out: utterance b's rows at out + b * o_bs; rows [0, M) only are written.  There is no other kernel behind
 * this entry; refused by message: the tuning key "conv_f22" = 0, C not a multiple of 32, x_bs < (2M + 1) C (frame 2M must exist),
 * o_bs < M C, strides that are not multiples of 4 floats, pointers that are not 16-byte aligned, null x / w_host / out.  A row's
 * bits depend on its three frames and the weights only: not on M, B, its utterance's place, or the grid.  Synchronises. */
int s3enc_op_conv_k3s2(const float* x, int64_t x_bs, const float* w_host, const float* bias, const int32_t* row_limit, int32_t B,
                       int32_t M, int32_t C, int32_t act, float* out, int64_t o_bs, void* stream);

/* Stride-1 nn.Conv2d(C, N, 3, padding = 1) on channel-last images, exact fp32, with bias -> act -> optional nn.MaxPool2d(2, 2) in
 * one pass (conv2d.hip; VGGish's features stack):
 *   v[b][y][x][:] = act(sum_{ky, kx} W[:, :, ky, kx] img[b][y + ky][x + kx] + bias),  act 0 none / 1 ReLU;
 *   pool = 1: out[b][y'][x'] = max of v over the 2 x 2 window (a NaN stays a NaN), H and W even; pool = 0: out = v.
 * x: device fp32, the BORDERED operand (B, H + 2, W + 2, C): every example's outermost pixels are zeros (the caller zeroes them).
 * w_host: HOST fp32 (N, C, 3, 3), nn.Conv2d's layout; packed tap-major (N, 9 C) and uploaded inside.  bias: device fp32 [N] or null.
 * dst: a bordered (B, Ho + 2 dst_pad, Wo + 2 dst_pad, ldo) buffer, Ho x Wo = H x W or H / 2 x W / 2 under pool, of which only the
 * interior pixels and columns [0, N) are written; dst_pad = 0 is a plain (B, Ho, Wo, ldo) tensor.  The un-pooled activation is
 * never written.  C = 1 runs the first-layer VALU kernel, otherwise C % 16 == 0 and the product runs on the fp32 MFMA as an
 * implicit GEMM over the pixels of all examples; N % 4 == 0, ldo % 4 == 0, ldo >= N, 16-byte aligned pointers (C = 1: x 4-byte).
 * An example's bits depend neither on B, nor on its place in the batch, nor on the tiling; the pooled output is bit for bit the
 * max over the un-pooled output.  Synchronises. */
int s3enc_op_conv2d3x3(const float* x, const float* w_host, const float* bias, int32_t B, int32_t H, int32_t W, int32_t C, int32_t N,
                       int32_t act, int32_t pool, float* dst, int32_t dst_pad, int64_t ldo, void* stream);

/* s3enc_op_conv2d3x3 with BYOL-A's additions (conv2d.hip); what the two entries share is described above.
 *   scale / shift: device fp32 [N] or both null.  With them v = act(acc * scale[n] + shift[n]) — an eval-mode BatchNorm behind the
 *   conv, scale = gamma / sqrt(var + eps), shift = (conv_bias - mean) * scale + beta — and `bias` must be null.  Null scale is the
 *   acc + bias path, bit for bit s3enc_op_conv2d3x3's.
 *   pool_floor = 1 (needs pool = 1): odd H / W are allowed, Ho = H / 2 and Wo = W / 2 rounded down as nn.MaxPool2d(2, 2) does; the
 *   dropped last row / column is never computed.  H, W >= 2.
 *   Cout <= 64 runs on a 64-wide n-tile (tuning key conv2d_n64 = 0: on the 128-wide one); an output's bits do not depend on it. */
int s3enc_op_conv2d3x3_affine(const float* x, const float* w_host, const float* bias, const float* scale, const float* shift, int32_t B,
                              int32_t H, int32_t W, int32_t C, int32_t N, int32_t act, int32_t pool, int32_t pool_floor, float* dst,
                              int32_t dst_pad, int64_t ldo, void* stream);

/* BYOL-A's front end on a table of segments (melspec.hip): segments: device fp32 (nseg, L) contiguous.  Every segment is
 * reflect-padded by 512 about its own ends; 1 + L / 160 frames of a 1024-point periodic-hann STFT; |X|^2 over 513 bins; 64 HTK mel
 * triangles 60..7800 Hz; out (nseg, frames, 64) = (log(mel + FLT_EPSILON) - (-5.4919195)) / 5.0389895.  power: null, or device fp32
 * (nseg, frames, 513) that receives |X|^2.  Tuning key melspec_fft: 1 = a real FFT in LDS, one workgroup per frame (a frame's bits
 * depend on its 1024 samples only), 0 = the overlapping-row GEMM against the folded hann x DFT matrix.  Refused by message: L <= 512
 * (the reflection is undefined), L < 1120 (fewer than 8 frames).  Synchronises. */
int s3enc_op_melspec1024(const float* segments, int32_t nseg, int32_t L, float* out, float* power, void* stream);

/* BYOL-S's front end: s3enc_op_melspec1024 with MelSpectrogram(win_length = 400) — a periodic hann(400) behind 312 zeros inside the
 * 1024-point frame — and no normalisation: out (nseg, frames, 64) = log(mel + FLT_EPSILON).  Always the FFT kernel.  Refused by
 * message: L <= 512.  Synchronises. */
int s3enc_op_melspec400(const float* segments, int32_t nseg, int32_t L, float* out, float* power, void* stream);

/* The general form of s3enc_op_conv2d3x3_affine (conv2d.hip, the GEN instantiations; a ResNet BasicBlock's layers): Conv2d(C, N, k,
 * stride, padding = (k - 1) / 2) on channel-last images, then act(acc * scale[n] + shift[n] + res[b][y][x][n]).
 *   x: device fp32 (B, H + 2, W + 2, C) with a zero border, for k = 1 as well (the border is then never read).  w_host: HOST fp32
 *   (N, C, k, k) as nn.Conv2d holds it.  k: 3 or 1.  stride: 1 or 2; Ho = (H + 2 p - k) / stride + 1, rounded down, Wo alike.  bias /
 *   scale / shift: as for s3enc_op_conv2d3x3_affine.  res: device fp32 (B, Ho, Wo, N) contiguous, or null.  dst: the interior of a
 *   (B, Ho + 2 dst_pad, Wo + 2 dst_pad, ldo) image whose border is never touched.  C a multiple of 16, N a multiple of 4.
 *   The M axis is the output pixels of all examples and the K order is fixed (kernel rows, taps, the step's order): an example's bits
 *   depend neither on B, nor on its place, nor on the tile; k = 3, stride = 1, res = null is bit for bit s3enc_op_conv2d3x3_affine
 *   without pooling.  Synchronises. */
int s3enc_op_conv2d_res(const float* x, const float* w_host, const float* bias, const float* scale, const float* shift, const float* res,
                        int32_t B, int32_t H, int32_t W, int32_t C, int32_t N, int32_t k, int32_t stride, int32_t act, float* dst,
                        int32_t dst_pad, int64_t ldo, void* stream);

/* BYOL-S's ResNet stem (stem.hip): Conv2d(1, 64, 7, stride 1, padding 3, no bias) -> per-channel affine -> ReLU -> MaxPool2d(3, 2, 1)
 * on (H, 64) single-channel images.  x: device fp32 (B, H + 8, 64 + 8), the 4 outermost rows / columns zeros.  w_host: HOST fp32 (64,
 * 1, 7, 7).  scale / shift: device fp32 [64].  dst: a (B, Hp + 2, 32 + 2, 64) image, Hp = (H - 1) / 2 + 1: its interior is written, its
 * border is never touched.  fused = 1: one kernel; fused = 0: map, device fp32 (B, H + 2, 64 + 2, 64) with a zero border, receives the
 * un-pooled activation and a second kernel pools it — the same bits.  Negative zero behind the ReLU is written as +0; a NaN stays a
 * NaN.  Synchronises. */
int s3enc_op_stem7x7_pool(const float* x, const float* w_host, const float* scale, const float* shift, int32_t B, int32_t H, int32_t fused,
                          float* dst, float* map, void* stream);

/* The patch embedding of (frames, 128) fp32 images as an implicit GEMM over the tokens of all utterances (patchembed.hip): nn.Unfold
 * with kernel = stride = (kt, kc), Linear(kt * kc, N) and a position row in one pass.
 *   out[b][t*V+v][n] = sum_{r<kt} sum_{c<kc} img[b][t*kt + r][v*kc + c] * w[n][r*kc + c] + bias[n] + (t*V+v < kv[b] ? pos[t*V+v][n] : 0)
 *   img: device fp32, utterance b at img + b * img_bs, rows of 128 floats; only rows [0, Tt * kt) are read.  w_host: HOST fp32 (N, kt *
 *   kc), the Linear's weight as stored.  bias: device [N] or null.  pos: device (>= Tt * V, N) with kv: device int32 [B], or both
 *   null.  out: device (B, Tt * V, N), V = 128 / kc.  fp32 MFMA on 64-byte K steps in a fixed order (patch rows ascending, then the
 *   step's order): a token row's bits depend neither on B, nor on its place in the batch, nor on Tt, nor on the tile height.
 * Refused by message: kc outside {16, 32, 64, 128}, kt outside 1..32, N % 4 != 0, img_bs < Tt * kt * 128 or not a multiple of 4,
 * operands that are not 16-byte aligned.  Tuning key patch_embed_fused = 0: gather + tile GEMM + position add.  Synchronises. */
int s3enc_op_patch_embed(const float* img, int64_t img_bs, const float* w_host, const float* bias, const float* pos, const int32_t* kv,
                         int32_t B, int32_t Tt, int32_t kt, int32_t kc, int32_t N, float* out, void* stream);

/* The patch embedding with OVERLAPPING patches of (rows, 128) fp32 images as an implicit GEMM over the tokens of all windows
 * (patchstrided.hip): SSAST's Conv2d(1, N, (fshape, tshape), stride (fstride, tstride)), the position row and the sequence layout.
 *   out[w][2 + ti*f_dim + fi][n] = sum_{t<tshape} sum_{f<fshape} img[w][ti*tstride + t][fi*fstride + f] * w[n][t*fshape + f] + bias[n]
 *                                  + pos[ti*f_dim + fi][n];   out[w][0 | 1][n] = prefix[0 | 1][n]
 *   f_dim = (128 - fshape) / fstride + 1, t_dim = (rows - tshape) / tstride + 1.  img: device fp32, window w at img + w * img_bs, `rows`
 *   rows of 128 floats: nothing behind them is read.  w_host: HOST fp32 (N, tshape * fshape), the conv weight permuted to [n][t][f].
 *   bias: device [N] or null.  pos: device (f_dim * t_dim, N) in the time-major token order, or null.  prefix: device (2, N) or null
 *   (rows 0 and 1 are then not written).  out: device (nwin, 2 + f_dim * t_dim, N).  tile_rows: 0 = the launcher's choice, 64 | 128 =
 *   that tile height (the bits are the same).  fp32 MFMA on 64-byte K steps in a fixed order: a token's bits depend neither on nwin,
 *   nor on the window it sits in, nor on the tile height.
 * Refused by message: fshape outside {16, 32, 64, 128}, tshape outside 1..32, an odd fstride, rows < tshape, N % 4 != 0, img_bs < rows
 * * 128 or not a multiple of 4, operands that are not 16-byte aligned.  Tuning key patch_strided_fused = 0: gather + tile GEMM +
 * position add (tile_rows is then not read).  Synchronises. */
int s3enc_op_patch_embed_strided(const float* img, int64_t img_bs, const float* w_host, const float* bias, const float* pos,
                                 const float* prefix, int32_t nwin, int32_t rows, int32_t fshape, int32_t tshape, int32_t fstride,
                                 int32_t tstride, int32_t N, int32_t tile_rows, float* out, void* stream);

/* A forward and a backward unidirectional nn.LSTM on packed sequences, side by side, on the batch-shared kernel: one launch per
 * time step for both directions, W_hh read once per step for the whole batch (fp32 MFMA).  pre_fwd / pre_bwd: device fp32, row
 * (b, t) at pre + (b * T + t) * ld_pre, 4 H values (i, f, g, o) of x W_ih^T + b_ih + b_hh, both in the utterance's own time order.
 * The forward direction runs rows 0 .. len - 1, the backward direction rows len - 1 .. 0 (what the reference gets by flipping
 * every utterance before and after its backward stack); no flipped copy is made.  w_hh_fwd_host / w_hh_bwd_host: HOST fp32
 * (4 H, H), packed and uploaded inside.  len_host: HOST int32 (B), each in 1..T.  out: device fp32, 16-byte aligned, row (b, t)
 * at out + (b * T + t) * ldo: the forward h in columns [0, H), the backward h in [H, 2 H); rows [len, T) of both halves are
 * written as zeros.  ldo % 4 == 0, ldo >= 2 H, ld_pre >= 4 H, H % 64 == 0, H <= 1024, B <= 128.  An utterance's bits depend
 * neither on B, nor on its place in the batch, nor on the other lengths.  Synchronises. */
int s3enc_op_lstm_bidir(const float* pre_fwd, const float* pre_bwd, const float* w_hh_fwd_host, const float* w_hh_bwd_host,
                        const int32_t* len_host, int32_t B, int32_t T, int32_t H, int64_t ld_pre, float* out, int64_t ldo,
                        void* stream);
/* The host-side packer of that kernel's W_hh image, for tests: w_hh_host (4 H, H) -> out_host, 4 H * H floats laid out
 * [H / 8 slices][H / 8 k blocks][64 lanes][4]: lane l of slice s and k block kb holds
 * w[((l & 31) / 8) * H + 8 s + (l & 7)][8 kb + 4 (l >> 5) + j], j = 0..3.  Needs no device. */
int s3enc_pack_lstm_bidir_whh(const float* w_hh_host, int32_t H, float* out_host);

/* Convolutional position embedding + residual: out = x + GELU(SamePad(Conv1d(D, D, K, padding=K/2, groups=G)(x)) + bias)
 * (make_conv_pos / SamePad, wav2vec2_model.py:2937-2953,1797-1808).  x, out: device fp32 (B, T, D); w_host: HOST fp32
 * (D, D/G, K), the nn.Conv1d weight with weight_norm already folded; packed and uploaded inside.  D / G must be 32, 48 or 64; every
 * other group width is refused.  Synchronises. */
int s3enc_op_posconv(int32_t dtype, const float* x, const float* w_host, const float* bias, int32_t B, int32_t T, int32_t D,
                     int32_t G, int32_t K, float* out, void* stream);
/* The same op at the group widths D / G = 24 and 40 (the LightHuBERT subnets; posconv_kernel<24>, <40>: the half-tile form of the fp32
 * kernel), which s3enc_op_posconv keeps refusing.  dtype must be S3ENC_F32: the other operand modes are refused by name. */
int s3enc_op_posconv_narrow(int32_t dtype, const float* x, const float* w_host, const float* bias, int32_t B, int32_t T, int32_t D,
                            int32_t G, int32_t K, float* out, void* stream);

/* ---- Featurizer: the consumer of hidden_states (next row of the path) --------------------------------
 * Replaces Featurizer._weighted_sum (s3prl/nn/upstream.py:312-328; upstream/interfaces.py:221-249):
 *   out = sum_l w[l] * (normalize ? F.layer_norm(h_l, (D,)) : h_l),   w = softmax(weights) computed by the caller.
 * hs: device fp32, layer l is the (rows, D) block at hs + l*layer_stride (the slab s3enc_forward writes);
 * w: HOST array of L floats (0 = layer not selected); out: device fp32 (rows, D). */
int s3enc_weighted_sum(const float* hs, int64_t layer_stride, int32_t L, const float* w, int32_t normalize, int64_t rows,
                       int32_t D, float* out, void* stream);
/* Gradient of the above w.r.t. w (the upstream is frozen): grad_w[l] = sum <grad_out, hn_l>; grad_w: device, L floats.
 * scratch: device, s3enc_weighted_sum_backward_scratch(rows, L) doubles, owned by the caller (stream-ordered reuse);
 * asynchronous on `stream`. */
int64_t s3enc_weighted_sum_backward_scratch(int64_t rows, int32_t L);
int s3enc_weighted_sum_backward(const float* hs, int64_t layer_stride, int32_t L, int32_t normalize, int64_t rows,
                                int32_t D, const float* grad_out, float* grad_w, double* scratch, void* stream);

/* ---- the `fbank` baseline upstream (BASELINE configs[0]) --------------------------------------------------------
 * Replaces get_extracter(fbank.yaml) + UpstreamExpert.forward of upstream/baseline (extracter.py:32-90,
 * expert.py:46-79): torchaudio.compliance.kaldi.fbank -> delta, delta-delta -> CMVN over time -> pad_sequence. */
typedef struct s3enc_fbank_config {
    int32_t sample_rate;      /* 16000 */
    int32_t num_mel_bins;     /* 80   (fbank.yaml) */
    float frame_length_ms;    /* 25 */
    float frame_shift_ms;     /* 10 */
    float preemphasis;        /* 0.97 (kaldi default) */
    int32_t delta_order;      /* 2 */
    int32_t delta_win_length; /* 5 */
    int32_t use_cmvn;         /* 1 */
    float cmvn_eps;           /* 1e-10 (extracter.py:80) */
} s3enc_fbank_config;
/* frames of an n-sample utterance (snip_edges): 1 + (n - window) / shift, 0 if shorter than one window */
int s3enc_fbank_num_frames(const s3enc_fbank_config* cfg, int64_t n_samples, int32_t* frames);
/* wavs: host array of B device pointers (borrowed); out: device fp32 (B, T_max, num_mel_bins*(delta_order+1)),
 * zero beyond each utterance's frames (pad_sequence); T_max >= the longest utterance's frame count. */
int s3enc_fbank_forward(const s3enc_fbank_config* cfg, const float* const* wavs, const int64_t* lengths, int32_t B,
                        float* out, int64_t T_max, int32_t device, void* stream);
/* The same with kaldi's window_type: 0 povey (s3enc_fbank_forward, bit for bit), 1 hamming
 * 0.54 - 0.46 cos(2 pi i / (N - 1)) (APC's front end, apc/audio.py:22,82-88).  s3enc_fbank_config is unchanged. */
int s3enc_fbank_forward_ex(const s3enc_fbank_config* cfg, int32_t window, const float* const* wavs, const int64_t* lengths,
                           int32_t B, float* out, int64_t T_max, int32_t device, void* stream);
/* The batch-wide pass of the same front end (fbank.hip: launch_fbank_batch; what S3ENC_DECOAR2 runs): ONE overlapping-row GEMM over
 * the padded batch, one power -> mel -> log launch, one CMVN launch with per-utterance counts.  cfg: delta_order 0 and use_cmvn 1 (the
 * rest is refused by name).  pcm: DEVICE (B, row_stride) fp32, 16-byte aligned, row_stride a multiple of 4 and >= n_max; whatever stands
 * behind an utterance's own samples is never part of a valid row.  lengths: HOST [B] samples, each at least one analysis window;
 * n_max: the batch's padded length (0: the longest utterance).  out: DEVICE (B, Fmax, num_mel_bins), Fmax =
 * s3enc_fbank_num_frames(n_max): rows [0, F_b) of utterance b are bit for bit what s3enc_fbank_forward_ex gives for it alone, rows
 * [F_b, Fmax) are exactly 0 (written by the last kernel, no memset in front).  spec_cap_bytes: the cap on the spectrum workspace (2 x 257
 * floats per frame); 0: the default 128 MiB.  A batch above it is walked in chunks of whole utterances.  Synchronises. */
int s3enc_op_fbank_batch(const s3enc_fbank_config* cfg, int32_t window, const float* pcm, int64_t row_stride, const int64_t* lengths,
                         int32_t B, int64_t n_max, float* out, int64_t spec_cap_bytes, int32_t device, void* stream);


/* ---- the OnlinePreprocessor log-mel front end (Mockingjay / TERA / AudioALBERT, upstream/baseline/preprocessor.py) ----
 * counts[b] = round(lengths[b] / (n_max / T)) with T = 1 + n_max / 160, in doubles, halves to even (Python's round): the frames
 * the reference's CMVN runs over.  n_max = 0: the longest length.  Host only. */
int s3enc_logmel_frame_counts(const int64_t* lengths, int32_t B, int64_t n_max, int32_t* counts);
/* wavs: host array of B device pointers; out: device fp32 (B, T, n_mels) with T = 1 + n_max / 160 (n_max = 0: the longest
 * length; it must exceed 200 samples, like every utterance).  Per utterance x * 10^(target_level / 20) / (rms + 1e-10), the
 * batch zero-padded to n_max, centred periodic-hann STFT (400 / 160, reflect) of the PADDED rows, |X|^2, HTK mel, log(x + 1e-10);
 * with cmvn: per mel bin over counts[b] frames (HOST int32, each >= 2), rows behind are zeros.  Synchronises. */
int s3enc_logmel_forward(const float* const* wavs, const int64_t* lengths, int32_t B, int64_t n_max, int32_t n_mels,
                         float target_level, int32_t cmvn, const int32_t* counts, float* out, int32_t device, void* stream);
/* TF-style LayerNorm with a run-time eps: y = (x - mean) / sqrt(var + eps) * gamma + beta over rows of C fp32 (C % 4 == 0,
 * C <= 2048; biased variance).  Asynchronous on `stream`. */
int s3enc_op_layernorm_eps(const float* x, const float* gamma, const float* beta, float eps, int64_t rows, int32_t C, float* out,
                           void* stream);
/* The family's input representation: out[r] = LayerNorm_eps(feat[r] W^T + bias + pos[r % Tc]) for `rows` rows; feat: device
 * (rows, F), W: device (D, F), pos_host: HOST (>= Tc, D) position rows (uploaded inside).  F % 4 == 0, D % 4 == 0.  Synchronises. */
int s3enc_op_input_repr(const float* feat, const float* w, const float* bias, const float* pos_host, int32_t Tc, const float* gamma,
                        const float* beta, float eps, int64_t rows, int32_t F, int32_t D, float* out, void* stream);

/* ---- the plain signal features: `spectrogram`, `mfcc`, `mel`, `linear` (upstream/baseline) and `stft_mag` (upstream/log_stft) ----
 * Exact fp32 at 16 kHz.  kind:
 *   S3ENC_SPECTRAL_SPECTROGRAM  torchaudio.compliance.kaldi.spectrogram (snip_edges, mean removal, pre-emphasis, povey window,
 *       zero-padded to the next power of two): log(max(|X|^2, eps32)) over bins 0 .. n/2, bin 0 replaced by the frame's raw log
 *       energy floored at log(1) = 0 -> deltas -> CMVN                                               (extracter.py:32-90)
 *   S3ENC_SPECTRAL_MFCC         kaldi.mfcc: the fbank log-mel at num_mel_bins (23), the orthonormal DCT-II's first num_ceps
 *       columns (column 0 sqrt(1 / num_mel_bins)), the lifter 1 + 0.5 Q sin(pi i / Q) -> deltas -> CMVN
 *   S3ENC_SPECTRAL_LINEAR / _MEL  the OnlinePreprocessor without a level normalisation (preprocessor.py:150-223, expert.py:55-67):
 *       T = 1 + max length / 160 centred reflect hann frames (400 / 160) of the zero-PADDED batch rows, log(|X|^2 + 1e-10) of the
 *       201 bins or of num_mel_bins HTK triangles.  With CMVN: over round(L' / (max length / T)) frames, L' = 1 + the index of the
 *       utterance's last NON-ZERO sample (an all-zero one: max length), zeros behind, and the batch cut to the largest such count,
 *       R (the reference's re-padding to max L' slices the channel axis and changes nothing); without: R = T.  Then
 *       min(round(length * (R / lengths[0])), R) rows are kept (Python's rounding both times)
 *   S3ENC_SPECTRAL_STFT_MAG     per utterance torch.stft(n_fft, hop, win, periodic hann, center, reflect): |X| (not the power),
 *       with log: log(max(|X|, 1e-8)); 1 + n / hop frames; an utterance of n_fft / 2 samples or fewer is refused
 * Fields a kind does not read are ignored.  CMVN: per column over time, unbiased std, cmvn_eps added to the std. */
#define S3ENC_SPECTRAL_SPECTROGRAM 0
#define S3ENC_SPECTRAL_MFCC 1
#define S3ENC_SPECTRAL_LINEAR 2
#define S3ENC_SPECTRAL_MEL 3
#define S3ENC_SPECTRAL_STFT_MAG 4
typedef struct s3enc_spectral_config {
    int32_t kind;
    int32_t sample_rate;      /* 16000 */
    float frame_length_ms;    /* kaldi kinds: 25 */
    float frame_shift_ms;     /* kaldi kinds: 10 */
    float preemphasis;        /* kaldi kinds: 0.97 */
    int32_t num_mel_bins;     /* mfcc: 23 (kaldi bank); mel: 80 (HTK bank) */
    int32_t num_ceps;         /* mfcc: 13, <= num_mel_bins */
    float cepstral_lifter;    /* mfcc: 22; 0 = none */
    int32_t delta_order;      /* kaldi kinds: 0..2 (spectrogram.yaml 0, mfcc.yaml 2) */
    int32_t delta_win_length; /* 5 */
    int32_t use_cmvn;
    float cmvn_eps;           /* 1e-10 */
    int32_t log;              /* stft_mag: 0 / 1; linear and mel: 1 */
    int32_t n_fft;            /* stft_mag: 512 (a multiple of 4); linear and mel: 400 */
    int32_t hop;              /* stft_mag: 320 (a multiple of 4); linear and mel: 160 */
    int32_t win;              /* stft_mag: 512 (<= n_fft, centred in it); linear and mel: 400 */
} s3enc_spectral_config;
/* frames[b] (HOST, B values) = the rows utterance b occupies in the output of the forward below; the output needs T_max >= the
 * largest.  The kaldi kinds and stft_mag read the lengths only (wavs may be null, no device is touched) and return 0 frames for
 * an utterance under one window (stft_mag: n_fft / 2 samples or fewer); linear and mel run the last-non-zero reduction over the
 * device waveforms on `stream` and synchronise it. */
int s3enc_spectral_num_frames(const s3enc_spectral_config* cfg, const float* const* wavs, const int64_t* lengths, int32_t B,
                              int32_t* frames, int32_t device, void* stream);
/* wavs: host array of B device pointers (borrowed, 4-byte alignment suffices); out: device fp32 (B, T_max, F), zero behind each
 * utterance's rows; F = (padded window / 2 + 1) x (delta_order + 1), num_ceps x (delta_order + 1), 201, num_mel_bins, n_fft / 2 + 1.
 * One frame under CMVN is NaN, as in the reference.  The kaldi kinds and stft_mag are asynchronous on `stream`; linear and mel
 * synchronise it (the frame count depends on the samples). */
int s3enc_spectral_forward(const s3enc_spectral_config* cfg, const float* const* wavs, const int64_t* lengths, int32_t B, float* out,
                           int64_t T_max, int32_t device, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* S3ENC_H */
