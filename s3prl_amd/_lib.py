"""ctypes binding of ``libs3enc.so`` (C ABI declared in ``include/s3enc.h``).

The library is built in-tree by ``__graft_entry__.build()`` / ``make -C s3prl_amd/csrc``.  There is no
fallback: if it is missing, or no gfx950 GPU is visible at ``s3enc_create`` time, we raise.
"""

from __future__ import annotations

import ctypes as C
import os
from typing import Callable, NamedTuple

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libs3enc.so")

S3ENC_MAX_CONV = 16
S3ENC_MAX_RES = 4
F32, BF16, F16, F32X3, F16X2 = 0, 1, 2, 3, 4
STATUS_NONFINITE, STATUS_PENDING = 1, 1 << 30  # s3enc_forward_status bits (include/s3enc.h)
DTYPES = {"fp32": F32, "f32": F32, "float32": F32, "bf16": BF16, "bfloat16": BF16, "fp16": F16, "f16": F16,
          "float16": F16, "fp32x3": F32X3, "f32x3": F32X3, "bf16x3": F32X3,
          "fp16x2": F16X2, "f16x2": F16X2}
FAMILY = {"hubert": 0, "wav2vec2": 1, "wavlm": 2, "distiller": 3, "multires_hubert": 4, "wav2vec": 5, "cpc": 6, "apc": 7, "mockingjay": 8, "decoar": 9, "npc": 10, "vggish": 11, "byol_a": 12, "mae_ast": 13, "byol_s": 14, "lighthubert": 15, "decoar2": 16, "ssast": 18}
CPC_NORM = {"layerNorm": 0, "instanceNorm": 1, "ID": 2, "batchNorm": 3}            # s3enc_cpc_config.norm_mode
CPC_AR = {"LSTM": 0, "GRU": 1, "RNN": 2, "transformer": 3, "no_ar": 4}             # s3enc_cpc_config.ar_mode
APC_WINDOW = {"povey": 0, "hamming": 1}                                            # s3enc_apc_config.window
VQ_TYPE = {"none": 0, "gumbel": 1, "kmeans": 2}  # s3enc_config.vq_type
SEL_HIDDEN, SEL_LAYER_OUT, SEL_FFN_OUT = 0, 1, 2
SELECTIONS = {None: SEL_HIDDEN, "hidden_states": SEL_HIDDEN, "fairseq_layers": SEL_LAYER_OUT,
              "fairseq_layers_before_residual": SEL_FFN_OUT}
ABI_VERSION = 8
POS_ENC = {"rel_pos": 1, "rope": 2}  # s3enc_config.pos_enc_type of a Conformer encoder
EXCHANGE_COLLECTIVE, EXCHANGE_DIRECT, EXCHANGE_COPY = 0, 1, 2   # S3ENC_EXCHANGE_*
COPY_HANDLE_BYTES = 256                                         # S3ENC_COPY_HANDLE_BYTES


class S3Config(C.Structure):
    _fields_ = [
        ("family", C.c_int32), ("n_conv", C.c_int32), ("conv_dim", C.c_int32),
        ("conv_kernel", C.c_int32 * S3ENC_MAX_CONV), ("conv_stride", C.c_int32 * S3ENC_MAX_CONV),
        ("extractor_layer_norm", C.c_int32), ("conv_bias", C.c_int32), ("encoder_layers", C.c_int32),
        ("embed_dim", C.c_int32), ("ffn_dim", C.c_int32), ("heads", C.c_int32), ("layer_norm_first", C.c_int32),
        ("conv_pos", C.c_int32), ("conv_pos_groups", C.c_int32), ("normalize", C.c_int32), ("rel_pos", C.c_int32),
        ("num_buckets", C.c_int32), ("max_distance", C.c_int32), ("gru_rel_pos", C.c_int32),
        ("compute_dtype", C.c_int32), ("no_feature_layer_norm", C.c_int32), ("pos_conv_depth", C.c_int32), ("wav_norm_eps", C.c_float), ("pred_heads", C.c_int32),
        ("mr_pairs", C.c_int32), ("mr_ratios", C.c_int32 * (2 * (S3ENC_MAX_RES - 1))),
        ("mr_layers", C.c_int32 * (2 * S3ENC_MAX_RES - 1)), ("mr_kernel", C.c_int32), ("mr_plain", C.c_int32),
        ("layer_type", C.c_int32), ("pos_enc_type", C.c_int32), ("dw_kernel", C.c_int32),
    ]


class S3Wav2vecConfig(C.Structure):
    """s3enc_wav2vec_config: the aggregator / quantizer block of a wav2vec handle (s3enc_create_ex)."""
    _fields_ = [
        ("n_agg", C.c_int32), ("agg_dim", C.c_int32 * S3ENC_MAX_CONV), ("agg_kernel", C.c_int32 * S3ENC_MAX_CONV),
        ("agg_stride", C.c_int32 * S3ENC_MAX_CONV), ("w2v_aggregator", C.c_int32), ("w2v_activation", C.c_int32),
        ("w2v_skip_feat", C.c_int32), ("log_compression", C.c_int32), ("skip_connections_agg", C.c_int32),
        ("residual_scale", C.c_float), ("non_affine_group_norm", C.c_int32), ("no_conv_bias", C.c_int32),
        ("agg_zero_pad", C.c_int32), ("vq_type", C.c_int32), ("vq_vars", C.c_int32), ("vq_groups", C.c_int32),
        ("vq_dim", C.c_int32), ("vq_depth", C.c_int32), ("combine_groups", C.c_int32),
    ]


class S3CpcConfig(C.Structure):
    """s3enc_cpc_config: the padding / recurrent-network block of a modified-CPC handle (s3enc_create_cpc)."""
    _fields_ = [
        ("conv_pad", C.c_int32 * S3ENC_MAX_CONV), ("norm_mode", C.c_int32), ("ar_mode", C.c_int32), ("ar_layers", C.c_int32),
        ("ar_hidden", C.c_int32), ("reverse", C.c_int32), ("keep_hidden", C.c_int32),
    ]


class S3ApcConfig(C.Structure):
    """s3enc_apc_config: the front-end / GRU block of an APC handle (s3enc_create_apc)."""
    _fields_ = [
        ("num_mel_bins", C.c_int32), ("frame_length_ms", C.c_float), ("frame_shift_ms", C.c_float), ("window", C.c_int32),
        ("cmvn", C.c_int32), ("hidden", C.c_int32), ("num_layers", C.c_int32), ("residual", C.c_int32),
    ]


class S3MockingjayConfig(C.Structure):
    """s3enc_mockingjay_config: the front-end / input-representation block of a Mockingjay handle (s3enc_create_mockingjay)."""
    _fields_ = [
        ("input_dim", C.c_int32), ("layer_norm_eps", C.c_float), ("share_layer", C.c_int32), ("sequence_length", C.c_int32),
        ("frontend", C.c_int32), ("n_mels", C.c_int32), ("target_level", C.c_float), ("cmvn", C.c_int32),
        ("pre_layer_norm", C.c_int32), ("hidden_act", C.c_int32),
        ("fbank_num_mel_bins", C.c_int32), ("fbank_frame_length_ms", C.c_float), ("fbank_frame_shift_ms", C.c_float),
        ("fbank_preemphasis", C.c_float), ("fbank_delta_order", C.c_int32), ("fbank_delta_win_length", C.c_int32),
        ("fbank_use_cmvn", C.c_int32), ("fbank_cmvn_eps", C.c_float),
    ]


class S3DecoarConfig(C.Structure):
    """s3enc_decoar_config: the front-end / LSTM block of a DeCoAR handle (s3enc_create_decoar)."""
    _fields_ = [
        ("num_mel_bins", C.c_int32), ("hidden", C.c_int32), ("num_layers", C.c_int32), ("frame_length_ms", C.c_float),
        ("frame_shift_ms", C.c_float), ("subsample", C.c_int32), ("per_layer_states", C.c_int32),
    ]


class S3NpcConfig(C.Structure):
    """s3enc_npc_config: the front-end / convolution block of an NPC handle (s3enc_create_npc)."""
    _fields_ = [
        ("num_mel_bins", C.c_int32), ("frame_length_ms", C.c_float), ("frame_shift_ms", C.c_float), ("window", C.c_int32),
        ("cmvn", C.c_int32), ("hidden", C.c_int32), ("n_blocks", C.c_int32), ("kernel_size", C.c_int32), ("mask_size", C.c_int32),
        ("residual", C.c_int32), ("batch_norm", C.c_int32), ("activate", C.c_int32), ("disable_cross_layer", C.c_int32),
        ("dim_bottleneck", C.c_int32),
    ]


S3ENC_VGGISH_MAX_LAYERS = 8


class S3VggishConfig(C.Structure):
    """s3enc_vggish_config: the front-end / layer block of a VGGish handle (s3enc_create_vggish)."""
    _fields_ = [
        ("num_mel_bins", C.c_int32), ("window", C.c_int32), ("shift", C.c_int32), ("n_fft", C.c_int32), ("mel_min_hz", C.c_float),
        ("mel_max_hz", C.c_float), ("log_offset", C.c_float), ("example_frames", C.c_int32), ("example_hop", C.c_int32),
        ("n_layers", C.c_int32), ("channels", C.c_int32 * S3ENC_VGGISH_MAX_LAYERS), ("pool_after", C.c_int32 * S3ENC_VGGISH_MAX_LAYERS),
        ("fc", C.c_int32 * 3), ("postprocess", C.c_int32), ("quant_min", C.c_float), ("quant_max", C.c_float),
    ]


class S3ByolAConfig(C.Structure):
    """s3enc_byol_a_config: the segment block of a BYOL-A handle (s3enc_create_byol_a)."""
    _fields_ = [("feature_d", C.c_int32), ("window", C.c_int32), ("stride", C.c_int32), ("norm_mean", C.c_float),
                ("norm_std", C.c_float), ("bn_eps", C.c_float)]


class S3MaeAstConfig(C.Structure):
    """s3enc_mae_ast_config: the patch / BatchNorm block of an MAE-AST handle (s3enc_create_mae_ast)."""
    _fields_ = [("kt", C.c_int32), ("kc", C.c_int32), ("feature_dim", C.c_int32), ("bn_mean", C.c_float), ("bn_var", C.c_float),
                ("bn_eps", C.c_float), ("pos_rows", C.c_int32)]


class S3SsastConfig(C.Structure):
    """s3enc_ssast_config: the window / patch block of an SSAST handle (s3enc_create_ssast)."""
    _fields_ = [("fshape", C.c_int32), ("tshape", C.c_int32), ("fstride", C.c_int32), ("tstride", C.c_int32),
                ("window_samples", C.c_int32), ("target_length", C.c_int32), ("ln_eps", C.c_float), ("pos_rows", C.c_int32)]


BYOL_S_NETWORK = {"default": 0, "resnetish": 1, "cvt": 2, "clstm": 3}          # s3enc_byol_s_config.network


class S3ByolSConfig(C.Structure):
    """s3enc_byol_s_config: the window / network block of a BYOL-S handle (s3enc_create_byol_s)."""
    _fields_ = [("network", C.c_int32), ("blocks", C.c_int32 * 4), ("bottleneck", C.c_int32), ("window", C.c_int32),
                ("step", C.c_int32), ("bn_eps", C.c_float)]


class S3ForwardOpts(C.Structure):
    _fields_ = [("selection", C.c_int32), ("out_dtype", C.c_int32), ("featurize", C.c_int32),
                ("feat_normalize", C.c_int32), ("feat_w", C.POINTER(C.c_float))]


class S3Tensor(C.Structure):
    _fields_ = [("name", C.c_char_p), ("data", C.POINTER(C.c_float)), ("ndim", C.c_int32), ("shape", C.c_int64 * 4)]


class S3ProfileEntry(C.Structure):
    _fields_ = [("name", C.c_char * 48), ("launches", C.c_int64), ("ms", C.c_double), ("flops", C.c_double),
                ("bytes", C.c_double)]


class S3FbankConfig(C.Structure):
    _fields_ = [("sample_rate", C.c_int32), ("num_mel_bins", C.c_int32), ("frame_length_ms", C.c_float),
                ("frame_shift_ms", C.c_float), ("preemphasis", C.c_float), ("delta_order", C.c_int32),
                ("delta_win_length", C.c_int32), ("use_cmvn", C.c_int32), ("cmvn_eps", C.c_float)]


SPECTRAL_KINDS = {"spectrogram": 0, "mfcc": 1, "linear": 2, "mel": 3, "stft_mag": 4}  # S3ENC_SPECTRAL_*


class S3SpectralConfig(C.Structure):
    _fields_ = [("kind", C.c_int32), ("sample_rate", C.c_int32), ("frame_length_ms", C.c_float), ("frame_shift_ms", C.c_float),
                ("preemphasis", C.c_float), ("num_mel_bins", C.c_int32), ("num_ceps", C.c_int32), ("cepstral_lifter", C.c_float),
                ("delta_order", C.c_int32), ("delta_win_length", C.c_int32), ("use_cmvn", C.c_int32), ("cmvn_eps", C.c_float),
                ("log", C.c_int32), ("n_fft", C.c_int32), ("hop", C.c_int32), ("win", C.c_int32)]


# every symbol include/s3enc.h declares: (restype, argtypes)
_VP, _I32, _I64 = C.c_void_p, C.c_int32, C.c_int64
_PROTOS = {
    "s3enc_version": (C.c_int, []),
    "s3enc_last_error": (C.c_char_p, []),
    "s3enc_create": (C.c_int, [C.POINTER(S3Config), C.POINTER(S3Tensor), _I32, _I32, C.POINTER(_VP)]),
    # (s3enc_create_ex and the later s3enc_create_*: one per entry of BLOCK_FAMILIES, added below it)
    "s3enc_destroy": (C.c_int, [_VP]),
    "s3enc_num_frames": (C.c_int, [_VP, _I64, C.POINTER(_I32)]),
    "s3enc_num_output_frames": (C.c_int, [_VP, _I64, C.POINTER(_I32)]),
    "s3enc_downsample_rate": (C.c_int, [_VP, C.POINTER(_I32)]),
    "s3enc_valid_frames": (C.c_int, [_VP, _I64, _I64, C.POINTER(_I32)]),
    "s3enc_forward": (C.c_int, [_VP, C.POINTER(_VP), C.POINTER(_I64), _I32, _I64, _VP, _I64, _VP]),
    "s3enc_forward_status": (C.c_int, [_VP, _I32, C.POINTER(_I32)]),
    "s3enc_forward_ex": (C.c_int, [_VP, C.POINTER(_VP), C.POINTER(_I64), _I32, _I64, C.POINTER(S3ForwardOpts), _VP, _I64, _VP]),
    "s3enc_forward_aux": (C.c_int, [_VP, C.POINTER(_VP), C.POINTER(_I64), _I32, _I64, C.POINTER(S3ForwardOpts), _VP, _I64, _VP, _VP, _VP]),
    "s3enc_num_states": (C.c_int, [_VP, _I32, C.POINTER(_I32)]),
    "s3enc_forward_padded": (C.c_int, [_VP, _VP, _I64, C.POINTER(_I64), _I32, _I64, _VP, _I64, _VP]),
    "s3enc_set_layer_events": (C.c_int, [_VP, C.POINTER(_VP), _I32]),
    "s3enc_profile_enable": (C.c_int, [_VP, _I32]),
    "s3enc_profile_reset": (C.c_int, [_VP]),
    "s3enc_profile_read": (C.c_int, [_VP, C.POINTER(S3ProfileEntry), _I32, C.POINTER(_I32)]),
    "s3enc_debug_tap": (C.c_int, [_VP, C.c_char_p, C.POINTER(C.c_float), _I64, C.POINTER(_I64)]),
    "s3enc_comm_version": (C.c_int, [C.POINTER(_I32)]),
    "s3enc_comm_unique_id": (C.c_int, [_VP]),
    "s3enc_comm_init_rank": (C.c_int, [_VP, _I32, _I32, _I32, C.POINTER(_VP)]),
    "s3enc_comm_info": (C.c_int, [_VP, C.POINTER(_I32), C.POINTER(_I32)]),
    "s3enc_comm_allgather_states": (C.c_int, [_VP, _VP, _I64, _VP, _I64, _I32, _I64, C.POINTER(_VP), _VP]),
    "s3enc_comm_exchange_states": (C.c_int, [_VP, _I32, _VP, _I64, _VP, _I64, _I32, _I64, C.POINTER(_VP), _VP]),
    "s3enc_comm_destroy": (C.c_int, [_VP]),
    "s3enc_comm_init_local": (C.c_int, [_I32, _I32, _I32, C.POINTER(_VP)]),
    "s3enc_comm_copy_export": (C.c_int, [_VP, _VP, _I64, _VP]),
    "s3enc_comm_copy_attach": (C.c_int, [_VP, _VP]),
    "s3enc_comm_copy_status": (C.c_int, [_VP, C.POINTER(_I32)]),
    "s3enc_comm_copy_release": (C.c_int, [_VP, _VP]),
    "s3enc_set_handle_tuning": (C.c_int, [_VP, C.c_char_p, _I32]),
    "s3enc_set_tuning": (C.c_int, [C.c_char_p, _I32]),
    "s3enc_op_gemm": (C.c_int, [_I32, _VP, _I64, _I64, _VP, _VP, _I32, _I32, _I32, _I32, _I32, _VP, _VP, _VP, _VP,
                                _I64, _I64, _VP]),
    "s3enc_debug_occupy_cus": (C.c_int, [_I32, _I32, C.c_double, _VP]),
    "s3enc_debug_clock_sample": (C.c_int, [_VP, _VP]),
    "s3enc_debug_gemm_schedule": (C.c_int, [_I32, _I32, _I32, _I32, _I32, _I32, _VP, _I64, C.POINTER(_I64)]),
    "s3enc_op_layernorm": (C.c_int, [_I32, _VP, _VP, _VP, _I32, _I32, _I32, _VP, _VP, _VP]),
    "s3enc_op_attention": (C.c_int, [_I32, _VP, _VP, _VP, _I32, _I32, _I32, _VP, _I32, _VP, _VP]),
    "s3enc_op_conv0": (C.c_int, [_I32, C.POINTER(_VP), C.POINTER(_I64), _I32, _I64, _I32, _VP, _VP, _VP, _VP, _VP, _VP, _I32,
                                 _I32, _VP, _VP]),
    "s3enc_op_wavlm_gate": (C.c_int, [_VP, _VP, _VP, _VP, _I32, _I32, _I32, _VP, _VP]),
    "s3enc_op_conformer_conv": (C.c_int, [_VP, _VP, _VP, _I32, _I32, _I32, _I32, _VP, _VP]),
    "s3enc_op_gn1_apply": (C.c_int, [_VP, _VP, _VP, _VP, C.c_float, _I32, _I32, _I32, _I32, _I32, _I32, _VP, _VP, _VP, C.c_float,
                                     _I32, _I32, _VP]),
    "s3enc_op_channelnorm_relu": (C.c_int, [_VP, _VP, _VP, _I32, _I32, _I32, _I32, _VP, _VP, _VP]),
    "s3enc_op_rnn": (C.c_int, [_I32, _VP, _VP, _VP, _I32, _I32, _I32, _I64, _VP, _I64, _VP]),
    "s3enc_op_rnn_len": (C.c_int, [_I32, _VP, _VP, _VP, _VP, _VP, _I64, _I32, _I32, _I32, _I64, _VP, _I64, _VP]),
    "s3enc_op_lstm_bidir": (C.c_int, [_VP, _VP, _VP, _VP, _VP, _I32, _I32, _I32, _I64, _VP, _I64, _VP]),
    "s3enc_pack_lstm_bidir_whh": (C.c_int, [_VP, _I32, _VP]),
    "s3enc_op_conv_taps": (C.c_int, [_VP, _VP, _VP, _I32, _I32, _I32, _I32, _I32, _I32, _I32, _VP, _I64, _VP, _I32, _I64, _VP, _VP,
                                     _I32, _I32, _VP]),
    "s3enc_op_conv_k3s2": (C.c_int, [_VP, _I64, _VP, _VP, _VP, _I32, _I32, _I32, _I32, _VP, _I64, _VP]),
    "s3enc_op_conv2d3x3": (C.c_int, [_VP, _VP, _VP, _I32, _I32, _I32, _I32, _I32, _I32, _I32, _VP, _I32, _I64, _VP]),
    "s3enc_op_conv2d3x3_affine": (C.c_int, [_VP, _VP, _VP, _VP, _VP, _I32, _I32, _I32, _I32, _I32, _I32, _I32, _I32, _VP, _I32, _I64, _VP]),
    "s3enc_op_melspec1024": (C.c_int, [_VP, _I32, _I32, _VP, _VP, _VP]),
    "s3enc_op_melspec400": (C.c_int, [_VP, _I32, _I32, _VP, _VP, _VP]),
    "s3enc_op_conv2d_res": (C.c_int, [_VP, _VP, _VP, _VP, _VP, _VP, _I32, _I32, _I32, _I32, _I32, _I32, _I32, _I32, _VP, _I32, _I64, _VP]),
    "s3enc_op_stem7x7_pool": (C.c_int, [_VP, _VP, _VP, _VP, _I32, _I32, _I32, _VP, _VP, _VP]),
    "s3enc_op_patch_embed": (C.c_int, [_VP, _I64, _VP, _VP, _VP, _VP, _I32, _I32, _I32, _I32, _I32, _VP, _VP]),
    "s3enc_op_patch_embed_strided": (C.c_int, [_VP, _I64, _VP, _VP, _VP, _VP, _I32, _I32, _I32, _I32, _I32, _I32, _I32, _I32, _VP, _VP]),
    "s3enc_op_argmax_gather": (C.c_int, [_VP, _VP, _I32, _I64, _I32, _I32, _I32, _VP, _VP, _VP]),
    "s3enc_op_relpos_attention": (C.c_int, [_VP, _VP, _VP, _I32, _I32, _I32, _VP, _VP, _VP]),
    "s3enc_op_posconv": (C.c_int, [_I32, _VP, _VP, _VP, _I32, _I32, _I32, _I32, _I32, _VP, _VP]),
    "s3enc_op_posconv_narrow": (C.c_int, [_I32, _VP, _VP, _VP, _I32, _I32, _I32, _I32, _I32, _VP, _VP]),
    "s3enc_weighted_sum": (C.c_int, [_VP, _I64, _I32, C.POINTER(C.c_float), _I32, _I64, _I32, _VP, _VP]),
    "s3enc_weighted_sum_backward_scratch": (_I64, [_I64, _I32]),
    "s3enc_weighted_sum_backward": (C.c_int, [_VP, _I64, _I32, _I32, _I64, _I32, _VP, _VP, _VP, _VP]),
    "s3enc_fbank_num_frames": (C.c_int, [C.POINTER(S3FbankConfig), _I64, C.POINTER(_I32)]),
    "s3enc_fbank_forward": (C.c_int, [C.POINTER(S3FbankConfig), _VP, C.POINTER(_I64), _I32, _VP, _I64, _I32, _VP]),
    "s3enc_fbank_forward_ex": (C.c_int, [C.POINTER(S3FbankConfig), _I32, _VP, C.POINTER(_I64), _I32, _VP, _I64, _I32, _VP]),
    "s3enc_op_fbank_batch": (C.c_int, [C.POINTER(S3FbankConfig), _I32, _VP, _I64, C.POINTER(_I64), _I32, _I64, _VP, _I64, _I32, _VP]),
    "s3enc_spectral_num_frames": (C.c_int, [C.POINTER(S3SpectralConfig), _VP, C.POINTER(_I64), _I32, C.POINTER(_I32), _I32, _VP]),
    "s3enc_spectral_forward": (C.c_int, [C.POINTER(S3SpectralConfig), _VP, C.POINTER(_I64), _I32, _VP, _I64, _I32, _VP]),
    "s3enc_logmel_frame_counts": (C.c_int, [C.POINTER(_I64), _I32, _I64, C.POINTER(_I32)]),
    "s3enc_logmel_forward": (C.c_int, [_VP, C.POINTER(_I64), _I32, _I64, _I32, C.c_float, _I32, C.POINTER(_I32), _VP, _I32, _VP]),
    "s3enc_op_layernorm_eps": (C.c_int, [_VP, _VP, _VP, C.c_float, _I64, _I32, _VP, _VP]),
    "s3enc_op_input_repr": (C.c_int, [_VP, _VP, _VP, _VP, _I32, _VP, _VP, C.c_float, _I64, _I32, _I32, _VP, _VP]),
}

_lib = None


class S3EncError(RuntimeError):
    pass


def load():
    """Load libs3enc.so (once).  ``import torch`` first so that the HIP runtime torch ships is the one
    the library binds to (same SONAME libamdhip64.so.7) and device pointers are interchangeable."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise S3EncError(
            f"{LIB_PATH} not found — build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            f"or `make -C s3prl_amd/csrc`.  There is no CPU / PyTorch fallback for the encoder path."
        )
    try:
        import torch  # noqa: F401  (loads libamdhip64 first)
    except Exception:  # pragma: no cover - torch is only plumbing
        pass
    lib = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    for name, (res, args) in _PROTOS.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    if lib.s3enc_version() != ABI_VERSION:
        raise S3EncError(f"{LIB_PATH} has ABI version {lib.s3enc_version()}, this package needs {ABI_VERSION}: rebuild it")
    _lib = lib
    return lib


def check(rc: int, what: str = "libs3enc"):
    if rc != 0:
        msg = load().s3enc_last_error()
        raise S3EncError(f"{what}: {msg.decode() if msg else 'unknown error'}")


def make_config(cfg, dtype: str) -> S3Config:
    """EncoderConfig → C struct."""
    c = S3Config()
    c.family = FAMILY[cfg.family]
    if len(cfg.conv_layers) > S3ENC_MAX_CONV:
        raise S3EncError("too many conv layers")
    c.n_conv = len(cfg.conv_layers)
    c.conv_dim = cfg.conv_dim
    for i, (_, k, s) in enumerate(cfg.conv_layers):
        c.conv_kernel[i] = k
        c.conv_stride[i] = s
    c.extractor_layer_norm = int(cfg.extractor_mode == "layer_norm")
    c.conv_bias = int(cfg.conv_bias)
    c.encoder_layers = cfg.encoder_layers
    c.embed_dim = cfg.encoder_embed_dim
    c.ffn_dim = cfg.encoder_ffn_embed_dim
    c.heads = cfg.encoder_attention_heads
    c.layer_norm_first = int(cfg.layer_norm_first)
    c.conv_pos = cfg.conv_pos
    c.conv_pos_groups = cfg.conv_pos_groups
    c.normalize = int(cfg.normalize)
    c.rel_pos = int(cfg.family == "wavlm" and cfg.relative_position_embedding)
    c.num_buckets = cfg.num_buckets
    c.max_distance = cfg.max_distance
    c.gru_rel_pos = int(cfg.gru_rel_pos)
    if dtype not in DTYPES:
        raise S3EncError(f"unknown dtype {dtype!r}; use one of fp32 / bf16 / fp16")
    c.compute_dtype = DTYPES[dtype]
    if DTYPES[dtype] != F32:  # s3enc_create refuses both with these messages too
        if cfg.family == "lighthubert":
            raise S3EncError(f"LightHuBERT is built for compute dtype fp32 only; {dtype} is not built")
        if cfg.layer_type != "conformer" and cfg.encoder_embed_dim // cfg.conv_pos_groups in (24, 40):
            raise S3EncError(f"the positional conv at group width {cfg.encoder_embed_dim // cfg.conv_pos_groups} is built for compute "
                             f"dtype fp32 only; {dtype} is not built")
    c.no_feature_layer_norm = int(not cfg.feature_layer_norm)
    c.pos_conv_depth = int(cfg.pos_conv_depth)
    c.wav_norm_eps = float(cfg.wav_norm_eps)
    c.pred_heads = int(cfg.pred_heads)
    if cfg.layer_type == "conformer":
        c.layer_type = 1
        c.pos_enc_type = POS_ENC[cfg.pos_enc_type]
        c.dw_kernel = int(cfg.depthwise_conv_kernel_size)
    if cfg.family == "multires_hubert":
        pairs = cfg.rate_pairs
        if len(pairs) > S3ENC_MAX_RES - 1:
            raise S3EncError("too many resolutions")
        c.mr_pairs = len(pairs)
        for i, r in enumerate(cfg.label_rate_ratios):
            c.mr_ratios[i] = int(r)
        for i, n in enumerate(cfg.block_layers):
            c.mr_layers[i] = int(n)
        c.mr_kernel = int(cfg.conv_adapter_kernel)
        c.mr_plain = int(cfg.use_plain_updownsample)
    return c


def make_wav2vec_config(cfg) -> S3Wav2vecConfig:
    """The second configuration block of a ``family="wav2vec"`` EncoderConfig (``s3enc_create_ex``)."""
    if cfg.family != "wav2vec":
        raise S3EncError("make_wav2vec_config needs a wav2vec configuration")
    c = S3Wav2vecConfig()
    if len(cfg.agg_layers) > S3ENC_MAX_CONV:
        raise S3EncError("too many aggregator layers")
    c.n_agg = len(cfg.agg_layers)
    for i, (d, k, s) in enumerate(cfg.agg_layers):
        c.agg_dim[i], c.agg_kernel[i], c.agg_stride[i] = d, k, s
    c.w2v_aggregator = int(cfg.aggregator != "cnn")
    c.w2v_activation = int(cfg.activation != "relu")
    c.w2v_skip_feat = int(cfg.skip_connections_feat)
    c.log_compression = int(cfg.log_compression)
    c.skip_connections_agg = int(cfg.skip_connections_agg)
    c.residual_scale = float(cfg.residual_scale)
    c.non_affine_group_norm = int(cfg.non_affine_group_norm)
    c.no_conv_bias = int(cfg.no_conv_bias)
    c.agg_zero_pad = int(cfg.agg_zero_pad)
    c.vq_type = VQ_TYPE[cfg.vq_type]
    c.vq_vars, c.vq_groups, c.vq_depth = int(cfg.vq_vars), int(cfg.vq_groups), int(cfg.vq_depth)
    c.vq_dim = int(cfg.vq_dim) or cfg.conv_dim
    c.combine_groups = int(cfg.combine_groups)
    return c


def make_cpc_config(cfg) -> S3CpcConfig:
    """The second configuration block of a ``family="cpc"`` EncoderConfig (``s3enc_create_cpc``)."""
    if cfg.family != "cpc":
        raise S3EncError("make_cpc_config needs a cpc configuration")
    c = S3CpcConfig()
    if len(cfg.conv_pads) > S3ENC_MAX_CONV:
        raise S3EncError("too many conv layers")
    for i, p in enumerate(cfg.conv_pads):
        c.conv_pad[i] = int(p)
    c.norm_mode = CPC_NORM.get(cfg.norm_mode, -1)
    c.ar_mode = CPC_AR.get(cfg.ar_mode, -1)
    c.ar_layers, c.ar_hidden = int(cfg.ar_layers), int(cfg.ar_hidden)
    c.reverse, c.keep_hidden = int(cfg.cpc_reverse), int(cfg.cpc_keep_hidden)
    return c


def make_apc_config(cfg) -> S3ApcConfig:
    """The second configuration block of a ``family="apc"`` EncoderConfig (``s3enc_create_apc``)."""
    if cfg.family != "apc":
        raise S3EncError("make_apc_config needs an apc configuration")
    c = S3ApcConfig()
    c.num_mel_bins = int(cfg.apc_feat_dim)
    c.frame_length_ms, c.frame_shift_ms = float(cfg.apc_frame_length), float(cfg.apc_frame_shift)
    c.window = APC_WINDOW.get(cfg.apc_window, -1)
    c.cmvn = int(cfg.apc_cmvn)
    c.hidden, c.num_layers, c.residual = int(cfg.conv_dim), int(cfg.apc_layers), int(cfg.apc_residual)
    return c


MJ_FRONTEND = {"kaldi": 0, "mel": 1}                                               # s3enc_mockingjay_config.frontend


def make_mockingjay_config(cfg) -> S3MockingjayConfig:
    """The second configuration block of a ``family="mockingjay"`` EncoderConfig (``s3enc_create_mockingjay``)."""
    if cfg.family != "mockingjay":
        raise S3EncError("make_mockingjay_config needs a mockingjay configuration")
    c = S3MockingjayConfig()
    c.input_dim, c.layer_norm_eps = int(cfg.mj_input_dim), float(cfg.mj_layer_norm_eps)
    c.share_layer, c.sequence_length = int(cfg.mj_share_layer), int(cfg.mj_sequence_length)
    c.frontend = MJ_FRONTEND.get(cfg.mj_frontend, -1)
    c.n_mels, c.target_level, c.cmvn = int(cfg.mj_input_dim), float(cfg.mj_target_level), int(cfg.mj_cmvn)
    c.pre_layer_norm, c.hidden_act = int(cfg.mj_pre_layer_norm), int(cfg.mj_hidden_act != "gelu")
    c.fbank_num_mel_bins = int(cfg.mj_kaldi_mel_bins)
    c.fbank_frame_length_ms, c.fbank_frame_shift_ms = float(cfg.mj_kaldi_frame_length), float(cfg.mj_kaldi_frame_shift)
    c.fbank_preemphasis = float(cfg.mj_kaldi_preemphasis)
    c.fbank_delta_order, c.fbank_delta_win_length = int(cfg.mj_delta_order), int(cfg.mj_delta_win)
    c.fbank_use_cmvn, c.fbank_cmvn_eps = int(cfg.mj_cmvn), 1e-10
    return c


def make_decoar_config(cfg) -> S3DecoarConfig:
    """The second configuration block of a ``family="decoar"`` EncoderConfig (``s3enc_create_decoar``)."""
    if cfg.family != "decoar":
        raise S3EncError("make_decoar_config needs a decoar configuration")
    c = S3DecoarConfig()
    c.num_mel_bins, c.hidden, c.num_layers = int(cfg.decoar_feat_dim), int(cfg.decoar_hidden), int(cfg.decoar_layers)
    c.frame_length_ms, c.frame_shift_ms = float(cfg.decoar_frame_length), float(cfg.decoar_frame_shift)
    c.subsample, c.per_layer_states = int(cfg.decoar_subsample), int(cfg.decoar_per_layer)
    return c


NPC_ACTIVATE = {"relu": 0, "tanh": 1}                                              # s3enc_npc_config.activate


def make_npc_config(cfg) -> S3NpcConfig:
    """The second configuration block of a ``family="npc"`` EncoderConfig (``s3enc_create_npc``)."""
    if cfg.family != "npc":
        raise S3EncError("make_npc_config needs an npc configuration")
    c = S3NpcConfig()
    c.num_mel_bins = int(cfg.apc_feat_dim)
    c.frame_length_ms, c.frame_shift_ms = float(cfg.apc_frame_length), float(cfg.apc_frame_shift)
    c.window = APC_WINDOW.get(cfg.apc_window, -1)
    c.cmvn = int(cfg.apc_cmvn)
    c.hidden, c.n_blocks = int(cfg.conv_dim), int(cfg.npc_blocks)
    c.kernel_size, c.mask_size = int(cfg.npc_kernel_size), int(cfg.npc_mask_size)
    c.residual, c.batch_norm = int(cfg.npc_residual), int(cfg.npc_batch_norm)
    c.activate = NPC_ACTIVATE.get(cfg.npc_activate, -1)
    c.disable_cross_layer = int(cfg.npc_disable_cross_layer)
    c.dim_bottleneck = int(cfg.npc_dim_bottleneck or 0)
    return c


def make_vggish_config(cfg) -> S3VggishConfig:
    """The second configuration block of a ``family="vggish"`` EncoderConfig (``s3enc_create_vggish``)."""
    if cfg.family != "vggish":
        raise S3EncError("make_vggish_config needs a vggish configuration")
    if len(cfg.vg_layers) > S3ENC_VGGISH_MAX_LAYERS:
        raise S3EncError("too many vggish conv layers")
    c = S3VggishConfig()
    c.num_mel_bins, c.n_fft = int(cfg.vg_num_mel_bins), int(cfg.vg_n_fft)
    c.window, c.shift = int(cfg.conv_layers[0][1]), int(cfg.conv_layers[0][2])
    c.mel_min_hz, c.mel_max_hz, c.log_offset = float(cfg.vg_mel_min_hz), float(cfg.vg_mel_max_hz), float(cfg.vg_log_offset)
    c.example_frames, c.example_hop = int(cfg.vg_example_frames), int(cfg.vg_example_hop)
    c.n_layers = len(cfg.vg_layers)
    for i, (ch, pool) in enumerate(cfg.vg_layers):
        c.channels[i], c.pool_after[i] = int(ch), int(bool(pool))
    for i, f in enumerate(cfg.vg_fc):
        c.fc[i] = int(f)
    c.postprocess = int(cfg.vg_postprocess)
    c.quant_min, c.quant_max = float(cfg.vg_quant_min), float(cfg.vg_quant_max)
    return c


def make_byol_a_config(cfg) -> S3ByolAConfig:
    """The second configuration block of a ``family="byol_a"`` EncoderConfig (``s3enc_create_byol_a``)."""
    if cfg.family != "byol_a":
        raise S3EncError("make_byol_a_config needs a byol_a configuration")
    c = S3ByolAConfig()
    c.feature_d, c.window, c.stride = (int(v) for v in cfg.conv_layers[0])
    c.norm_mean, c.norm_std, c.bn_eps = float(cfg.ba_norm_mean), float(cfg.ba_norm_std), float(cfg.ba_bn_eps)
    return c


def make_mae_ast_config(cfg, weights) -> S3MaeAstConfig:
    """The second configuration block of a ``family="mae_ast"`` EncoderConfig (``s3enc_create_mae_ast``).  The BatchNorm's running
    statistics are checkpoint tensors: they are read off ``weights`` and travel in the block."""
    if cfg.family != "mae_ast":
        raise S3EncError("make_mae_ast_config needs a mae_ast configuration")
    for name in ("batch_norm.running_mean", "batch_norm.running_var"):
        if name not in weights:
            raise S3EncError(f"make_mae_ast_config: missing parameter {name}")
    as_float = lambda w: float(w.detach().cpu().reshape(-1)[0]) if hasattr(w, "detach") else float(w.reshape(-1)[0])
    c = S3MaeAstConfig()
    c.kt, c.kc, c.feature_dim = int(cfg.ma_kt), int(cfg.ma_kc), int(cfg.ma_feature_dim)
    c.bn_mean, c.bn_var = as_float(weights["batch_norm.running_mean"]), as_float(weights["batch_norm.running_var"])
    c.bn_eps, c.pos_rows = float(cfg.ma_bn_eps), int(cfg.ma_pos_rows)
    return c


def make_byol_s_config(cfg) -> S3ByolSConfig:
    """The second configuration block of a ``family="byol_s"`` EncoderConfig (``s3enc_create_byol_s``)."""
    if cfg.family != "byol_s":
        raise S3EncError("make_byol_s_config needs a byol_s configuration")
    c = S3ByolSConfig()
    c.network = BYOL_S_NETWORK[cfg.bs_network]
    for i, b in enumerate(cfg.bs_blocks):
        c.blocks[i] = int(b)
    c.bottleneck = int(cfg.bs_block != "basic")
    _, c.window, c.step = (int(v) for v in cfg.conv_layers[0])
    c.bn_eps = float(cfg.bs_bn_eps)
    return c


def make_ssast_config(cfg) -> S3SsastConfig:
    """The second configuration block of a ``family="ssast"`` EncoderConfig (``s3enc_create_ssast``)."""
    if cfg.family != "ssast":
        raise S3EncError("make_ssast_config needs an ssast configuration")
    c = S3SsastConfig()
    c.fshape, c.tshape, c.fstride, c.tstride = int(cfg.ss_fshape), int(cfg.ss_tshape), int(cfg.ss_fstride), int(cfg.ss_tstride)
    c.window_samples, c.target_length = int(cfg.ss_window_samples), int(cfg.ss_target_length)
    c.ln_eps, c.pos_rows = float(cfg.ss_ln_eps), int(cfg.ss_f_dim * cfg.ss_t_dim)
    return c


class BlockFamily(NamedTuple):
    """A family whose handle takes a second configuration block through a create entry of its own (csrc: its FamilyOps record)."""
    block: type                  # the ctypes struct of the block
    make: Callable               # its make_*_config: EncoderConfig (and the weights, with reads_weights) -> block
    create: str                  # the create symbol that takes the block
    built: str                   # who "is" / "are" built for compute dtype fp32 only, with the verb
    reads_weights: bool = False  # make_*_config(cfg, weights)

    def make_block(self, cfg, weights):
        return self.make(cfg, weights) if self.reads_weights else self.make(cfg)


# keyed as FAMILY; a family that is not here is created by s3enc_create from s3enc_config alone
BLOCK_FAMILIES = {
    "wav2vec": BlockFamily(S3Wav2vecConfig, make_wav2vec_config, "s3enc_create_ex", "wav2vec / vq-wav2vec are"),
    "cpc": BlockFamily(S3CpcConfig, make_cpc_config, "s3enc_create_cpc", "modified CPC is"),
    "apc": BlockFamily(S3ApcConfig, make_apc_config, "s3enc_create_apc", "APC / VQ-APC are"),
    "mockingjay": BlockFamily(S3MockingjayConfig, make_mockingjay_config, "s3enc_create_mockingjay", "Mockingjay / TERA / AudioALBERT are"),
    "decoar": BlockFamily(S3DecoarConfig, make_decoar_config, "s3enc_create_decoar", "DeCoAR is"),
    "npc": BlockFamily(S3NpcConfig, make_npc_config, "s3enc_create_npc", "NPC is"),
    "vggish": BlockFamily(S3VggishConfig, make_vggish_config, "s3enc_create_vggish", "VGGish is"),
    "byol_a": BlockFamily(S3ByolAConfig, make_byol_a_config, "s3enc_create_byol_a", "BYOL-A is"),
    "mae_ast": BlockFamily(S3MaeAstConfig, make_mae_ast_config, "s3enc_create_mae_ast", "MAE-AST is", reads_weights=True),
    "byol_s": BlockFamily(S3ByolSConfig, make_byol_s_config, "s3enc_create_byol_s", "BYOL-S is"),
    "ssast": BlockFamily(S3SsastConfig, make_ssast_config, "s3enc_create_ssast", "SSAST is"),
}
assert set(BLOCK_FAMILIES) <= set(FAMILY)
_PROTOS.update({f.create: (C.c_int, [C.POINTER(S3Config), C.POINTER(f.block), C.POINTER(S3Tensor), _I32, _I32, C.POINTER(_VP)])
                for f in BLOCK_FAMILIES.values()})
