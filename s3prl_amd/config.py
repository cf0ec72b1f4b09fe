"""Typed view of the hyper-parameters that select kernel variants on the upstream-encoder path.

Mirrors the subset of the reference config objects that the forward actually reads:

* ``HubertConfig`` / ``HubertPretrainingConfig``  (s3prl/upstream/hubert/hubert_model.py:33-278)
* ``Wav2Vec2Config`` / ``AudioPretrainingConfig`` (s3prl/upstream/wav2vec2/wav2vec2_model.py:2103-2350,3325-3345)
* ``WavLMConfig``                                 (s3prl/upstream/wavlm/WavLM.py:162-245)
* ``MultiresHubertConfig``                        (s3prl/upstream/multires_hubert/hubert_model.py:97-330)

Like ``merge_with_parent`` (s3prl/upstream/utils.py:31-44) unknown keys of a checkpoint's
config dict are dropped, missing ones fall back to the reference defaults.
"""

from __future__ import annotations

import ast
from dataclasses import dataclass, field, asdict
from typing import Dict, List, Tuple

FAMILIES = ("hubert", "wav2vec2", "wavlm", "distiller", "multires_hubert", "wav2vec", "cpc", "apc", "mockingjay", "decoar", "npc", "vggish", "byol_a", "mae_ast", "byol_s", "lighthubert", "decoar2", "ssast")

# reference default: "[(512,10,5)] + [(512,3,2)] * 4 + [(512,2,2)] * 2"
DEFAULT_CONV_LAYERS = "[(512,10,5)] + [(512,3,2)] * 4 + [(512,2,2)] * 2"


def parse_conv_layers(spec) -> List[Tuple[int, int, int]]:
    """The reference ``eval``s this string (hubert_model.py:297, wav2vec2_model.py:2357).

    We only accept the arithmetic-on-literal-lists subset, evaluated without ``eval``.
    """
    if not isinstance(spec, str):
        return [tuple(int(v) for v in t) for t in spec]

    def ev(node):
        if isinstance(node, ast.Expression):
            return ev(node.body)
        if isinstance(node, ast.BinOp) and isinstance(node.op, ast.Add):
            return ev(node.left) + ev(node.right)
        if isinstance(node, ast.BinOp) and isinstance(node.op, ast.Mult):
            l, r = ev(node.left), ev(node.right)
            return l * r
        if isinstance(node, (ast.List, ast.Tuple)):
            vals = [ev(e) for e in node.elts]
            return vals if isinstance(node, ast.List) else tuple(vals)
        if isinstance(node, ast.Constant) and isinstance(node.value, int):
            return node.value
        raise ValueError(f"unsupported conv_feature_layers expression: {spec!r}")

    layers = ev(ast.parse(spec, mode="eval"))
    out = []
    for t in layers:
        if len(t) != 3:
            raise ValueError("invalid conv definition: " + str(t))
        out.append((int(t[0]), int(t[1]), int(t[2])))
    return out


@dataclass
class EncoderConfig:
    family: str = "hubert"
    conv_layers: List[Tuple[int, int, int]] = field(
        default_factory=lambda: parse_conv_layers(DEFAULT_CONV_LAYERS)
    )
    extractor_mode: str = "default"  # "default" (GroupNorm after conv0) | "layer_norm"
    conv_bias: bool = False
    encoder_layers: int = 12
    encoder_embed_dim: int = 768
    encoder_ffn_embed_dim: int = 3072
    encoder_attention_heads: int = 12
    layer_norm_first: bool = False
    conv_pos: int = 128
    conv_pos_groups: int = 16
    normalize: bool = False  # task_cfg.normalize: per-utterance waveform layer-norm
    # WavLM only
    relative_position_embedding: bool = False
    num_buckets: int = 320
    max_distance: int = 1280
    gru_rel_pos: bool = False
    # DistilHuBERT (family "distiller", upstream/distiller/model.py:17-80): no LayerNorm between the conv stack and
    # post_extract_proj, and ``pred_heads`` prediction heads (Linear -> GELU -> SplitLinear) on the last layer
    feature_layer_norm: bool = True
    pred_heads: int = 0
    # data2vec-audio (upstream/data2vec, wav2vec2_model.py:2995-3023): pos_conv_depth > 1 replaces the weight-normed
    # positional conv by that many {Conv1d(k = max(3, conv_pos // depth), groups) -> LayerNorm(no affine) -> GELU} blocks
    pos_conv_depth: int = 1
    # LightHuBERT (family "lighthubert", upstream/lighthubert): the encoder_* fields describe the SUBNET that runs; the checkpoint
    # holds the 768-wide supernet it is cut from.  ``lh_model`` is the checkpoint's ``cfg.model._name`` ("hubert_pruner": the
    # released subnet of ``lh_supernet``; "student_hubert": the supernet's largest subnet), ``lh_supernet`` "base" | "small"
    lh_model: str = ""
    lh_supernet: str = ""
    # eps of the per-utterance waveform normalisation: F.layer_norm's 1e-5 in the fairseq experts (hubert/expert.py:57-58),
    # 1e-7 in Hugging Face's Wav2Vec2FeatureExtractor (hf_hubert / hf_wav2vec2 upstreams)
    wav_norm_eps: float = 1e-5
    # multi-resolution HuBERT (family "multires_hubert", upstream/multires_hubert/hubert_model.py:337-530): a U-net of
    # TransformerEncoders — encoders[i] -> conv adapter (down) ... middle ... conv adapter (up) -> decoders[i] — over the
    # frame rates given by ``label_rate_ratios`` = [up_0, down_0, up_1, down_1, ...].  ``block_layers``: layers of every
    # encoder in execution order (encoders..., middle, decoders...); ``encoder_layers`` is then their sum.
    label_rate_ratios: List[int] = field(default_factory=list)
    block_layers: List[int] = field(default_factory=list)
    conv_adapter_kernel: int = 7          # the reference spells it ``conv_adapator_kernal``
    use_plain_updownsample: bool = False  # ConvDownsampler / ConvUpsampler instead of the two-conv ConvAdapter
    # wav2vec 2.0 Conformer (family "wav2vec2", ConformerEncoder, wav2vec2_model.py:440-578,3132-3211): layer_type "conformer"
    # replaces the Transformer block by FFN/2 -> MHA -> conv module -> FFN/2 -> LayerNorm and drops the positional conv;
    # pos_enc_type "rel_pos" (Transformer-XL relative attention) or "rope" (rotary), attn_type "espnet" only
    layer_type: str = "transformer"
    pos_enc_type: str = "abs"
    attn_type: str = ""
    depthwise_conv_kernel_size: int = 31
    # wav2vec / vq-wav2vec (family "wav2vec", Wav2VecConfig, upstream/wav2vec/wav2vec_model.py:289-410): ``conv_layers`` is the
    # extractor, ``agg_layers`` the causal convolutional aggregator; every block is Conv1d -> GroupNorm(1, C) -> ReLU.  There is no
    # Transformer: ``encoder_layers`` = len(agg_layers) and ``encoder_embed_dim`` = the conv width, so the states are
    # (encoder_layers + 1) x (B, T, C): z and every aggregator layer's output
    agg_layers: List[Tuple[int, int, int]] = field(default_factory=list)
    aggregator: str = "cnn"
    activation: str = "relu"
    log_compression: bool = True
    skip_connections_feat: bool = False
    skip_connections_agg: bool = True
    residual_scale: float = 0.5
    non_affine_group_norm: bool = False
    no_conv_bias: bool = False
    agg_zero_pad: bool = False
    vq_type: str = "none"  # "none" | "gumbel" | "kmeans"
    vq_vars: int = 320
    vq_groups: int = 2
    vq_dim: int = 0        # 0 = the extractor width
    vq_depth: int = 1
    combine_groups: bool = False
    # modified CPC (family "cpc", upstream/cpc/model.py:62-104,146-191, cpc_default_config.py): ``conv_layers`` with ``conv_pads``
    # zero frames on both sides of every convolution, each followed by a per-frame channel norm and ReLU, then ``ar_layers``
    # LSTM / GRU layers of width ``ar_hidden``.  No Transformer: ``encoder_layers`` = 1 and ``encoder_embed_dim`` = the conv
    # width, so the states are 2 x (B, T, C): the encoder output and the recurrent output
    conv_pads: List[int] = field(default_factory=list)
    norm_mode: str = "layerNorm"   # normMode: only the channel norm is built
    ar_mode: str = "LSTM"          # arMode: "LSTM" | "GRU"
    ar_layers: int = 1             # nLevelsGRU
    ar_hidden: int = 256           # hiddenGar
    cpc_reverse: bool = False      # cpc_mode == "reverse" (refused)
    cpc_keep_hidden: bool = False  # samplingType == "sequential" (refused)
    # APC / VQ-APC (family "apc", upstream/apc/apc.py:26-169, audio.py:53-115): a kaldi log-mel front end and ``apc_layers`` GRU
    # layers of width ``conv_dim`` on packed sequences.  ``conv_layers`` = [(hidden, window, shift)] in samples carries the frame
    # geometry; ``encoder_layers`` = 2 and ``encoder_embed_dim`` = hidden, so the states are 3 x (B, T, hidden): the inputs of
    # rnn_layers[1] and rnn_layers[2] and the last layer's output
    apc_feat_type: str = "fbank"      # audio.feat_type: only the Mel spectrogram exists in the reference
    apc_feat_dim: int = 80            # audio.feat_dim = num_mel_bins
    apc_frame_length: float = 25.0    # ms
    apc_frame_shift: float = 10.0     # ms
    apc_window: str = "hamming"       # the reference's WINDOW_TYPE constant
    apc_cmvn: bool = True             # audio.cmvn
    apc_layers: int = 3               # paras.num_layers
    apc_residual: bool = True         # paras.residual
    apc_vq: Dict | None = None        # paras.vq (VQ-APC): feeds only the discarded prediction; kept for the checkpoint round trip
    # Mockingjay / TERA / AudioALBERT (family "mockingjay", upstream/mockingjay/{builder,model}.py): a spectrogram front end, the
    # input representation (Linear + sinusoid position table + LayerNorm) and ``encoder_layers`` post-LN BERT layers of width
    # ``encoder_embed_dim``.  ``conv_layers`` = [(hidden, window, 160)] carries the frame geometry: window 0 for the mel front end
    # (centred frames: T = 1 + n // 160), the analysis window in samples for the kaldi one
    mj_input_dim: int = 80            # width of a feature row (n_mels, or num_mel_bins * (delta order + 1))
    mj_layer_norm_eps: float = 1e-12  # transformer.layer_norm_eps: EVERY LayerNorm of the family
    mj_share_layer: bool = False      # transformer.share_layer (AudioALBERT): one layer's weights run encoder_layers times
    mj_sequence_length: int = 1500    # task.sequence_length: longer inputs are forwarded in torch.chunk pieces; 0 = never
    mj_frontend: str = "mel"          # "mel" (audio.input: OnlinePreprocessor) or "kaldi" (audio.kaldi: baseline/extracter.py)
    mj_target_level: float = -25.0    # audio.target_level (mel)
    mj_cmvn: bool = True              # audio.input.cmvn (mel) / audio.cmvn.use_cmvn (kaldi)
    mj_pre_layer_norm: bool = False   # transformer.pre_layer_norm (refused)
    mj_hidden_act: str = "gelu"       # transformer.hidden_act (anything else is refused)
    mj_kaldi_mel_bins: int = 80       # audio.kaldi.fbank.num_mel_bins
    mj_kaldi_frame_length: float = 25.0
    mj_kaldi_frame_shift: float = 10.0
    mj_kaldi_preemphasis: float = 0.97
    mj_delta_order: int = 2           # audio.delta.order (kaldi)
    mj_delta_win: int = 5             # audio.delta.win_length
    # DeCoAR / DeCoAR-layers (family "decoar", upstream/decoar/{decoar,audio,expert}.py, upstream/decoar_layers/): a kaldi log-mel
    # front end (hamming, CMVN over time), Linear feat_dim -> hidden, a forward and a backward stack of ``decoar_layers``
    # unidirectional LSTM layers on packed sequences, concatenated.  ``conv_layers`` = [(2 * hidden, window, shift)] in samples
    # carries the frame geometry and the state width; ``encoder_layers`` = the number of states - 1
    decoar_feat_dim: int = 80           # num_mel_bins
    decoar_hidden: int = 1024           # d
    decoar_layers: int = 4              # encoder_layers of the reference's Decoar()
    decoar_frame_length: float = 25.0   # ms (kaldi.fbank's default)
    decoar_frame_shift: float = 10.0    # ms
    decoar_subsample: int = 1           # every n-th frame: 1 (decoar/audio.py keeps them all) or 2 (decoar2/audio.py:84)
    decoar_per_layer: bool = False      # False: one state, the last layer (decoar); True: one per layer (decoar_layers)

    # NPC (family "npc", upstream/npc/npc.py:21-248): APC's front end — the ``apc_*`` fields above are its ``data.audio`` — and
    # ``npc_blocks`` ConvBlocks, each (or, with ``npc_disable_cross_layer``, only the last) followed by a masked convolution.
    # ``conv_layers`` = [(hidden, window, shift)] in samples; ``encoder_layers`` = the number of states - 1
    npc_blocks: int = 4               # paras.n_blocks
    npc_kernel_size: int = 15         # paras.kernel_size of the masked convolutions
    npc_mask_size: int = 5            # paras.mask_size: block i masks mask_size + 2 (i + 1) taps in the middle
    npc_residual: bool = True         # paras.residual (blocks 1..)
    npc_batch_norm: bool = True       # paras.batch_norm
    npc_activate: str = "relu"        # paras.activate: relu | tanh
    npc_disable_cross_layer: bool = False  # paras.disable_cross_layer
    npc_vq: Dict | None = None        # paras.vq: feeds only the discarded prediction; kept for the checkpoint round trip
    npc_dim_bottleneck: int | None = None  # paras.dim_bottleneck: the last state would have another width (refused)

    # VGGish (family "vggish", upstream/vggish/{audio,vggish,vggish_params}.py): an un-padded log-mel front end cut into examples,
    # a 3 x 3 Conv2d + ReLU (+ 2 x 2 max-pool) stack, three Linear + ReLU layers and the PCA / 8-bit quantiser.
    # ``conv_layers`` = [(embedding width, window, shift)] in samples; ``encoder_layers`` = 0: one state
    vg_num_mel_bins: int = 64         # NUM_MEL_BINS
    vg_n_fft: int = 512               # the power of two at or above the window
    vg_mel_min_hz: float = 125.0      # MEL_MIN_HZ
    vg_mel_max_hz: float = 7500.0     # MEL_MAX_HZ
    vg_log_offset: float = 0.01       # LOG_OFFSET
    vg_example_frames: int = 96       # EXAMPLE_WINDOW_SECONDS in frames
    vg_example_hop: int = 96          # EXAMPLE_HOP_SECONDS in frames (only = vg_example_frames is built)
    vg_layers: List[Tuple[int, bool]] = field(default_factory=lambda: [(64, True), (128, True), (256, False), (256, True),
                                                                      (512, False), (512, True)])  # (channels, pool behind it)
    vg_fc: Tuple[int, int, int] = (4096, 4096, 128)  # the three Linear widths; the last one is the embedding
    vg_postprocess: bool = True       # the PCA + clamp + 8-bit quantiser (vggish.py:44-120)
    vg_quant_min: float = -2.0        # QUANTIZE_MIN_VAL
    vg_quant_max: float = 2.0         # QUANTIZE_MAX_VAL

    # BYOL-A (family "byol_a", upstream/byol_a/{expert,byol_a}.py, config.yaml): segments of ``window`` samples every ``stride``
    # samples, each through a 1024-point log-mel front end, three conv + BatchNorm + ReLU + floor-pool layers, two Linears and
    # max + mean over time.  ``conv_layers`` = [(feature_d, window, stride)] in samples; ``encoder_layers`` = 0: one state
    ba_window_secs: float = 1.0       # the expert's constructor arguments as given; the samples are int(secs * 16000)
    ba_stride_secs: float = 1.0
    ba_norm_mean: float = -5.4919195  # expert.py:56-60: PrecomputedNorm's statistics
    ba_norm_std: float = 5.0389895
    ba_bn_eps: float = 1e-5           # nn.BatchNorm2d's default

    # MAE-AST (family "mae_ast", upstream/mae_ast/{expert,mae_ast}.py): a kaldi log-mel front end at 128 bins, eval BatchNorm2d(1) x 0.5,
    # nn.Unfold into ``ma_kt`` x ``ma_kc`` patches, Linear, the checkpoint's sinusoidal position rows, ``encoder_layers`` Transformer
    # layers with key padding.  ``conv_layers`` = [(D, 400, 160)] carries the frame geometry; the states are ``encoder_layers`` x
    # (B, F // kt, (128 // kc) * D): the layer outputs, not the embedding.  The BatchNorm statistics are checkpoint tensors
    ma_kt: int = 16                   # ast_kernel_size_time (= ast_kernel_stride_time)
    ma_kc: int = 16                   # ast_kernel_size_chan (= ast_kernel_stride_chan)
    ma_stride_t: int = 16             # ast_kernel_stride_time: anything but the kernel is refused
    ma_stride_c: int = 16             # ast_kernel_stride_chan
    ma_feature_dim: int = 128         # task.feature_dim (the reference's mask rule hard-codes 128)
    ma_sample_rate: int = 16000       # task.sample_rate
    ma_bn_eps: float = 1e-5           # nn.BatchNorm2d's default
    ma_max_token_length: int = 48000  # rows of the checkpoint's sinusoidal tables
    ma_enc_sine_pos: bool = True      # enc_sine_pos (False is refused: no released checkpoint)
    ma_enc_conv_pos: bool = False     # enc_conv_pos (True is refused)
    ma_activation: str = "gelu"       # activation_fn (anything else is refused)
    ma_decoder_layers: int = 2        # the decoder is in the strict state dict and never runs
    ma_dec_sine_pos: bool = True

    # BYOL-S (family "byol_s", upstream/byol_s/{expert.py,serab_byols,byol_a/models}): centred windows of ``window`` samples every
    # ``step`` samples, a hann(400) log-mel front end, the statistics of the whole batch, AudioNTT2020 ("default") or a ResNet of
    # BasicBlocks ("resnetish"), mean + max over time.  ``conv_layers`` = [(2048, window, step)] in samples; one state
    bs_network: str = "default"       # "default" | "resnetish"; "cvt" and "clstm" are refused by name
    bs_blocks: Tuple[int, ...] = (3, 4, 6, 3)  # resnetish: BasicBlocks per layer (resnetish34)
    bs_block: str = "basic"           # "bottleneck" (resnetish50) is refused by name
    bs_window_secs: float = 1.0       # the expert's constructor arguments as given
    bs_hop_secs: float = 0.05
    bs_bn_eps: float = 1e-5           # nn.BatchNorm2d's default

    # SSAST (family "ssast", upstream/ssast/{expert,ast_models,audio}.py): fixed windows of ``ss_window_secs``, per window a hanning
    # kaldi log-mel at 128 bins with an affine normalisation, zero rows up to ``ss_target_length``, a Conv2d patch embedding with
    # overlapping patches behind a cls and a dist token, ``encoder_layers`` pre-LN timm blocks.  ``conv_layers`` = [(D, 400, 160)]
    # carries the frame geometry; the states are ``encoder_layers`` x (B, T_out, f_dim * D)
    ss_fshape: int = 16               # patch extent in mel bins (frame model: 128)
    ss_tshape: int = 16               # patch extent in frames (frame model: 2)
    ss_fstride: int = 10              # (frame model: 128)
    ss_tstride: int = 10              # (frame model: 1)
    ss_window_secs: float = 1.0       # the expert's constructor argument as given; the samples are int(secs * 16000)
    ss_ln_eps: float = 1e-6           # timm 0.4.5 VisionTransformer: partial(nn.LayerNorm, eps=1e-6)
    ss_p_input_fdim: int = 128        # module.p_input_fdim / p_input_tdim of the pretraining file: the grid its pos_embed was made for
    ss_p_input_tdim: int = 1024

    # ---- derived -------------------------------------------------------------------------
    @property
    def conv_dim(self) -> int:
        return self.conv_layers[-1][0]

    @property
    def head_dim(self) -> int:
        return self.encoder_embed_dim // self.encoder_attention_heads

    @property
    def pos_conv_kernel(self) -> int:
        return self.conv_pos if self.pos_conv_depth <= 1 else max(3, self.conv_pos // self.pos_conv_depth)

    @property
    def num_hidden_states(self) -> int:
        """Entries of the default ``hidden_states`` list: layer inputs + encoder output; DistilHuBERT:
        feat_final + every layer output + the prediction heads (distiller/expert.py:43-52)."""
        if self.family == "multires_hubert":  # every block: its layer inputs + its output (multires_hubert/expert.py:49-91)
            return sum(n + 1 for n in self.block_layers)
        if self.family == "mae_ast":  # the layer outputs; the embedding is not among them (mae_ast.py:671-677)
            return self.encoder_layers
        if self.family == "ssast":  # the blocks' outputs (ast_models.py:381-393)
            return self.encoder_layers
        return self.encoder_layers + 1 + self.pred_heads

    # ---- SSAST geometry (ssast/expert.py:44-78, ast_models.py:354-365) ----------------------
    @property
    def ss_window_samples(self) -> int:
        return int(self.ss_window_secs * 16000)

    @property
    def ss_target_length(self) -> int:
        return int(self.ss_window_secs * 16000 / 160)

    @property
    def ss_f_dim(self) -> int:
        return (128 - self.ss_fshape) // self.ss_fstride + 1

    @property
    def ss_t_dim(self) -> int:
        return (self.ss_target_length - self.ss_tshape) // self.ss_tstride + 1

    @property
    def ss_pretrain_grid(self) -> Tuple[int, int]:
        """(p_f_dim, p_t_dim): the patch grid of the pretraining stage, where stride = shape (ast_models.py:236-249)."""
        return self.ss_p_input_fdim // self.ss_fshape, self.ss_p_input_tdim // self.ss_tshape

    def ss_num_windows(self, n: int) -> int:
        return -(-n // self.ss_window_samples) if n > 0 else 0

    def ss_num_steps(self, n: int) -> int:
        """T_out: nseg * t_dim rows cut to len(range(0, max_len, 160 * tstride)) (ssast/expert.py:127-131)."""
        return min(self.ss_num_windows(n) * self.ss_t_dim, -(-n // (160 * self.ss_tstride))) if n > 0 else 0

    @property
    def downsample_rate(self) -> int:
        if self.family == "vggish":  # vggish/expert.py:21-22 (the examples are 15360 samples apart; the reference says 16000)
            return 16000
        if self.family == "mae_ast":  # mae_ast/expert.py:57-58
            return self.ma_kt * 160
        if self.family == "ssast":  # ssast/expert.py:82-83
            return self.ss_tstride * 160
        r = 1
        for _, _, s in self.conv_layers:
            r *= s
        return 2 * r if self.family == "decoar2" else r  # decoar2/expert.py:65-66: 320, every second 10 ms frame

    def conv_lengths(self, n: int) -> List[int]:
        """floor((L-k)/s)+1 per layer (wav2vec2_model.py:2615-2616); modified CPC: floor((L + 2 pad - k)/s)+1."""
        out = []
        pads = self.conv_pads if self.family == "cpc" else [0] * len(self.conv_layers)
        for (_, k, s), p in zip(self.conv_layers, pads):
            n = (n + 2 * p - k) // s + 1 if n > 0 and n + 2 * p >= k else 0
            out.append(n)
        return out

    def num_frames(self, n: int) -> int:
        if self.family == "mockingjay" and self.mj_frontend == "mel":  # centred STFT frames; torch.stft refuses n <= 200
            return 1 + n // 160 if n > 200 else 0
        if self.family == "decoar":  # ceil(fbank frames / subsample)
            return -(-self.conv_lengths(n)[-1] // self.decoar_subsample)
        if self.family == "decoar2":  # y[::2] of the fbank frames (decoar2/audio.py:84)
            return -(-self.conv_lengths(n)[-1] // 2)
        if self.family == "mae_ast":  # time steps of kt frames; the frames behind the last whole step are dropped by nn.Unfold
            return self.conv_lengths(n)[-1] // self.ma_kt
        if self.family == "ssast":
            return self.ss_num_steps(n)
        if self.family == "byol_s":  # windows: frame_audio's loop (byol_s/serab_byols/utils.py:79-96)
            return n // self.conv_layers[0][2] + 1 if n >= 0 else 0
        if self.family == "byol_a":  # segments: len(range(0, n, stride)) (byol_a/expert.py:85)
            return -(-n // self.conv_layers[0][2]) if n > 0 else 0
        if self.family == "vggish":  # examples: complete groups of vg_example_frames un-padded frames (audio.py:90-111)
            F = self.conv_lengths(n)[-1]
            return 1 + (F - self.vg_example_frames) // self.vg_example_hop if F >= self.vg_example_frames else 0
        return self.conv_lengths(n)[-1]

    def valid_frames(self, length: int, n_max: int) -> int:
        """Number of un-masked frames of an utterance of ``length`` samples in a batch padded to
        ``n_max`` samples.

        hubert / wavlm: ``forward_padding_mask`` (hubert_model.py:454-464, WavLM.py:339-349):
        chunk = n_max // T; frame t is padding iff all samples of its chunk are padding.
        wav2vec2: conv-length formula of ``length`` (wav2vec2_model.py:2652-2669).
        """
        T = self.num_frames(n_max)
        if T <= 0:
            return 0
        if self.family == "mae_ast":  # forward_padding_mask (mae_ast.py:305-325): a step that is only partly real counts as real
            return min(T, max(-(-self.conv_lengths(length)[-1] // self.ma_kt), 0))
        if self.family == "ssast":  # the wrapper's rule at the expert's rate; the rows behind it are the reference's values, not zeros
            return min(T, max(-(-length // self.downsample_rate), 0))
        if self.family == "mockingjay" and self.mj_frontend == "mel":
            # preprocessor.py:204-205: batch-dependent, Python floats and Python's round; without CMVN no feature row is zero
            return min(T, max(round(length / (n_max / T)), 0)) if self.mj_cmvn else T
        if self.family == "mockingjay":
            return min(T, max(self.num_frames(length), 0))
        if self.family in ("wav2vec2", "distiller", "wav2vec", "cpc", "apc", "decoar", "decoar2", "npc", "vggish", "byol_a", "byol_s"):  # decoar2: the utterance's own frames (decoar2/expert.py:86-94); byol_s: the utterance's own windows (the rows behind them are the reference's values, not zeros); byol_a: the utterance's own segments (the rows behind them are the reference's values, not zeros); vggish: the utterance's own examples, exact zeros behind them; distiller: cal_pad_mask, distiller/model.py:271-285; wav2vec, cpc: no mask; apc: the packed length; npc: the utterance's own frames (the rows behind them are the reference's values, not zeros)
            return min(T, max(self.num_frames(length), 0))
        chunk = n_max // T
        return min(T, -(-length // chunk))

    # ---- multires-HuBERT geometry ---------------------------------------------------------
    @property
    def rate_pairs(self) -> List[Tuple[int, int]]:
        r = self.label_rate_ratios
        return [(int(r[2 * i]), int(r[2 * i + 1])) for i in range(len(r) // 2)]

    def adapter_frames(self, T: int, up: int, down: int, kind: str) -> int:
        """Output frames of a conv adapter on ``T`` frames (hubert_model.py:1038-1095 ConvAdapter, :1146-1180
        ConvDownsampler, :1232-1266 ConvUpsampler): every stage is cut to min(conv length, skip-connection length)."""
        k = self.conv_adapter_kernel
        n = T
        if kind in ("full", "up"):
            n = min(up * T + k - 1, up * T)  # ConvTranspose1d(padding=0, output_padding=stride-1) vs repeat_interleave
        if kind in ("full", "down"):
            ld = (n + 2 * ((k - 1) // 2) - k) // down + 1
            n2 = min(ld, -(-n // down))
            n = min(n2, -(-(up * T) // down)) if kind == "full" else n2  # highway branch (ConvAdapter only)
        return n

    def multires_plan(self, T0: int):
        """Frame geometry of the U-net for a conv-stack output of ``T0`` frames: a list of blocks
        ``dict(prefix, layers, T, factor, adapter)`` in execution order (adapter = the (kind, up, down, module prefix)
        applied BEFORE the block, None for the first), the per-decoder truncation of ``align_size_sum``
        (hubert_model.py:777-783) as ``T_sum``, and ``T_out`` = the common length the expert cuts every (upsampled)
        state to (multires_hubert/expert.py:26-27,93-101)."""
        import math

        pairs = self.rate_pairs
        R = len(pairs) + 1
        assert len(self.block_layers) == 2 * R - 1
        ds = [self.downsample_rate]
        for u, d in pairs:  # hubert_model.py:512-533
            ds.append(ds[-1] * d // u)
        lcm = 1
        for x in ds:
            lcm = lcm * x // math.gcd(lcm, x)
        upf = [lcm // x for x in ds][::-1]  # (sic) expert.py:44-45
        rev = upf[::-1][1:]
        plain = self.use_plain_updownsample
        blocks, T, enc_T, ad = [], T0, [], None
        for i in range(R - 1):
            blocks.append(dict(prefix=f"encoders.{i}", layers=self.block_layers[i], T=T, factor=upf[i], adapter=ad))
            enc_T.append(T)
            u, d = pairs[i]
            ad = ("down" if plain else "full", u, d, f"downsample_modules.{i}")
            T = self.adapter_frames(T, u, d, ad[0])
        blocks.append(dict(prefix="middle_encoder", layers=self.block_layers[R - 1], T=T, factor=upf[R - 1], adapter=ad))
        res = enc_T[::-1]
        for i in range(R - 1):
            d, u = pairs[i]  # upsample_modules[i] is built from the INVERTED pair i (hubert_model.py:474-507)
            ad = ("up" if plain else "full", u, d, f"upsample_modules.{i}")
            T = self.adapter_frames(T, u, d, ad[0])
            blocks.append(dict(prefix=f"decoders.{i}", layers=self.block_layers[R + i], T=T, factor=rev[i], adapter=ad,
                               T_sum=min(T, res[i])))
            T = min(T, res[i])
        cand = []
        for b in blocks:
            cand.append(b["T"] * b["factor"])
            if b["layers"] > 0:
                cand.append((b["T"] + b["T"] % 2) * b["factor"])  # layer inputs are padded to a multiple of 2
        return blocks, min(cand)

    def num_output_frames(self, n: int) -> int:
        """Frames of every entry of ``hidden_states`` for a batch padded to ``n`` samples."""
        T = self.num_frames(n)
        if self.family != "multires_hubert" or T < 1:
            return T
        return self.multires_plan(T)[1]

    def validate(self) -> None:
        if self.family not in FAMILIES:
            raise ValueError(f"unknown family {self.family!r}")
        if self.family == "multires_hubert":
            pairs = self.rate_pairs
            if not pairs or len(self.label_rate_ratios) % 2:
                raise ValueError("multires_hubert needs label_rate_ratios = [up, down, ...]")
            if len(pairs) > 3:
                raise ValueError("multires_hubert: at most 4 resolutions")
            if len(self.block_layers) != 2 * len(pairs) + 1 or min(self.block_layers) < 1:
                raise ValueError("multires_hubert: block_layers needs one positive entry per encoder / middle / decoder")
            if self.encoder_layers != sum(self.block_layers):
                raise ValueError("multires_hubert: encoder_layers must equal sum(block_layers)")
            k = self.conv_adapter_kernel
            if k < 1 or k % 2 == 0 or k > 15:
                raise ValueError("multires_hubert: conv_adapter_kernel must be odd and <= 15")
            for u, d in pairs:
                if self.use_plain_updownsample and u != 1:
                    raise ValueError("use_plain_updownsample needs label_rate_ratios of the form (1, d)")  # :1130,1214
                for s in (u, d):
                    if s < 1 or s > 4 or (k - 1) % s:
                        raise ValueError("multires_hubert: every rate must divide conv_adapter_kernel - 1 (the transposed "
                                         "conv is run as `rate` interleaved stride-1 convs)")
        if self.family == "wav2vec":
            return self._validate_wav2vec()
        if self.family == "cpc":
            return self._validate_cpc()
        if self.family == "apc":
            return self._validate_apc()
        if self.family == "mockingjay":
            return self._validate_mockingjay()
        if self.family == "decoar":
            return self._validate_decoar()
        if self.family == "npc":
            return self._validate_npc()
        if self.family == "vggish":
            return self._validate_vggish()
        if self.family == "byol_a":
            return self._validate_byol_a()
        if self.family == "mae_ast":
            return self._validate_mae_ast()
        if self.family == "byol_s":
            return self._validate_byol_s()
        if self.family == "ssast":
            return self._validate_ssast()
        if self.layer_type not in ("transformer", "conformer"):
            raise ValueError(f"unknown layer_type {self.layer_type!r}")
        if self.family == "lighthubert":
            if self.lh_model not in ("hubert_pruner", "student_hubert") or self.lh_supernet not in ("base", "small"):
                raise ValueError("lighthubert: lh_model must be 'hubert_pruner' or 'student_hubert' and lh_supernet 'base' or "
                                 f"'small', got {self.lh_model!r} / {self.lh_supernet!r} (config_from_lighthubert sets them)")
            if self.layer_norm_first:
                raise ValueError("lighthubert with layer_norm_first=True is not built (the released checkpoints are post-LN)")
            if self.pos_conv_depth > 1:
                raise ValueError("lighthubert with pos_conv_depth > 1 is not built (the released checkpoints have one positional conv)")
            if self.layer_type != "transformer":
                raise ValueError("lighthubert: only layer_type='transformer' exists in the reference")
        if self.family == "decoar2":
            if list(map(tuple, self.conv_layers)) != [DECOAR2_FRONT_END]:
                raise ValueError("decoar2: conv_layers carries the front end's constants as one (80 mel bins, 400, 160 samples) entry "
                                 f"(decoar2_config sets it), got {self.conv_layers}")
            if self.layer_norm_first:
                raise ValueError("decoar2 with layer_norm_first=True is not built (the reference hard-codes a post-LN encoder)")
            if self.pos_conv_depth > 1:
                raise ValueError("decoar2 with pos_conv_depth > 1 is not built (the reference has one positional conv)")
            if self.layer_type != "transformer":
                raise ValueError("decoar2: only layer_type='transformer' exists in the reference")
            if self.relative_position_embedding or self.pred_heads or not self.feature_layer_norm:
                raise ValueError("decoar2 takes none of the WavLM / DistilHuBERT options")
            if self.normalize or self.conv_bias or self.extractor_mode != "default":
                raise ValueError("decoar2 has no conv extractor and no waveform normalisation: normalize and conv_bias must be False and "
                                 "extractor_mode 'default'")
            if self.encoder_embed_dim % 64 or self.encoder_attention_heads != self.encoder_embed_dim // 64:
                raise ValueError("decoar2: embed_dim must be a multiple of 64 and heads embed_dim / 64 (768 / 12 in the reference, which "
                                 f"hard-codes its widths), got {self.encoder_embed_dim} / {self.encoder_attention_heads}")
        if self.layer_type == "conformer":
            if self.family != "wav2vec2" or self.pos_conv_depth > 1:
                raise ValueError("conformer layers are a wav2vec2-family encoder")
            if self.pos_enc_type not in ("rel_pos", "rope"):
                # ConformerEncoder is selected only for these two (wav2vec2_model.py:2447-2449); "abs" builds a Transformer
                # encoder whose layers are ConformerWav2Vec2EncoderLayer with absolute positions
                raise ValueError(f"conformer pos_enc_type={self.pos_enc_type!r} is not built: only 'rel_pos' and 'rope'")
            if self.attn_type != "espnet":
                raise ValueError(f"conformer attn_type={self.attn_type!r} is not built: only 'espnet' (the released models)")
            k = self.depthwise_conv_kernel_size
            if k < 1 or k % 2 == 0 or k > 63:
                raise ValueError("conformer depthwise_conv_kernel_size must be odd and <= 63")
        if self.extractor_mode not in ("default", "layer_norm"):
            raise ValueError(f"unknown extractor_mode {self.extractor_mode!r}")
        dims = {d for d, _, _ in self.conv_layers}
        if len(dims) != 1:
            raise ValueError("all conv feature layers must have the same width")
        if self.encoder_embed_dim % self.encoder_attention_heads:
            raise ValueError("embed_dim must be divisible by num_heads")
        if self.head_dim != 64:
            raise ValueError("the HIP attention kernel is specialised for head_dim == 64")
        if self.encoder_embed_dim % self.conv_pos_groups:
            raise ValueError("embed_dim must be divisible by conv_pos_groups")
        if self.encoder_embed_dim // self.conv_pos_groups not in (24, 32, 40, 48, 64):
            # the positional-conv kernels are built for these group widths (s3enc_create repeats it); a Conformer never runs
            # its positional conv, but its checkpoint carries one and the handle packs it.  24 and 40 (the LightHuBERT subnets)
            # exist in exact fp32 only: make_config / s3enc_create refuse the other operand modes there
            raise ValueError("embed_dim / conv_pos_groups (the positional conv's group width) must be 32, 48 or 64 (fp32: also 24 or "
                             f"40), got {self.encoder_embed_dim} / {self.conv_pos_groups}")
        if not 1 <= self.conv_pos <= 256:
            raise ValueError(f"conv_pos (the positional conv's kernel) must be 1..256, got {self.conv_pos}")

    def _validate_wav2vec(self) -> None:
        """What the HIP path builds of ``Wav2VecConfig``; everything else is refused by name (s3enc_create repeats it)."""
        if self.aggregator != "cnn":
            raise ValueError(f"wav2vec aggregator={self.aggregator!r} is not built: only the convolutional aggregator 'cnn'")
        if self.activation != "relu":
            raise ValueError(f"wav2vec activation={self.activation!r} is not built: only 'relu' (the released models)")
        if self.skip_connections_feat:
            raise ValueError("wav2vec skip_connections_feat is not built (off in the released models)")
        if not self.agg_layers:
            raise ValueError("wav2vec needs conv_aggregator_layers")
        if len({d for d, _, _ in self.conv_layers} | {d for d, _, _ in self.agg_layers}) != 1:
            raise ValueError("wav2vec layers of unequal widths are not built (the aggregator would need residual_proj)")
        if any(s != 1 for _, _, s in self.agg_layers):
            raise ValueError("wav2vec aggregator strides other than 1 are not built")
        if self.encoder_layers != len(self.agg_layers) or self.encoder_embed_dim != self.conv_dim:
            raise ValueError("wav2vec: encoder_layers / encoder_embed_dim must mirror the aggregator (config_from_wav2vec sets them)")
        if self.vq_type not in ("none", "gumbel", "kmeans"):
            raise ValueError(f"unknown vq_type {self.vq_type!r}")
        if self.vq_type != "none":
            if self.vq_dim not in (0, self.conv_dim):
                raise ValueError("wav2vec vq_dim must be 0 or the extractor width (the aggregator reads the codewords)")
            if self.conv_dim % self.vq_groups or (self.conv_dim // self.vq_groups) % 4:
                raise ValueError("wav2vec vq_groups must divide the width into multiples of 4")

    def _validate_cpc(self) -> None:
        """What the HIP path builds of the CPC configuration; everything else is refused by name (s3enc_create_cpc repeats it)."""
        if self.norm_mode != "layerNorm":
            raise ValueError(f"cpc normMode={self.norm_mode!r} is not built: only 'layerNorm' (the channel norm)")
        if self.ar_mode not in ("LSTM", "GRU"):
            raise ValueError(f"cpc arMode={self.ar_mode!r} is not built: only 'LSTM' and 'GRU'")
        if self.cpc_reverse:
            raise ValueError("cpc_mode='reverse' is not built")
        if self.cpc_keep_hidden:
            raise ValueError("cpc samplingType='sequential' (the recurrent state carried between forwards) is not built")
        if len({d for d, _, _ in self.conv_layers}) != 1 or len(self.conv_pads) != len(self.conv_layers):
            raise ValueError("cpc needs conv layers of one width and one padding per layer")
        if self.ar_hidden != self.conv_dim:
            raise ValueError(f"cpc hiddenGar != hiddenEncoder ({self.ar_hidden} != {self.conv_dim}) is not built: the two states share one width")
        if self.conv_dim % 64 or not 64 <= self.conv_dim <= 512:
            raise ValueError(f"cpc widths must be a multiple of 64, at most 512 (the recurrent kernel's limit), got {self.conv_dim}")
        if not 1 <= self.ar_layers <= 4:
            raise ValueError(f"cpc nLevelsGRU must be 1..4 recurrent layers, got {self.ar_layers}")
        if self.encoder_layers != 1 or self.encoder_embed_dim != self.conv_dim:
            raise ValueError("cpc: encoder_layers / encoder_embed_dim must be 1 / the conv width (cpc_config sets them)")

    def _validate_apc(self) -> None:
        """What the HIP path builds of the APC configuration; everything else is refused by name (s3enc_create_apc repeats it)."""
        if self.apc_feat_type != "fbank":
            raise ValueError(f"apc feat_type={self.apc_feat_type!r} is not built: only 'fbank' (the reference implements nothing else)")
        if self.apc_window not in ("hamming", "povey"):
            raise ValueError(f"apc window_type={self.apc_window!r} is not built: only 'hamming' and 'povey'")
        if not 3 <= self.apc_layers <= 4:
            raise ValueError(f"apc num_layers must be 3 or 4, got {self.apc_layers} (the reference's hooks read rnn_layers[1] and "
                             "rnn_layers[2]: fewer layers raise IndexError there; more than 4 are not built)")
        if len(self.conv_layers) != 1:
            raise ValueError("apc: conv_layers carries the frame geometry as one (hidden, window, shift) entry (apc_config sets it)")
        H, size, shift = self.conv_layers[0]
        if H % 64 or not 64 <= H <= 512:
            raise ValueError(f"apc hidden_size must be a multiple of 64, at most 512 (the recurrent kernel's limit), got {H}")
        if (size, shift) != (int(16000 * self.apc_frame_length * 0.001), int(16000 * self.apc_frame_shift * 0.001)):
            raise ValueError("apc: conv_layers does not match frame_length / frame_shift (apc_config sets it)")
        if size < 4 or shift < 4 or size % 4 or shift % 4:
            raise ValueError(f"apc frame_length / frame_shift of {size} / {shift} samples are not built: both must be a multiple of 4 "
                             "samples (the front end's GEMM reads 16-byte vectors)")
        if self.apc_feat_dim % 4 or not 4 <= self.apc_feat_dim <= 256:
            raise ValueError(f"apc feat_dim must be a multiple of 4, at most 256, got {self.apc_feat_dim}")
        if self.encoder_layers != 2 or self.encoder_embed_dim != H:
            raise ValueError("apc: encoder_layers / encoder_embed_dim must be 2 / hidden_size (apc_config sets them)")

    def npc_mask(self, i: int) -> int:
        """Masked taps of block ``i``'s masked convolution (npc.py:133-148)."""
        return self.npc_mask_size + 2 * (i + 1)

    def npc_has_mask(self, i: int) -> bool:
        return not self.npc_disable_cross_layer or i == self.npc_blocks - 1

    def _validate_npc(self) -> None:
        """What the HIP path builds of the NPC configuration; everything else is refused by name (s3enc_create_npc repeats it)."""
        if self.apc_feat_type != "fbank":
            raise ValueError(f"npc feat_type={self.apc_feat_type!r} is not built: only 'fbank' (the reference implements nothing else)")
        if self.apc_window not in ("hamming", "povey"):
            raise ValueError(f"npc window_type={self.apc_window!r} is not built: only 'hamming' and 'povey'")
        if self.npc_dim_bottleneck is not None:
            raise ValueError(f"npc dim_bottleneck={self.npc_dim_bottleneck} is not built: the last state would have another width")
        if not 1 <= self.npc_blocks <= 8:
            raise ValueError(f"npc n_blocks must be 1..8, got {self.npc_blocks}")
        k = self.npc_kernel_size
        if k < 1 or k % 2 == 0:
            raise ValueError(f"npc kernel_size must be odd, got {k}")
        if self.npc_mask_size < 1 or self.npc_mask_size % 2 == 0:
            raise ValueError(f"npc mask_size must be odd, got {self.npc_mask_size}")
        if k > 63:
            raise ValueError(f"npc kernel_size above 63 is not built, got {k}")
        for i in range(self.npc_blocks):
            if self.npc_has_mask(i) and k - self.npc_mask(i) <= 0:
                raise ValueError(f"npc mask leaves no tap in block {i} (mask {self.npc_mask(i)} of kernel_size {k})")
        if self.npc_activate not in ("relu", "tanh"):
            raise ValueError(f"npc activate={self.npc_activate!r} is not built: only 'relu' and 'tanh' (the reference implements nothing else)")
        if len(self.conv_layers) != 1:
            raise ValueError("npc: conv_layers carries the frame geometry as one (hidden, window, shift) entry (npc_config sets it)")
        H, size, shift = self.conv_layers[0]
        if H % 64 or not 64 <= H <= 1024:
            raise ValueError(f"npc hidden_size must be a multiple of 64, at most 1024, got {H}")
        if (size, shift) != (int(16000 * self.apc_frame_length * 0.001), int(16000 * self.apc_frame_shift * 0.001)):
            raise ValueError("npc: conv_layers does not match frame_length / frame_shift (npc_config sets it)")
        if size < 4 or shift < 4 or size % 4 or shift % 4:
            raise ValueError(f"npc frame_length / frame_shift of {size} / {shift} samples are not built: both must be a multiple of 4 "
                             "samples (the front end's GEMM reads 16-byte vectors)")
        if self.apc_feat_dim % 16 or not 16 <= self.apc_feat_dim <= 256:
            raise ValueError(f"npc feat_dim must be a multiple of 16, at most 256 (a tap is a whole number of 64-byte K steps), got "
                             f"{self.apc_feat_dim}")
        states = self.npc_blocks + 2 if self.npc_disable_cross_layer else 2 * self.npc_blocks + 1
        if self.encoder_layers != states - 1 or self.encoder_embed_dim != H:
            raise ValueError("npc: encoder_layers / encoder_embed_dim must be the number of states - 1 / hidden_size (npc_config sets them)")

    @property
    def vg_pools(self) -> int:
        return sum(1 for _, pool in self.vg_layers if pool)

    def vg_seq_index(self, i: int) -> int:
        """Index of conv layer ``i`` in the reference's ``nn.Sequential`` (vggish.py:123-133): a conv and its ReLU count two, a
        pool one — 0, 3, 6, 8, 11, 13 at the released shape."""
        return sum(2 + int(pool) for _, pool in self.vg_layers[:i])

    @property
    def vg_min_samples(self) -> int:
        """The shortest utterance that yields one example (15600 at the released shape)."""
        return self.conv_layers[0][1] + (self.vg_example_frames - 1) * self.conv_layers[0][2]

    def _validate_vggish(self) -> None:
        """What the HIP path builds of VGGish; everything else is refused by name (s3enc_create_vggish repeats it)."""
        if not 1 <= len(self.vg_layers) <= 8:
            raise ValueError(f"vggish needs 1..8 conv layers, got {len(self.vg_layers)}")
        for i, (ch, _) in enumerate(self.vg_layers):
            if ch % 16 or not 16 <= ch <= 4096:
                raise ValueError(f"vggish channels of layer {i} must be a multiple of 16, at most 4096 (a tap is a whole number of "
                                 f"64-byte K steps), got {ch}")
        div = 1 << self.vg_pools
        if self.vg_example_frames < 1 or self.vg_example_frames % div:
            raise ValueError(f"vggish example_frames {self.vg_example_frames} is not divisible by 2^pools = {div}")
        if self.vg_num_mel_bins < 1 or self.vg_num_mel_bins % div:
            raise ValueError(f"vggish num_mel_bins {self.vg_num_mel_bins} is not divisible by 2^pools = {div}")
        if self.vg_example_hop != self.vg_example_frames:
            raise ValueError(f"vggish example_hop {self.vg_example_hop} is not built: only example_hop = example_frames "
                             f"({self.vg_example_frames}), examples that do not overlap")
        if len(self.conv_layers) != 1:
            raise ValueError("vggish: conv_layers carries the frame geometry as one (embedding, window, shift) entry (vggish_config sets it)")
        D, size, shift = self.conv_layers[0]
        if size < 4 or shift < 4 or size % 4 or shift % 4 or size > 4096:
            raise ValueError(f"vggish window / shift of {size} / {shift} samples are not built: both must be a multiple of 4 samples "
                             "(the front end's GEMM reads 16-byte vectors)")
        if self.vg_n_fft != 1 << max(size - 1, 1).bit_length():
            raise ValueError(f"vggish n_fft must be the power of two at or above the window, got {self.vg_n_fft}")
        if not 0.0 <= self.vg_mel_min_hz < self.vg_mel_max_hz <= 8000.0:
            raise ValueError("vggish mel edges must satisfy 0 <= mel_min_hz < mel_max_hz <= 8000")
        if not self.vg_log_offset > 0:
            raise ValueError("vggish log_offset must be positive")
        if len(self.vg_fc) != 3 or any(int(f) % 4 or not 4 <= int(f) <= 16384 for f in self.vg_fc):
            raise ValueError(f"vggish needs three Linear widths that are multiples of 4, at most 16384, got {tuple(self.vg_fc)}")
        if self.vg_postprocess and not self.vg_quant_min < self.vg_quant_max:
            raise ValueError("vggish quantiser range must satisfy quant_min < quant_max")
        if D != self.vg_fc[2] or self.encoder_embed_dim != self.vg_fc[2] or self.encoder_layers != 0:
            raise ValueError("vggish: conv_dim / encoder_embed_dim must be the last Linear's width and encoder_layers 0 (vggish_config "
                             "sets them)")

    def _validate_byol_a(self) -> None:
        """What the HIP path builds of BYOL-A; everything else is refused by name (s3enc_create_byol_a repeats it)."""
        if len(self.conv_layers) != 1:
            raise ValueError("byol_a: conv_layers carries the segment geometry as one (feature_d, window, stride) entry (byol_a_config sets it)")
        d, window, stride = self.conv_layers[0]
        if d % 4 or not 4 <= d <= 16384:
            raise ValueError(f"byol_a feature_d must be a multiple of 4, at most 16384, got {d}")
        if window <= 512:
            raise ValueError(f"byol_a window of {window} samples is too short: a segment of at most 512 samples cannot be reflect-padded "
                             "by 512 (n_fft / 2)")
        if window < 1120:
            raise ValueError(f"byol_a window of {window} samples is too short: fewer than 8 frames (1120 samples), nothing survives "
                             "three 2 x 2 pools")
        if stride < 1:
            raise ValueError(f"byol_a stride must be at least one sample, got {stride}")
        if (window, stride) != (int(self.ba_window_secs * 16000), int(self.ba_stride_secs * 16000)):
            raise ValueError("byol_a: conv_layers does not match window_secs / stride_secs (byol_a_config sets it)")
        if not self.ba_norm_std > 0 or not self.ba_bn_eps > 0:
            raise ValueError("byol_a norm_std and bn_eps must be positive")
        if self.encoder_embed_dim != d or self.encoder_layers != 0:
            raise ValueError("byol_a: encoder_embed_dim must be feature_d and encoder_layers 0 (byol_a_config sets them)")

    def _validate_byol_s(self) -> None:
        """What the HIP path builds of BYOL-S; everything else is refused by name (s3enc_create_byol_s repeats it)."""
        if self.bs_network in ("cvt", "clstm"):
            raise ValueError(f"byol_s network {self.bs_network} is not built (default and resnetish are)")
        if self.bs_network not in ("default", "resnetish"):
            raise ValueError(f"unknown byol_s network {self.bs_network!r}")
        if self.bs_network == "resnetish":
            if self.bs_block != "basic":
                raise ValueError("byol_s Bottleneck blocks (resnetish50) are not built: BasicBlock layers only")
            if len(self.bs_blocks) != 4 or any(not 1 <= int(b) <= 64 for b in self.bs_blocks):
                raise ValueError(f"byol_s needs four layers of 1..64 BasicBlocks, got {tuple(self.bs_blocks)}")
        if len(self.conv_layers) != 1:
            raise ValueError("byol_s: conv_layers carries the window geometry as one (2048, window, step) entry (byol_s_config sets it)")
        d, window, step = self.conv_layers[0]
        if window <= 512:
            raise ValueError(f"byol_s window of {window} samples is too short: a window of at most 512 samples cannot be reflect-padded "
                             "by 512 (n_fft / 2)")
        if self.bs_network == "default" and window < 1120:
            raise ValueError(f"byol_s window of {window} samples is too short for the default network: fewer than 8 frames (1120 "
                             "samples), nothing survives three 2 x 2 pools")
        if step < 1:
            raise ValueError(f"byol_s step must be at least one sample, got {step}")
        if (window, step) != byol_s_samples(self.bs_window_secs, self.bs_hop_secs):
            raise ValueError("byol_s: conv_layers does not match window_secs / hop_secs (byol_s_config sets it)")
        if not self.bs_bn_eps > 0:
            raise ValueError("byol_s bn_eps must be positive")
        if d != 2048 or self.encoder_embed_dim != 2048 or self.encoder_layers != 0:
            raise ValueError("byol_s: the state is 2048 wide and encoder_layers 0 (byol_s_config sets them)")

    @property
    def ma_tokens_per_step(self) -> int:
        """V = feature_dim // kc: tokens per time step, and state rows are V * D wide (mae_ast/expert.py:51-53,94)."""
        return self.ma_feature_dim // self.ma_kc

    @property
    def ma_pos_rows(self) -> int:
        """Leading rows of ``enc_sine_pos_embed.pe`` that travel to the device."""
        return min(self.ma_max_token_length, 8192)

    def ma_key_counts(self, lengths) -> List[int]:
        """``kv_b = min(ceil(F_b / kt) * V, Ttok)`` of a batch (forward_padding_mask, mae_ast.py:305-325)."""
        V, Ttok = self.ma_tokens_per_step, self.num_frames(max(lengths)) * self.ma_tokens_per_step
        return [min(-(-self.conv_lengths(n)[-1] // self.ma_kt) * V, Ttok) for n in lengths]

    def _validate_ssast(self) -> None:
        """What the HIP path builds of SSAST; everything else is refused by name (s3enc_create_ssast repeats what it can see)."""
        D, H = self.encoder_embed_dim, self.encoder_attention_heads
        if not self.layer_norm_first:
            raise ValueError("ssast blocks are pre-LN (layer_norm_first must be True)")
        if H < 1 or D != 64 * H:
            raise ValueError(f"ssast embed_dim / heads must be 64 (the attention kernel's head width), got {D} / {H}")
        if self.encoder_layers < 1:
            raise ValueError("ssast encoder_layers must be positive")
        if self.encoder_ffn_embed_dim < 4 or self.encoder_ffn_embed_dim % 4:
            raise ValueError("ssast ffn dim must be a multiple of 4")
        if self.ss_fshape not in (16, 32, 64, 128):
            raise ValueError(f"ssast fshape must be 16, 32, 64 or 128 (the strided patch kernel's set), got {self.ss_fshape}")
        if not 1 <= self.ss_tshape <= 32:
            raise ValueError(f"ssast tshape must be 1..32 (the strided patch kernel's set), got {self.ss_tshape}")
        if self.ss_fstride < 2 or self.ss_fstride % 2 or self.ss_fstride > 128:
            raise ValueError(f"ssast fstride must be even, 2..128 (a patch row starts 8-byte aligned), got {self.ss_fstride}")
        if self.ss_tstride < 1:
            raise ValueError("ssast tstride must be positive")
        W = self.ss_window_samples
        if W < 400 or W % 4:
            raise ValueError(f"ssast window_secs={self.ss_window_secs!r} gives {W} samples: a window must be a multiple of 4 samples "
                             "and hold at least one 400-sample analysis window")
        if self.ss_target_length < self.ss_tshape:
            raise ValueError(f"ssast window_secs={self.ss_window_secs!r} gives {self.ss_target_length} image rows, fewer than one patch "
                             f"of {self.ss_tshape} frames")
        if self.ss_f_dim * self.ss_t_dim + 2 > 8192:
            raise ValueError("ssast windows of more than 8192 tokens are not built")
        pf, pt = self.ss_pretrain_grid
        if pf < 1 or pt < 1:
            raise ValueError("ssast p_input_fdim / p_input_tdim are smaller than one patch")
        if self.ss_f_dim < pf:
            raise ValueError(f"ssast f_dim {self.ss_f_dim} < p_f_dim {pf}: the reference's frequency cut of the position rows slices with "
                             "t_dim (ast_models.py:325-334) and is reached by neither released model; it is not built")
        if not self.ss_ln_eps > 0:
            raise ValueError("ssast ln_eps must be positive")
        if list(self.conv_layers) != [(D, 400, 160)]:
            raise ValueError("ssast: conv_layers carries the frame geometry as one (D, 400, 160) entry (ssast_config sets it)")

    def _validate_mae_ast(self) -> None:
        """What the HIP path builds of MAE-AST; everything else is refused by name (s3enc_create_mae_ast repeats what it can see)."""
        D, H = self.encoder_embed_dim, self.encoder_attention_heads
        if self.ma_enc_conv_pos:
            raise ValueError("mae_ast enc_conv_pos=True is not built (no released checkpoint uses the convolutional position embedding)")
        if not self.ma_enc_sine_pos:
            raise ValueError("mae_ast enc_sine_pos=False is not built (the released checkpoints add the sinusoidal table)")
        if (self.ma_stride_t, self.ma_stride_c) != (self.ma_kt, self.ma_kc):
            raise ValueError(f"mae_ast kernel stride ({self.ma_stride_t}, {self.ma_stride_c}) must equal the kernel size "
                             f"({self.ma_kt}, {self.ma_kc}) on both axes")
        if self.ma_feature_dim != 128:
            raise ValueError(f"mae_ast feature_dim must be 128 (the reference's padding-mask rule hard-codes 128 mel bins), got {self.ma_feature_dim}")
        if self.ma_kc not in (16, 32, 64, 128):
            raise ValueError(f"mae_ast ast_kernel_size_chan must be 16, 32, 64 or 128 (the patch kernel's set), got {self.ma_kc}")
        if not 1 <= self.ma_kt <= 32:
            raise ValueError(f"mae_ast ast_kernel_size_time must be 1..32 (the patch kernel's set), got {self.ma_kt}")
        if self.ma_sample_rate != 16000:
            raise ValueError(f"mae_ast sample_rate must be 16000, got {self.ma_sample_rate}")
        if H < 1 or D != 64 * H:
            raise ValueError(f"mae_ast encoder_embed_dim / encoder_attention_heads must be 64 (the attention kernel's head width), got {D} / {H}")
        if self.ma_activation != "gelu":
            raise ValueError(f"mae_ast activation_fn={self.ma_activation!r} is not built: only 'gelu'")
        if self.encoder_layers < 1:
            raise ValueError("mae_ast encoder_layers must be positive")
        if self.encoder_ffn_embed_dim % 4 or self.encoder_ffn_embed_dim < 4:
            raise ValueError("mae_ast encoder_ffn_embed_dim must be a multiple of 4")
        if self.ma_max_token_length < 1 or not self.ma_bn_eps > 0:
            raise ValueError("mae_ast max_token_length and the BatchNorm eps must be positive")
        if self.conv_layers != [(D, 400, 160)]:
            raise ValueError("mae_ast: conv_layers carries the frame geometry as one (D, 400, 160) entry (mae_ast_config sets it)")

    def _validate_decoar(self) -> None:
        """What the HIP path builds of DeCoAR; everything else is refused by name (s3enc_create_decoar repeats it)."""
        H = self.decoar_hidden
        if not 1 <= self.decoar_layers <= 4:
            raise ValueError(f"decoar num_layers must be 1..4, got {self.decoar_layers}")
        if H % 64 or not 64 <= H <= 1024:
            raise ValueError(f"decoar hidden must be a multiple of 64, at most 1024 (the batch-shared recurrent kernel's limit), got {H}")
        if self.decoar_subsample not in (1, 2):
            raise ValueError(f"decoar subsample must be 1 or 2, got {self.decoar_subsample}")
        if self.decoar_feat_dim % 4 or not 4 <= self.decoar_feat_dim <= 256:
            raise ValueError(f"decoar num_mel_bins must be a multiple of 4, at most 256, got {self.decoar_feat_dim}")
        if len(self.conv_layers) != 1:
            raise ValueError("decoar: conv_layers carries the frame geometry as one (2 * hidden, window, shift) entry (decoar_config sets it)")
        D, size, shift = self.conv_layers[0]
        if (size, shift) != (int(16000 * self.decoar_frame_length * 0.001), int(16000 * self.decoar_frame_shift * 0.001)):
            raise ValueError("decoar: conv_layers does not match frame_length / frame_shift (decoar_config sets it)")
        if size < 4 or shift < 4 or size % 4 or shift % 4:
            raise ValueError(f"decoar frame_length / frame_shift of {size} / {shift} samples are not built: both must be a multiple of 4 "
                             "samples (the front end's GEMM reads 16-byte vectors)")
        if D != 2 * H or self.encoder_embed_dim != 2 * H or self.encoder_layers != (self.decoar_layers - 1 if self.decoar_per_layer else 0):
            raise ValueError("decoar: conv_dim / encoder_embed_dim must be 2 * hidden and encoder_layers the number of states - 1 "
                             "(decoar_config sets them)")

    def _validate_mockingjay(self) -> None:
        """What the HIP path builds of the Mockingjay configuration; everything else is refused by name (s3enc_create_mockingjay
        repeats it)."""
        D, H = self.encoder_embed_dim, self.encoder_attention_heads
        if self.mj_pre_layer_norm:
            raise ValueError("mockingjay pre_layer_norm=True is not built (no released checkpoint uses it)")
        if self.mj_hidden_act != "gelu":
            raise ValueError(f"mockingjay hidden_act={self.mj_hidden_act!r} is not built: only 'gelu'")
        if H < 1 or D != 64 * H:
            raise ValueError(f"mockingjay hidden_size / num_attention_heads must be 64 (the attention kernel's head width), got {D} / {H}")
        if self.encoder_layers < 1:
            raise ValueError("mockingjay num_hidden_layers must be positive")
        if self.encoder_ffn_embed_dim % 4 or self.encoder_ffn_embed_dim < 4:
            raise ValueError("mockingjay intermediate_size must be a multiple of 4")
        if self.mj_input_dim % 4 or self.mj_input_dim < 4:
            raise ValueError(f"mockingjay input_dim must be a multiple of 4 (the GEMM reads 16-byte vectors), got {self.mj_input_dim}")
        if self.mj_sequence_length < 0:
            raise ValueError("mockingjay sequence_length must not be negative")
        if not 0.0 <= self.mj_layer_norm_eps <= 1.0:
            raise ValueError("mockingjay layer_norm_eps out of range")
        if self.mj_frontend not in ("mel", "kaldi"):
            raise ValueError(f"mockingjay front end {self.mj_frontend!r}: 'mel' or 'kaldi'")
        if self.mj_frontend == "mel":
            if self.mj_input_dim > 256:
                raise ValueError("mockingjay n_mels above 256 is not built")
            want = [(D, 0, 160)]
        else:
            size, shift = int(16000 * self.mj_kaldi_frame_length * 0.001), int(16000 * self.mj_kaldi_frame_shift * 0.001)
            if shift != 160 or size % 4 or size < 4:
                raise ValueError("mockingjay kaldi front end: a 10 ms frame shift and a window that is a multiple of 4 samples")
            if not 0 <= self.mj_delta_order <= 2 or self.mj_delta_win < 3 or self.mj_delta_win % 2 == 0:
                raise ValueError("mockingjay kaldi front end: delta order 0..2 and an odd win_length >= 3")
            if self.mj_input_dim != self.mj_kaldi_mel_bins * (self.mj_delta_order + 1):
                raise ValueError("mockingjay input_dim must be num_mel_bins * (delta order + 1)")
            want = [(D, size, 160)]
        if [tuple(x) for x in self.conv_layers] != want:
            raise ValueError("mockingjay: conv_layers carries the frame geometry as one (hidden, window, 160) entry (mockingjay_config sets it)")

    def to_dict(self) -> Dict:
        return asdict(self)


_MODEL_KEYS = (
    "extractor_mode", "conv_bias", "encoder_layers", "encoder_embed_dim", "encoder_ffn_embed_dim",
    "encoder_attention_heads", "layer_norm_first", "conv_pos", "conv_pos_groups",
)
_WAVLM_KEYS = ("relative_position_embedding", "num_buckets", "max_distance", "gru_rel_pos", "normalize")


# DeCoAR 2.0's front end as a one-layer "conv stack": (mel bins, analysis window, frame shift in samples) — the family's own constants
# (decoar2/audio.py: kaldi.fbank's 80 bins, 25 ms / 10 ms at 16 kHz, hamming; CMVN eps 1e-10; every second frame)
DECOAR2_FRONT_END = (80, 400, 160)


def decoar2_config(embed_dim: int = 768, ffn_dim: int = 3072, layers: int = 12, conv_pos: int = 128, conv_pos_groups: int = 16) -> "EncoderConfig":
    """An :class:`EncoderConfig` of family "decoar2" (decoar2/decoar2.py:9-24 hard-codes 768 / 3072 / 12 / 128 / 16).  Heads are
    embed_dim / 64: the head count cannot be read from a tensor and the released shape is 768 / 12."""
    D = int(embed_dim)
    if D % 64:
        raise ValueError(f"decoar2: embed_dim must be a multiple of 64 (heads are embed_dim / 64), got {D}")
    if int(conv_pos_groups) < 1 or D % int(conv_pos_groups) or D // int(conv_pos_groups) not in (24, 32, 40, 48, 64):
        raise ValueError("decoar2: embed_dim / conv_pos_groups (the positional conv's group width) must be 32, 48 or 64 (fp32: also 24 "
                         f"or 40), got {D} / {conv_pos_groups}")
    cfg = EncoderConfig(family="decoar2", conv_layers=[DECOAR2_FRONT_END], extractor_mode="default", conv_bias=False, normalize=False,
                        encoder_layers=int(layers), encoder_embed_dim=D, encoder_ffn_embed_dim=int(ffn_dim),
                        encoder_attention_heads=D // 64, layer_norm_first=False, conv_pos=int(conv_pos),
                        conv_pos_groups=int(conv_pos_groups))
    cfg.validate()
    return cfg


def config_from_decoar2(sd) -> "EncoderConfig":
    """The configuration a DeCoAR 2.0 state dict implies: D, FFN, layers and the positional conv's K and G from the tensors' shapes."""
    def shape(name):
        if name not in sd:
            raise ValueError(f"decoar2: missing parameter {name}")
        return tuple(sd[name].shape)

    D, feat = shape("post_extract_proj.weight")
    if feat != DECOAR2_FRONT_END[0]:
        raise ValueError(f"decoar2: post_extract_proj reads {feat} features, the front end gives {DECOAR2_FRONT_END[0]} mel bins")
    v = shape("encoder.pos_conv.0.weight_v")
    if len(v) != 3 or v[0] != D or v[1] < 1 or D % v[1]:
        raise ValueError(f"decoar2: encoder.pos_conv.0.weight_v has shape {v}, expected ({D}, {D} / groups, kernel)")
    layers = 0
    while f"encoder.layers.{layers}.fc1.weight" in sd:
        layers += 1
    if layers < 1:
        raise ValueError("decoar2: missing parameter encoder.layers.0.fc1.weight")
    return decoar2_config(D, shape("encoder.layers.0.fc1.weight")[0], layers, v[2], D // v[1])


LIGHTHUBERT_SUPERNET = dict(embed_dim=768, ffn_embed=3072, heads_num=12, layer_num=12)  # the checkpoint's own width, hard-coded by the reference


def lighthubert_subnet(model_name: str, supernet_type: str) -> Dict:
    """The subnet the reference's expert runs (lighthubert/expert.py:38-42, lighthubert.py:199-272): for ``hubert_pruner`` the
    released subnet of the supernet type, for ``student_hubert`` the largest subnet of its search space."""
    if supernet_type not in ("base", "small"):
        raise ValueError(f"lighthubert: unknown supernet type {supernet_type!r}")
    if model_name == "hubert_pruner":
        embed = 640 if supernet_type == "base" else 384
    elif model_name == "student_hubert":
        embed = 768 if supernet_type == "base" else 512
    else:
        raise ValueError(f"lighthubert: cfg.model._name must be 'hubert_pruner' or 'student_hubert', got {model_name!r}")
    heads = embed // 64
    return dict(atten_dim=[embed] * 12, embed_dim=embed, ffn_embed=[4 * embed] * 12, heads_num=[heads] * 12, layer_num=12,
                slide_wsz=["global"] * 12)


def check_lighthubert_subnet(subnet: Dict) -> None:
    """What the HIP path builds of a subnet description; the rest is refused by name."""
    n = int(subnet["layer_num"])
    if n != 12:
        raise ValueError(f"lighthubert: a subnet of {n} layers is not built (the 10- and 11-layer depth maps drop supernet layers)")
    for key in ("atten_dim", "ffn_embed", "heads_num"):
        if len(set(subnet[key])) != 1 or len(subnet[key]) != n:
            raise ValueError(f"lighthubert: a subnet with non-uniform {key} is not built, got {list(subnet[key])}")
    if subnet["atten_dim"][0] != subnet["embed_dim"]:
        raise ValueError(f"lighthubert: a subnet with atten_dim != embed_dim is not built, got {subnet['atten_dim'][0]} / "
                         f"{subnet['embed_dim']}")
    if any(w != "global" for w in subnet.get("slide_wsz", ["global"])):
        raise ValueError("lighthubert: sliding-window attention (slide_wsz) is not built")


def config_from_lighthubert(model_cfg: Dict, subnet: Dict | None = None) -> EncoderConfig:
    """``checkpoint["cfg"]["model"]`` of a LightHuBERT file -> the configuration of the subnet its expert runs
    (lighthubert/expert.py:17-47; LightHuBERTConfig.update keeps only the keys it knows, lighthubert.py:341-428)."""
    name = model_cfg.get("_name")
    stype = str(model_cfg.get("supernet_type", "base")).lower()
    if name == "hubert_pruner":  # expert.py:24-36: the yaml's name decides, else the configured / default type stays
        yaml = str(model_cfg.get("pruner_supernet", "")).lower()
        stype = "small" if yaml.endswith("small.yaml") else "base" if yaml.endswith("base.yaml") else stype
    subnet = subnet or lighthubert_subnet(name, stype)
    check_lighthubert_subnet(subnet)
    for key, want in (("encoder_layers", 12), ("encoder_embed_dim", 768), ("encoder_ffn_embed_dim", 3072), ("encoder_attention_heads", 12)):
        if int(model_cfg.get(key, want)) != want:
            raise ValueError(f"lighthubert: the supernet is {want} for {key} (hard-coded by the reference), got {model_cfg[key]}")
    if str(model_cfg.get("layer_type", "transformer")) != "transformer":
        raise ValueError("lighthubert: only layer_type='transformer' exists in the reference")
    act = str(getattr(model_cfg.get("activation_fn", "gelu"), "name", model_cfg.get("activation_fn", "gelu")))
    if act != "gelu":
        raise ValueError(f"only activation_fn='gelu' is on the hot path, got {act!r}")
    cfg = EncoderConfig(
        family="lighthubert", lh_model=str(name), lh_supernet=stype, normalize=True,  # expert.py:56: F.layer_norm on every waveform
        extractor_mode=str(model_cfg.get("extractor_mode", "layer_norm")), conv_bias=bool(model_cfg.get("conv_bias", False)),
        conv_layers=parse_conv_layers(model_cfg.get("conv_feature_layers", DEFAULT_CONV_LAYERS)),
        encoder_layers=12, encoder_embed_dim=int(subnet["embed_dim"]), encoder_ffn_embed_dim=int(subnet["ffn_embed"][0]),
        encoder_attention_heads=int(subnet["heads_num"][0]), layer_norm_first=bool(model_cfg.get("layer_norm_first", False)),
        conv_pos=int(model_cfg.get("conv_pos", 128)), conv_pos_groups=int(model_cfg.get("conv_pos_groups", 16)),
        pos_conv_depth=int(model_cfg.get("pos_conv_depth", 1) or 1))
    cfg.validate()
    return cfg


def config_from_dicts(family: str, model_cfg: Dict, task_cfg: Dict | None = None) -> EncoderConfig:
    """Build an :class:`EncoderConfig` from the dicts stored in a converted checkpoint (§3.4)."""
    cfg = EncoderConfig(family=family)
    for k in _MODEL_KEYS:
        if k in model_cfg and model_cfg[k] is not None:
            setattr(cfg, k, type(getattr(cfg, k))(model_cfg[k]))
    if "conv_feature_layers" in model_cfg:
        cfg.conv_layers = parse_conv_layers(model_cfg["conv_feature_layers"])
    act = model_cfg.get("activation_fn", "gelu")
    act = getattr(act, "name", act)
    if str(act) != "gelu" and not str(model_cfg.get("layer_type", "")).endswith("conformer"):
        raise ValueError(f"only activation_fn='gelu' is on the hot path, got {act!r}")
    layer_type = str(getattr(model_cfg.get("layer_type", "transformer"), "name", model_cfg.get("layer_type", "transformer")))
    if layer_type.endswith("conformer"):  # a str, or a fairseq ChoiceEnum member whose str() is "LAYER_TYPE_CHOICES.conformer"
        if family != "wav2vec2":
            raise ValueError("conformer layers are a wav2vec2-family encoder")
        cfg.layer_type = "conformer"
        cfg.pos_enc_type = str(model_cfg.get("pos_enc_type", "abs"))
        cfg.attn_type = str(model_cfg.get("attn_type", "") or "")
        cfg.depthwise_conv_kernel_size = int(model_cfg.get("depthwise_conv_kernel_size", 31))
    cfg.pos_conv_depth = int(model_cfg.get("pos_conv_depth", 1) or 1)
    if cfg.pos_conv_depth > 1 and family != "wav2vec2":
        raise ValueError("pos_conv_depth > 1 is the data2vec-audio encoder (wav2vec2 family)")
    if family == "wavlm":
        for k in _WAVLM_KEYS:
            if k in model_cfg:
                setattr(cfg, k, type(getattr(cfg, k))(model_cfg[k]))
    else:
        if task_cfg is not None and "normalize" in task_cfg:
            cfg.normalize = bool(task_cfg["normalize"])
    cfg.validate()
    return cfg


_W2V_KEYS = ("aggregator", "activation", "log_compression", "skip_connections_feat", "skip_connections_agg", "residual_scale",
             "non_affine_group_norm", "no_conv_bias", "agg_zero_pad", "vq_type", "vq_vars", "vq_groups", "vq_dim", "vq_depth",
             "combine_groups")
# Wav2VecConfig defaults (wav2vec_model.py:307-318)
W2V_DEFAULT_FEATURE_LAYERS = "[(512, 10, 5), (512, 8, 4), (512, 4, 2), (512, 4, 2), (512, 4, 2), (512, 1, 1), (512, 1, 1), (512, 1, 1)]"
W2V_DEFAULT_AGG_LAYERS = "[" + ", ".join(f"(512, {k}, 1)" for k in range(2, 14)) + "]"


def wav2vec_config(conv_layers, agg_layers, **flags) -> EncoderConfig:
    """An :class:`EncoderConfig` of family "wav2vec": the Transformer fields mirror the aggregator."""
    conv_layers, agg_layers = parse_conv_layers(conv_layers), parse_conv_layers(agg_layers)
    cfg = EncoderConfig(family="wav2vec", conv_layers=conv_layers, agg_layers=agg_layers, encoder_layers=len(agg_layers),
                        encoder_embed_dim=conv_layers[-1][0], **flags)
    cfg.validate()
    return cfg


def config_from_wav2vec(model_cfg: Dict, task_cfg: Dict | None = None) -> EncoderConfig:
    """``Wav2VecConfig`` (upstream/wav2vec/wav2vec_model.py:289-410) from a converted checkpoint's ``model_cfg``; keys the forward
    does not read are dropped, missing ones take the reference defaults (``merge_with_parent``)."""
    flags = {}
    proto = EncoderConfig()
    for k in _W2V_KEYS:
        if k in model_cfg and model_cfg[k] is not None:
            v = model_cfg[k]
            v = getattr(v, "name", v)  # fairseq ChoiceEnum members
            d = getattr(proto, k)
            flags[k] = str(v) if isinstance(d, str) else type(d)(v)
    if flags.get("vq_type") in ("None",):
        flags["vq_type"] = "none"
    return wav2vec_config(model_cfg.get("conv_feature_layers", W2V_DEFAULT_FEATURE_LAYERS),
                          model_cfg.get("conv_aggregator_layers", W2V_DEFAULT_AGG_LAYERS), **flags)


# cpc_default_config.py: the arguments the forward reads, at their defaults
CPC_DEFAULTS = dict(hiddenEncoder=256, hiddenGar=256, arMode="LSTM", nLevelsGRU=1, normMode="layerNorm", encoder_type="cpc",
                    cpc_mode=None, samplingType="samespeaker")


def cpc_config(hidden: int = 256, ar_mode: str = "LSTM", ar_layers: int = 1, ar_hidden: int | None = None, **flags) -> EncoderConfig:
    """An :class:`EncoderConfig` of family "cpc" (CPCEncoder's five convolutions, cpc/model.py:84-93)."""
    C = int(hidden)
    cfg = EncoderConfig(family="cpc", conv_layers=[(C, 10, 5), (C, 8, 4), (C, 4, 2), (C, 4, 2), (C, 4, 2)], conv_pads=[3, 2, 1, 1, 1],
                        conv_bias=True, encoder_layers=1, encoder_embed_dim=C, ar_mode=str(ar_mode), ar_layers=int(ar_layers),
                        ar_hidden=int(C if ar_hidden is None else ar_hidden), **flags)
    cfg.validate()
    return cfg


def config_from_cpc(config: Dict) -> EncoderConfig:
    """The checkpoint's ``config`` dict over the defaults, exactly as ``loadArgs`` merges them (cpc/expert.py:29-31)."""
    a = dict(CPC_DEFAULTS)
    a.update({k: v for k, v in config.items() if k in CPC_DEFAULTS})
    if a["encoder_type"] != "cpc":
        raise ValueError(f"cpc encoder_type={a['encoder_type']!r} is not built: only 'cpc' (the convolutional encoder)")
    return cpc_config(a["hiddenEncoder"], a["arMode"], a["nLevelsGRU"], a["hiddenGar"], norm_mode=str(a["normMode"]),
                      cpc_reverse=a["cpc_mode"] == "reverse", cpc_keep_hidden=a["samplingType"] == "sequential")


def apc_config(hidden: int = 512, num_layers: int = 3, residual: bool = True, feat_dim: int = 80, frame_length: float = 25.0,
               frame_shift: float = 10.0, cmvn: bool = True, vq: Dict | None = None, **flags) -> EncoderConfig:
    """An :class:`EncoderConfig` of family "apc" (apc/apc.py:27-71, apc/audio.py:107-115)."""
    H = int(hidden)
    size, shift = int(16000 * float(frame_length) * 0.001), int(16000 * float(frame_shift) * 0.001)
    cfg = EncoderConfig(family="apc", conv_layers=[(H, size, shift)], encoder_layers=2, encoder_embed_dim=H,
                        apc_feat_dim=int(feat_dim), apc_frame_length=float(frame_length), apc_frame_shift=float(frame_shift),
                        apc_cmvn=bool(cmvn), apc_layers=int(num_layers), apc_residual=bool(residual),
                        apc_vq=None if vq is None else dict(vq), **flags)
    cfg.validate()
    return cfg


def config_from_apc(config: Dict) -> EncoderConfig:
    """The checkpoint's ``config``: ``data.audio`` as ``create_transform`` reads it (apc/audio.py:107-115: feat_type, feat_dim,
    decode_wav and cmvn are popped, the rest goes to ``kaldi.fbank``) and ``model.paras`` as ``APC(feat_dim, **paras)`` does."""
    audio = dict(config["data"]["audio"])
    feat_type, feat_dim = audio.pop("feat_type"), audio.pop("feat_dim")
    audio.pop("decode_wav", None)  # how a FILE is read; the upstream is handed waveforms
    cmvn = audio.pop("cmvn", True)
    frame_length, frame_shift = audio.pop("frame_length", 25.0), audio.pop("frame_shift", 10.0)
    if audio:
        raise ValueError(f"apc audio options {sorted(audio)} are not built: only frame_length / frame_shift reach kaldi.fbank here")
    paras = dict(config["model"]["paras"])
    for key in ("hidden_size", "num_layers", "residual"):
        if key not in paras:
            raise ValueError(f"apc checkpoint: model.paras.{key} is missing")
    return apc_config(paras["hidden_size"], paras["num_layers"], paras["residual"], feat_dim, frame_length, frame_shift, cmvn,
                      paras.get("vq"), apc_feat_type=str(feat_type))


def npc_config(hidden: int = 512, n_blocks: int = 4, kernel_size: int = 15, mask_size: int = 5, residual: bool = True,
               batch_norm: bool = True, activate: str = "relu", disable_cross_layer: bool = False, feat_dim: int = 80,
               frame_length: float = 25.0, frame_shift: float = 10.0, cmvn: bool = True, vq: Dict | None = None,
               dim_bottleneck: int | None = None, **flags) -> EncoderConfig:
    """An :class:`EncoderConfig` of family "npc" (npc/npc.py:99-171, npc/audio.py:107-115)."""
    H, nb = int(hidden), int(n_blocks)
    size, shift = int(16000 * float(frame_length) * 0.001), int(16000 * float(frame_shift) * 0.001)
    cfg = EncoderConfig(family="npc", conv_layers=[(H, size, shift)], encoder_layers=nb + 1 if disable_cross_layer else 2 * nb,
                        encoder_embed_dim=H, apc_feat_dim=int(feat_dim), apc_frame_length=float(frame_length),
                        apc_frame_shift=float(frame_shift), apc_cmvn=bool(cmvn), npc_blocks=nb, npc_kernel_size=int(kernel_size),
                        npc_mask_size=int(mask_size), npc_residual=bool(residual), npc_batch_norm=bool(batch_norm),
                        npc_activate=str(activate), npc_disable_cross_layer=bool(disable_cross_layer),
                        npc_vq=None if vq is None else dict(vq),
                        npc_dim_bottleneck=None if dim_bottleneck is None else int(dim_bottleneck), **flags)
    cfg.validate()
    return cfg


def config_from_npc(config: Dict) -> EncoderConfig:
    """The checkpoint's ``config``: ``data.audio`` as ``create_transform`` reads it (npc/audio.py:107-115) and ``model.paras`` as
    ``NPC(feat_dim, **paras)`` does (npc/npc.py:99-113: batch_norm, activate, disable_cross_layer, vq and dim_bottleneck have
    defaults)."""
    audio = dict(config["data"]["audio"])
    feat_type, feat_dim = audio.pop("feat_type"), audio.pop("feat_dim")
    audio.pop("decode_wav", None)  # how a FILE is read; the upstream is handed waveforms
    cmvn = audio.pop("cmvn", True)
    frame_length, frame_shift = audio.pop("frame_length", 25.0), audio.pop("frame_shift", 10.0)
    if audio:
        raise ValueError(f"npc audio options {sorted(audio)} are not built: only frame_length / frame_shift reach kaldi.fbank here")
    paras = dict(config["model"]["paras"])
    for key in ("hidden_size", "n_blocks", "residual", "kernel_size", "mask_size"):
        if key not in paras:
            raise ValueError(f"npc checkpoint: model.paras.{key} is missing")
    return npc_config(paras["hidden_size"], paras["n_blocks"], paras["kernel_size"], paras["mask_size"], paras["residual"],
                      paras.get("batch_norm", True), paras.get("activate", "relu"), paras.get("disable_cross_layer", False),
                      feat_dim, frame_length, frame_shift, cmvn, paras.get("vq"), paras.get("dim_bottleneck"),
                      apc_feat_type=str(feat_type))


def vggish_config(layers=None, fc=(4096, 4096, 128), example_frames: int = 96, num_mel_bins: int = 64, postprocess: bool = True,
                  window: int = 400, shift: int = 160, mel_min_hz: float = 125.0, mel_max_hz: float = 7500.0,
                  log_offset: float = 0.01, example_hop: int | None = None, quant_min: float = -2.0, quant_max: float = 2.0,
                  **flags) -> EncoderConfig:
    """An :class:`EncoderConfig` of family "vggish" (vggish/vggish.py:18-41,123-133, vggish_params.py).  ``layers``: (channels,
    pool behind it) per conv layer, or the reference's ``make_layers`` list with ``"M"`` entries; default: the released shape."""
    if layers is None:
        layers = [64, "M", 128, "M", 256, 256, "M", 512, 512, "M"]
    if all(v == "M" or isinstance(v, int) for v in layers):
        if layers[0] == "M" or any(a == "M" and b == "M" for a, b in zip(layers, layers[1:])):
            raise ValueError("vggish layers: every 'M' must follow a conv layer")
        pairs = []
        for v in layers:
            if v == "M":
                pairs[-1] = (pairs[-1][0], True)
            else:
                pairs.append((int(v), False))
    else:
        pairs = [(int(c), bool(p)) for c, p in layers]
    fc = tuple(int(f) for f in fc)
    size, sh = int(window), int(shift)
    cfg = EncoderConfig(family="vggish", conv_layers=[(fc[-1], size, sh)], encoder_layers=0, encoder_embed_dim=fc[-1],
                        vg_num_mel_bins=int(num_mel_bins), vg_n_fft=1 << max(size - 1, 1).bit_length(),
                        vg_mel_min_hz=float(mel_min_hz), vg_mel_max_hz=float(mel_max_hz), vg_log_offset=float(log_offset),
                        vg_example_frames=int(example_frames),
                        vg_example_hop=int(example_frames if example_hop is None else example_hop), vg_layers=pairs, vg_fc=fc,
                        vg_postprocess=bool(postprocess), vg_quant_min=float(quant_min), vg_quant_max=float(quant_max), **flags)
    cfg.validate()
    return cfg


def byol_s_samples(window_secs: float, hop_secs: float) -> Tuple[int, int]:
    """(window, step) in samples, with the reference's own expressions: expert.py:22-23 turns the seconds into milliseconds,
    serab.py:151-153 and utils.py:72,79 turn those into samples."""
    frame_duration, hop_size = window_secs * 1000, hop_secs * 1000
    return int((frame_duration / 1000) * 16000), int(hop_size / 1000.0 * 16000)


def byol_s_config(network: str = "default", blocks=(3, 4, 6, 3), window_secs: float = 1, hop_secs: float = 0.05, block: str = "basic",
                  **flags) -> EncoderConfig:
    """An :class:`EncoderConfig` of family "byol_s" (byol_s/expert.py:12-28).  The samples, not the seconds, travel through the ABI."""
    window, step = byol_s_samples(window_secs, hop_secs)
    cfg = EncoderConfig(family="byol_s", conv_layers=[(2048, window, step)], encoder_layers=0, encoder_embed_dim=2048,
                        bs_network=str(network), bs_blocks=tuple(int(b) for b in blocks), bs_block=str(block),
                        bs_window_secs=float(window_secs), bs_hop_secs=float(hop_secs), **flags)
    cfg.validate()
    return cfg


def byol_a_config(feature_d: int = 2048, window_secs: float = 1.0, stride_secs: float = 1.0, **flags) -> EncoderConfig:
    """An :class:`EncoderConfig` of family "byol_a" (byol_a/expert.py:27-65).  The two ``int(secs * 16000)`` are the reference's own
    expressions: the samples, not the seconds, travel through the ABI."""
    window, stride = int(window_secs * 16000), int(stride_secs * 16000)
    cfg = EncoderConfig(family="byol_a", conv_layers=[(int(feature_d), window, stride)], encoder_layers=0,
                        encoder_embed_dim=int(feature_d), ba_window_secs=float(window_secs), ba_stride_secs=float(stride_secs), **flags)
    cfg.validate()
    return cfg


def mae_ast_config(kt: int = 16, kc: int = 16, embed_dim: int = 768, layers: int = 12, heads: int = 12, ffn: int = 3072,
                   layer_norm_first: bool = False, max_token_length: int = 48000, stride_t: int = None, stride_c: int = None,
                   feature_dim: int = 128, sample_rate: int = 16000, **flags) -> EncoderConfig:
    """An :class:`EncoderConfig` of family "mae_ast" (mae_ast/mae_ast.py:35-199; the defaults are ``mae_ast_patch``)."""
    cfg = EncoderConfig(family="mae_ast", conv_layers=[(int(embed_dim), 400, 160)], encoder_layers=int(layers),
                        encoder_embed_dim=int(embed_dim), encoder_ffn_embed_dim=int(ffn), encoder_attention_heads=int(heads),
                        layer_norm_first=bool(layer_norm_first), ma_kt=int(kt), ma_kc=int(kc),
                        ma_stride_t=int(kt if stride_t is None else stride_t), ma_stride_c=int(kc if stride_c is None else stride_c),
                        ma_feature_dim=int(feature_dim), ma_sample_rate=int(sample_rate), ma_max_token_length=int(max_token_length),
                        **flags)
    cfg.validate()
    return cfg


SSAST_SIZES = {"tiny": (192, 3), "small": (384, 6), "base": (768, 12)}  # timm's deit_{tiny,small,base}_distilled_patch16: D, heads
SSAST_TYPES = {"p": (16, 16, 10, 10), "f": (128, 2, 128, 1)}            # fshape, tshape, fstride, tstride (ssast/expert.py:51-78)


def ssast_config(model_type: str = "p", model_size: str = "base", window_secs: float = 1.0, embed_dim: int = None, heads: int = None,
                 layers: int = 12, ffn: int = None, p_input_fdim: int = 128, p_input_tdim: int = 1024, **flags) -> EncoderConfig:
    """An :class:`EncoderConfig` of family "ssast": ``model_type`` "p" (patch) or "f" (frame), ``model_size`` of SSAST_SIZES (or
    ``embed_dim`` / ``heads`` given), ``window_secs`` the expert's constructor argument.  The defaults are ``ssast_patch_base``."""
    if model_type not in SSAST_TYPES:
        raise ValueError(f"ssast model type must be 'p' or 'f', got {model_type!r}")
    if embed_dim is None:
        if model_size not in SSAST_SIZES:
            raise ValueError(f"ssast model size must be one of {sorted(SSAST_SIZES)}, got {model_size!r}")
        embed_dim, heads = SSAST_SIZES[model_size]
    fshape, tshape, fstride, tstride = SSAST_TYPES[model_type]
    cfg = EncoderConfig(family="ssast", conv_layers=[(int(embed_dim), 400, 160)], encoder_layers=int(layers),
                        encoder_embed_dim=int(embed_dim), encoder_ffn_embed_dim=int(4 * embed_dim if ffn is None else ffn),
                        encoder_attention_heads=int(heads), layer_norm_first=True, ss_fshape=fshape, ss_tshape=tshape,
                        ss_fstride=fstride, ss_tstride=tstride, ss_window_secs=float(window_secs), ss_p_input_fdim=int(p_input_fdim),
                        ss_p_input_tdim=int(p_input_tdim), **flags)
    cfg.validate()
    return cfg


def config_from_mae_ast(model_cfg: Dict, task_cfg: Dict) -> EncoderConfig:
    """``checkpoint["cfg"]["model"]`` / ``["task"]`` of an MAE-AST file (mae_ast/expert.py:28-50); a missing model key takes the
    default of ``MAE_AST_Config``."""
    m, t = dict(model_cfg), dict(task_cfg)
    for key in ("feature_dim", "sample_rate"):
        if key not in t:
            raise ValueError(f"mae_ast checkpoint: cfg.task has no {key!r}")
    kt, kc = int(m.get("ast_kernel_size_time", 16)), int(m.get("ast_kernel_size_chan", 16))
    return mae_ast_config(kt=kt, kc=kc, embed_dim=m.get("encoder_embed_dim", 768), layers=m.get("encoder_layers", 12),
                          heads=m.get("encoder_attention_heads", 12), ffn=m.get("encoder_ffn_embed_dim", 3072),
                          layer_norm_first=m.get("layer_norm_first", False), max_token_length=m.get("max_token_length", 48000),
                          stride_t=m.get("ast_kernel_stride_time", 16), stride_c=m.get("ast_kernel_stride_chan", 16),
                          feature_dim=t["feature_dim"], sample_rate=t["sample_rate"],
                          ma_enc_sine_pos=bool(m.get("enc_sine_pos", False)), ma_enc_conv_pos=bool(m.get("enc_conv_pos", False)),
                          ma_activation=str(m.get("activation_fn", "gelu")), ma_decoder_layers=int(m.get("decoder_layers", 2)),
                          ma_dec_sine_pos=bool(m.get("dec_sine_pos", False)))


def decoar_config(hidden: int = 1024, num_layers: int = 4, per_layer: bool = False, feat_dim: int = 80, subsample: int = 1,
                  frame_length: float = 25.0, frame_shift: float = 10.0, **flags) -> EncoderConfig:
    """An :class:`EncoderConfig` of family "decoar" (decoar/decoar.py:9-39: the reference hard-codes 80 / 1024 / 4)."""
    H = int(hidden)
    size, shift = int(16000 * float(frame_length) * 0.001), int(16000 * float(frame_shift) * 0.001)
    cfg = EncoderConfig(family="decoar", conv_layers=[(2 * H, size, shift)], encoder_embed_dim=2 * H,
                        encoder_layers=int(num_layers) - 1 if per_layer else 0, decoar_feat_dim=int(feat_dim), decoar_hidden=H,
                        decoar_layers=int(num_layers), decoar_frame_length=float(frame_length),
                        decoar_frame_shift=float(frame_shift), decoar_subsample=int(subsample), decoar_per_layer=bool(per_layer),
                        **flags)
    cfg.validate()
    return cfg


def mockingjay_config(hidden: int = 768, layers: int = 3, heads: int = 12, intermediate: int = 3072, input_dim: int = 80,
                      frontend: str = "mel", sequence_length: int = 1500, share_layer: bool = False, layer_norm_eps: float = 1e-12,
                      cmvn: bool = True, target_level: float = -25.0, **flags) -> EncoderConfig:
    """An :class:`EncoderConfig` of family "mockingjay" (mockingjay/model.py:25-41, builder.py:96-122)."""
    cfg = EncoderConfig(family="mockingjay", encoder_layers=int(layers), encoder_embed_dim=int(hidden),
                        encoder_ffn_embed_dim=int(intermediate), encoder_attention_heads=int(heads), mj_input_dim=int(input_dim),
                        mj_frontend=frontend, mj_sequence_length=int(sequence_length), mj_share_layer=bool(share_layer),
                        mj_layer_norm_eps=float(layer_norm_eps), mj_cmvn=bool(cmvn), mj_target_level=float(target_level), **flags)
    if frontend == "kaldi":
        window = int(16000 * cfg.mj_kaldi_frame_length * 0.001)
    else:
        window = 0
    cfg.conv_layers = [(int(hidden), window, 160)]
    cfg.validate()
    return cfg


def config_from_mockingjay(config: Dict) -> EncoderConfig:
    """The checkpoint's ``Upstream_Config`` (legacy: ``Config``): ``transformer`` as ``TransformerConfig`` reads it
    (mockingjay/model.py:25-41), ``task.sequence_length`` and the ``audio`` block as ``TransformerBuilder`` does
    (builder.py:100-114): ``audio.kaldi`` -> baseline/extracter.py, otherwise ``audio.input`` -> OnlinePreprocessor."""
    for key in ("transformer", "task"):
        if key not in config:
            raise ValueError(f"mockingjay checkpoint: the upstream config has no {key!r} block")
    if "audio" not in config:
        raise ValueError("mockingjay checkpoint: no `audio` block — the upstream expert only supports on-the-fly checkpoints with "
                         "a built-in feature extracter (upstream/mockingjay/expert.py:52-54)")
    t, audio = config["transformer"], config["audio"]
    flags = dict(mj_pre_layer_norm=bool(t.get("pre_layer_norm", False)), mj_hidden_act=str(t.get("hidden_act", "gelu")))
    if "kaldi" in audio:
        kaldi = audio["kaldi"]
        if kaldi.get("feat_type", "fbank") != "fbank":
            raise NotImplementedError(f"mockingjay audio.kaldi.feat_type={kaldi.get('feat_type')!r} is not built: only 'fbank'")
        fb = dict(kaldi.get("fbank", {}))
        if not fb.pop("use_log_fbank", True):
            raise NotImplementedError("mockingjay audio.kaldi.fbank.use_log_fbank=False is not built")
        flags.update(mj_kaldi_mel_bins=int(fb.pop("num_mel_bins", 23)), mj_kaldi_frame_length=float(fb.pop("frame_length", 25.0)),
                     mj_kaldi_frame_shift=float(fb.pop("frame_shift", 10.0)),
                     mj_kaldi_preemphasis=float(fb.pop("preemphasis_coefficient", 0.97)))
        if fb:
            raise NotImplementedError(f"mockingjay audio.kaldi.fbank options {sorted(fb)} are not built")
        delta, cm = audio.get("delta", {}), audio.get("cmvn", {})
        flags.update(mj_delta_order=int(delta.get("order", 2)), mj_delta_win=int(delta.get("win_length", 5)))
        frontend, cmvn, target = "kaldi", bool(cm.get("use_cmvn", False)), -25.0
        input_dim = flags["mj_kaldi_mel_bins"] * (flags["mj_delta_order"] + 1)
    else:
        if "input" not in audio:
            raise ValueError("mockingjay checkpoint: audio has neither a `kaldi` nor an `input` block")
        inp = audio["input"]
        if inp.get("feat_type") != "mel":
            raise NotImplementedError(f"mockingjay audio.input.feat_type={inp.get('feat_type')!r} is not built: only 'mel'")
        if int(inp.get("delta", 0)) > 0:
            raise NotImplementedError("mockingjay audio.input.delta > 0 is not built")
        if not bool(inp.get("log", False)):
            raise NotImplementedError("mockingjay audio.input.log=False is not built")
        for key, want in (("win_ms", 25), ("hop_ms", 10), ("n_freq", 201), ("sample_rate", 16000)):
            if audio.get(key, want) != want:
                raise NotImplementedError(f"mockingjay audio.{key}={audio[key]!r} is not built: only {want}")
        frontend, cmvn, target = "mel", bool(inp.get("cmvn", False)), float(audio["target_level"])
        input_dim = int(audio.get("n_mels", 40))
    return mockingjay_config(t["hidden_size"], t["num_hidden_layers"], t["num_attention_heads"], t["intermediate_size"], input_dim,
                             frontend, config["task"]["sequence_length"], bool(t.get("share_layer", False)),
                             float(t.get("layer_norm_eps", 1e-12)), cmvn, target, **flags)


def config_from_multires(model_cfg: Dict, task_cfg: Dict | None = None) -> EncoderConfig:
    """``MultiresHubertConfig`` (upstream/multires_hubert/hubert_model.py:97-330) + ``task_cfg.normalize``."""
    cfg = EncoderConfig(family="multires_hubert")
    for k in _MODEL_KEYS:
        if k in model_cfg and model_cfg[k] is not None:
            setattr(cfg, k, type(getattr(cfg, k))(model_cfg[k]))
    if "conv_feature_layers" in model_cfg:
        cfg.conv_layers = parse_conv_layers(model_cfg["conv_feature_layers"])
    act = model_cfg.get("activation_fn", "gelu")
    if str(getattr(act, "name", act)) != "gelu":
        raise ValueError(f"only activation_fn='gelu' is on the hot path, got {act!r}")
    if str(model_cfg.get("layer_type", "transformer")).endswith("conformer"):
        raise ValueError("conformer layers are out of scope (SURVEY §2.1)")
    ratios = model_cfg.get("label_rate_ratios", [1, 2])
    if ratios in (None, "None"):
        raise ValueError("without ratios, the model is exactly as the Hubert model")  # hubert_model.py:362-364
    cfg.label_rate_ratios = [int(x) for x in ratios]
    n_blocks = len(cfg.label_rate_ratios) // 2 * 2 + 1
    per_block = int(model_cfg.get("encoder_layers", 2))
    over = model_cfg.get("override_encoder_layers", "") or ""
    if over:  # hubert_model.py:377-403,415-424: encoders[i] = o[i], middle = o[len // 2], decoders[i] = o[len - 1 - i]
        o = [int(x) for x in (ast.literal_eval(over) if isinstance(over, str) else over)]
        if len(o) != n_blocks:
            raise ValueError("number of override encoder layers must match the label rate ratios information")
        R = n_blocks // 2 + 1
        cfg.block_layers = o[:R] + [o[len(o) - 1 - i] for i in range(R - 1)]
    else:
        cfg.block_layers = [per_block] * n_blocks
    cfg.encoder_layers = sum(cfg.block_layers)
    cfg.conv_adapter_kernel = int(model_cfg.get("conv_adapator_kernal", 7))
    cfg.use_plain_updownsample = bool(model_cfg.get("use_plain_updownsample", False))
    if task_cfg is not None and "normalize" in task_cfg:
        cfg.normalize = bool(task_cfg["normalize"])
    cfg.validate()
    return cfg


def config_from_distiller(d: Dict) -> EncoderConfig:
    """``DistillerConfig`` (upstream/distiller/model.py:17-80) from ``ckpt["Config"]["distiller"]``."""
    cfg = EncoderConfig(family="distiller", feature_layer_norm=False)
    cfg.extractor_mode = str(d.get("extractor_mode", "default"))
    cfg.conv_layers = parse_conv_layers(d.get("extractor_conv_feature_layers", DEFAULT_CONV_LAYERS))
    cfg.conv_pos = int(d.get("conv_pos", 128))
    cfg.conv_pos_groups = int(d.get("conv_pos_groups", 16))
    cfg.encoder_layers = int(d.get("encoder_layers", 1))
    cfg.encoder_embed_dim = int(d.get("encoder_embed_dim", 768))
    cfg.encoder_ffn_embed_dim = int(d.get("encoder_ffn_embed_dim", 3072))
    cfg.encoder_attention_heads = int(d.get("encoder_attention_heads", 12))
    cfg.layer_norm_first = bool(d.get("layer_norm_first", False))
    if str(d.get("activation_fn", "gelu")) != "gelu":
        raise ValueError("only activation_fn='gelu' is on the hot path")
    if str(d.get("attention_type", "original")) != "original":
        raise ValueError("distiller attention_type must be 'original'")
    task, out = str(d.get("task_emb_type", "expand-last")), str(d.get("out_layer_type", "expand-last"))
    if task != "expand-last" or out != "expand-last":
        raise ValueError("only the DistilHuBERT head layout (task_emb_type = out_layer_type = 'expand-last') is built")
    cfg.pred_heads = int(d.get("n_tasks", 12))
    if int(d.get("final_dim", 768)) != cfg.encoder_embed_dim or int(d.get("out_layer_inter_dim", -1)) > 0:
        raise ValueError("distiller heads must keep the encoder width (final_dim == encoder_embed_dim, no inter dim)")
    if cfg.conv_dim == cfg.encoder_embed_dim:
        raise ValueError("distiller without post_extract_proj (conv width == encoder width) is not built")
    cfg.validate()
    return cfg
