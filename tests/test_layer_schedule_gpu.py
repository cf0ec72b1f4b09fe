"""The Transformer layer's schedule, counted: one profiled forward per fixture, and the launches of every kind the layer enqueues
(q|k|v GEMM, attention, out_proj, LayerNorm 1, fc1, fc2, LayerNorm 2) and of what surrounds it (encoder.layer_norm, the positional
conv, the ffn_out selection's residual add, Mockingjay's own LayerNorm, the DistilHuBERT heads) against numbers worked out from the
configuration alone.  Every encoder family that runs the layer is here, in both LayerNorm orders and in the 16-bit operand modes."""

import pytest

pytestmark = pytest.mark.gpu

LAYER_KINDS = ["gemm:qkv", "attention", "gemm:out_proj", "layernorm:ln1", "gemm:fc1", "gemm:fc2", "layernorm:ln2"]
AROUND = ["layernorm:enc", "residual_add", "posconv", "layernorm_eps", "gemm:mj_in", "gemm:head1", "gemm:head2"]
FFN_OUT = "fairseq_layers_before_residual"


def _launches(cfg, weights, wavs, dtype="fp32", selection=None):
    """{kind: launches} of one forward"""
    import torch

    from s3prl_amd.encoder import HipEncoder

    enc = HipEncoder(cfg, weights, dtype=dtype)
    try:
        enc.profile_enable(True)
        enc.forward([torch.from_numpy(w).cuda() for w in wavs], selection=selection)
        torch.cuda.synchronize()
        return {p["name"]: p["launches"] for p in enc.profile_read()}
    finally:
        enc.close()


def _check(what, got, layers, **around):
    want = dict({k: layers for k in LAYER_KINDS}, **{k.replace("__", ":"): v for k, v in around.items()})
    found = {k: got.get(k, 0) for k in LAYER_KINDS + AROUND}
    assert found == dict({k: 0 for k in AROUND}, **want), what


@pytest.mark.parametrize("name, dtype, selection", [
    ("tiny_hubert_pad", "fp32", None), ("tiny_hubert_pad", "bf16", None), ("tiny_hubert_pad", "fp32", FFN_OUT), ("tiny_hubert_pad", "bf16", FFN_OUT),
    ("tiny_hubert_large_pad", "fp32", None), ("tiny_hubert_large_pad", "fp32", FFN_OUT), ("tiny_wavlm_large_pad", "fp32", None),
    ("tiny_wavlm_pad", "fp32", None), ("tiny_wav2vec2_fsbefore", "fp32", FFN_OUT), ("tiny_distiller_pad", "fp32", None)])
def test_single_resolution_encoder(name, dtype, selection, golden_loader):
    """post-LN (HuBERT-base, WavLM-base+, wav2vec 2.0, DistilHuBERT) and pre-LN (HuBERT-large, WavLM-large) stacks: NL of every
    layer kind, one encoder.layer_norm, one positional conv; the residual is a separate add only where fc2's product is a state"""
    meta, cfg, weights, wavs, _, _ = golden_loader(name)
    if name == "tiny_wav2vec2_fsbefore":
        assert meta["selection"] == FFN_OUT
    NL = cfg.encoder_layers
    heads = {"gemm__head1": 1, "gemm__head2": cfg.pred_heads} if cfg.pred_heads else {}
    _check((name, dtype, selection), _launches(cfg, weights, wavs, dtype, selection), NL, layernorm__enc=1, posconv=1,
           residual_add=NL if selection == FFN_OUT else 0, **heads)


@pytest.mark.parametrize("fold", [0, 1])
def test_fp16x2_with_and_without_the_layernorm1_fold(fold, golden_loader):
    """tuning key ln1_fold: LayerNorm 1 folded into fc2's epilogue or not, the layer enqueues the same launches"""
    from s3prl_amd import _lib

    _, cfg, weights, wavs, _, _ = golden_loader("tiny_hubert_pad")
    lib = _lib.load()
    try:
        _lib.check(lib.s3enc_set_tuning(b"ln1_fold", fold))
        got = _launches(cfg, weights, wavs, "fp16x2")
    finally:
        _lib.check(lib.s3enc_set_tuning(b"ln1_fold", 1))
    _check(("tiny_hubert_pad", "fp16x2", fold), got, cfg.encoder_layers, layernorm__enc=1, posconv=1)


@pytest.mark.parametrize("name", ["tiny_multires_pad", "tiny_multires_large_pad", "tiny_multires3_pad"])
def test_multires_blocks(name, golden_loader):
    """every block of the U-net runs its own number of layers and its own encoder.layer_norm; only the first has a positional conv"""
    _, cfg, weights, wavs, _, _ = golden_loader(name)
    assert len(cfg.block_layers) >= 3 and sum(cfg.block_layers) == cfg.encoder_layers
    _check(name, _launches(cfg, weights, wavs), sum(cfg.block_layers), layernorm__enc=len(cfg.block_layers), posconv=1)


@pytest.mark.parametrize("name", ["mae_ast/tiny_patch_pad", "mae_ast/tiny_preln_pad"])
def test_mae_ast(name, golden_loader):
    """no positional conv; encoder.layer_norm runs in front of a post-LN stack and not at all in a pre-LN one"""
    _, cfg, weights, wavs, _, _ = golden_loader(name)
    assert cfg.layer_norm_first == (name == "mae_ast/tiny_preln_pad")
    _check(name, _launches(cfg, weights, wavs), cfg.encoder_layers, layernorm__enc=0 if cfg.layer_norm_first else 1)


@pytest.mark.parametrize("name", ["mockingjay/tiny_pad", "mockingjay/tiny_albert", "mockingjay/tiny_chunk"])
def test_mockingjay(name, golden_loader):
    """BERT layers around the family's own LayerNorm (the input representation's, then two per layer); a shared layer runs NL times"""
    _, cfg, weights, wavs, _, _ = golden_loader(name)
    assert cfg.mj_share_layer == (name == "mockingjay/tiny_albert")
    NL = cfg.encoder_layers
    _check(name, _launches(cfg, weights, wavs), NL, layernorm__ln1=0, layernorm__ln2=0, layernorm_eps=1 + 2 * NL, gemm__mj_in=1)
