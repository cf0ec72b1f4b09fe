"""LightHuBERT end to end on the GPU: every fixture of tests/golden/lighthubert/ (the reference's own expert on seeded supernet
checkpoints) through the C ABI (HipEncoder) and through the Python expert (``lighthubert_local`` on a written checkpoint).

Bands: per state rel_err < FP32_TOL = 1e-4 against the golden subsample and against the stored full-tensor norms
(tests/test_encoder_gpu.py's), < 5e-5 per utterance and state against the float64 restatement tests/lighthubert_ref.py (that file's
oracle band), which tests/test_lighthubert_cpu.py holds to the same fixtures on all rows.  Exact: state 0's padded rows are zero, a
forward repeats bit for bit, an utterance alone equals its rows inside a batch padded to the same n_max, one handle forwarded at
several lengths equals fresh handles."""

import numpy as np
import pytest

import lighthubert_ref as R
from oracle import encoder_oracle as O
from test_encoder_gpu import FP32_TOL, _encoder, _run

pytestmark = pytest.mark.gpu

FIXTURES = ("base_ragged", "base_equal", "base_two_tiles", "small_ragged", "small_one_frame", "stage1", "base_pl")
ORACLE_TOL = 5e-5


@pytest.fixture(scope="module")
def cases(golden_loader):
    """name -> (meta, cfg, supernet weights, wavs, golden, norms, float64 restatement, states of one C-ABI forward, its handle kept
    for the tests that forward again); every value computed once."""
    cache = {}

    def get(name):
        if name not in cache:
            meta, cfg, weights, wavs, golden, norms = golden_loader(f"lighthubert/{name}")
            enc = _encoder(cfg, weights)
            cache[name] = (meta, cfg, weights, wavs, golden, norms, R.forward(cfg, weights, wavs), _run(enc, wavs), enc)
        return cache[name]

    yield get
    for c in cache.values():
        c[-1].close()


def _check_states(name, meta, cfg, wavs, golden, norms, ref, hs):
    assert hs.shape[0] == 13 == meta["n_states"] and list(hs.shape[1:]) == meta["shape"] and np.isfinite(hs).all()
    ts, cs = meta["t_stride"], meta["c_stride"]
    errs = [O.rel_err(hs[l][:, ::ts, ::cs], golden[l]) for l in range(13)]
    nerr = [abs(np.linalg.norm(hs[l].astype(np.float64)) - norms[l]) / norms[l] for l in range(13)]
    oerr = [O.rel_err(hs[l][b], ref[l][b]) for l in range(13) for b in range(len(wavs))]
    print(f"LIGHTHUBERT {name}: golden {max(errs):.2e} norms {max(nerr):.2e} (< {FP32_TOL:.0e}), restatement per utterance {max(oerr):.2e} (< {ORACLE_TOL:.0e})")
    assert max(errs) < FP32_TOL, f"{name}: per-state rel-err against the golden {['%.2e' % e for e in errs]}"
    assert max(nerr) < FP32_TOL, f"{name}: per-state norm error {['%.2e' % e for e in nerr]}"
    assert max(oerr) < ORACLE_TOL, f"{name}: per (state, utterance) rel-err against float64 {['%.2e' % e for e in oerr]}"
    for b, v in enumerate(meta["valid"]):
        assert not hs[0][b, v:].any(), f"{name}: state 0, utterance {b}: padded rows must be exactly zero"
        assert hs[0][b, :v].any(axis=1).all()


@pytest.mark.parametrize("name", FIXTURES)
def test_c_abi_matches_the_reference_fixture(name, cases):
    meta, cfg, weights, wavs, golden, norms, ref, hs, enc = cases(name)
    assert enc.num_states() == 13 and enc.status() == 0
    _check_states(name, meta, cfg, wavs, golden, norms, ref, hs)
    again = _run(enc, wavs)
    assert np.array_equal(again.view(np.int32), hs.view(np.int32)), "a second forward of the same handle differs"


@pytest.mark.parametrize("name", FIXTURES)
def test_python_expert_matches_the_reference_fixture(name, cases, tmp_path):
    """``lighthubert_local(ckpt)``: the checkpoint is written in the released layout, read and cut by the product reader."""
    import torch

    import s3prl_amd.hub as hub
    from s3prl_amd.ckpt import save_checkpoint

    meta, cfg, weights, wavs, golden, norms, ref, hs_abi, _ = cases(name)
    path = str(tmp_path / f"{name}.pt")
    save_checkpoint(path, cfg, weights)
    expert = hub.lighthubert_local(path)
    assert expert.get_downsample_rates("hidden_states") == 320 and expert.cfg.to_dict() == cfg.to_dict()
    assert "encoder.pos_conv.0.weight_v" not in expert._weights and "mask_emb" not in expert._weights, "only the subnet is kept"
    with torch.no_grad():
        out = expert([torch.from_numpy(w).cuda() for w in wavs])
    assert list(out) == ["hidden_states"] and len(out["hidden_states"]) == 13
    hs = torch.stack(list(out["hidden_states"])).cpu().numpy()
    _check_states(name, meta, cfg, wavs, golden, norms, ref, hs)
    assert np.array_equal(hs.view(np.int32), hs_abi.view(np.int32)), "the expert and the C ABI run the same handle code"


@pytest.mark.parametrize("name", ("base_ragged", "small_one_frame"))
def test_an_utterance_alone_equals_its_rows_in_the_batch(name, cases):
    """Padded to the batch's n_max, every utterance on its own gives the rows it has inside the batch, bit for bit, padded rows included."""
    meta, cfg, weights, wavs, golden, norms, ref, hs, enc = cases(name)
    n_max = max(meta["lengths"])
    for b, w in enumerate(wavs):
        alone = _run(enc, [w], n_max=n_max)
        assert np.array_equal(alone[:, 0].view(np.int32), hs[:, b].view(np.int32)), f"{name}: utterance {b} alone differs from its batch rows"


def test_one_handle_at_several_lengths_equals_fresh_handles(cases):
    """The workspace and the staging ring are reused across shapes: growing, shrinking and single-frame batches on one handle."""
    from s3prl_amd.synth import synth_wavs

    meta, cfg, weights, wavs, golden, norms, ref, hs, enc = cases("small_ragged")
    batches = [synth_wavs(lens, 90 + i) for i, lens in enumerate(([3000, 2000], [41999], [400], [6319, 3500, 4777, 801]))]
    reused = [_run(enc, b) for b in batches]
    for b, got in zip(batches, reused):
        fresh = _encoder(cfg, weights)
        want = _run(fresh, b)
        fresh.close()
        assert got.shape == want.shape and np.array_equal(got.view(np.int32), want.view(np.int32)), [len(x) for x in b]


@pytest.mark.parametrize("dtype", ("bf16", "fp16", "fp32x3", "fp16x2"))
def test_a_non_fp32_dtype_is_refused_by_name(dtype, cases):
    from s3prl_amd.upstream.lighthubert.expert import UpstreamExpert

    meta, cfg, weights = cases("small_ragged")[:3]
    with pytest.raises(Exception, match=f"fp32 only; {dtype} is not built"):
        _encoder(cfg, weights, dtype=dtype)
    with pytest.raises(ValueError, match=f"fp32 only; {dtype} is not built"):
        UpstreamExpert("unused.pt", dtype=dtype)


def test_feature_selection_is_refused_by_name(cases):
    from s3prl_amd import _lib

    enc = cases("small_ragged")[-1]
    for sel in ("fairseq_layers", "fairseq_layers_before_residual"):
        with pytest.raises(_lib.S3EncError, match="feature_selection is not defined for LightHuBERT"):
            enc.num_states(sel)
        with pytest.raises(_lib.S3EncError, match="feature_selection is not defined for LightHuBERT"):
            _run(enc, cases("small_ragged")[3], selection=sel)


def test_the_featurizer_epilogue_sums_this_state_list(cases):
    """``s3enc_forward_opts.featurize``: the weighted sum over the 13 states — state 0 being the projection output, not HuBERT's
    layer-0 input — with and without the per-state LayerNorm, against the same sum of the states a plain forward returns
    (tests/test_fuzz_gpu.py's band for that comparison)."""
    import torch

    meta, cfg, weights, wavs, golden, norms, ref, hs, enc = cases("small_ragged")
    dev = [torch.from_numpy(w).cuda() for w in wavs]
    w = np.random.default_rng(5).random(13) + 0.05  # positive, summing to one: a softmax's output, as in tests/test_fuzz_gpu.py
    w = (w / w.sum()).astype(np.float32)
    for normalize in (False, True):
        got = enc.forward_featurized(dev, w, normalize=normalize).cpu().numpy()
        want = np.zeros(hs[0].shape, dtype=np.float64)
        for wi, h in zip(w, hs.astype(np.float64)):
            want += wi * (O.layer_norm(h, None, None) if normalize else h)
        assert O.rel_err(got, want) < 3e-6, normalize
