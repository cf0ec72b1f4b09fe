"""DeCoAR 2.0 end to end on the GPU: every fixture of tests/golden/decoar2/ (the reference's own expert, hooks and postprocess
included, on seeded checkpoints) through the C ABI (HipEncoder) and through the Python expert (``decoar2_local`` on a written
checkpoint).

Bands: per state rel_err < FP32_TOL = 1e-4 against the golden subsample and against the stored full-tensor norms
(tests/test_encoder_gpu.py's), < ORACLE_TOL per utterance and state against the float64 restatement tests/decoar2_ref.py
(tests/test_lighthubert_gpu.py's band), which tests/test_decoar2_cpu.py holds to the same fixtures on all rows — padded rows
included: they follow HuBERT's rule, the reference's values.  Exact, in fp32: a forward repeats bit for bit, an utterance alone equals
its rows inside a batch and inside a permuted batch padded to the same n_max, shards equal the full batch, one handle forwarded at
several lengths equals fresh handles.

Operand modes, on the full-size fixture ``pseudo`` (released shape, pretrained-like statistics): every mode meets the bound
tests/test_encoder_gpu.py holds HuBERT-base's pretrained-like fixtures to in that mode (``PL_16BIT_TOL``; fp32x3: that file's 1e-4,
its ``FP32_TOL``), with finite outputs."""

import numpy as np
import pytest

import decoar2_ref as R
from oracle import encoder_oracle as O
from test_encoder_gpu import FP32_TOL, PL_16BIT_TOL, _encoder, _run
from test_lighthubert_gpu import ORACLE_TOL

pytestmark = pytest.mark.gpu

FIXTURES = ("tiny_ragged_odd", "tiny_ragged_even", "tiny_equal", "tiny_t1", "tiny_two_tiles", "tiny_d192", "pseudo")
MODE_TOL = dict(PL_16BIT_TOL, fp32x3=FP32_TOL)  # tests/test_encoder_gpu.py::test_fp32x3_on_pretrained_like_statistics: < 1e-4


@pytest.fixture(scope="module")
def cases(golden_loader):
    """name -> (meta, cfg, weights, wavs, golden, norms, float64 restatement, states of one C-ABI forward, its handle kept for the
    tests that forward again); every value computed once."""
    cache = {}

    def get(name):
        if name not in cache:
            meta, cfg, weights, wavs, golden, norms = golden_loader(f"decoar2/{name}")
            enc = _encoder(cfg, weights)
            cache[name] = (meta, cfg, weights, wavs, golden, norms, R.forward(cfg, weights, wavs), _run(enc, wavs), enc)
        return cache[name]

    yield get
    for c in cache.values():
        c[-1].close()


def _check_states(name, meta, cfg, wavs, golden, norms, ref, hs):
    NS = cfg.encoder_layers + 1
    assert hs.shape[0] == NS == meta["n_states"] and list(hs.shape[1:]) == meta["shape"] and np.isfinite(hs).all()
    ts, cs = meta["t_stride"], meta["c_stride"]
    errs = [O.rel_err(hs[l][:, ::ts, ::cs], golden[l]) for l in range(NS)]
    nerr = [abs(np.linalg.norm(hs[l].astype(np.float64)) - norms[l]) / norms[l] for l in range(NS)]
    oerr = [O.rel_err(hs[l][b], ref[l][b]) for l in range(NS) for b in range(len(wavs))]
    # the padded rows alone: state 0's and the later states' (golden: the stored subsample of them; float64: all of them)
    pad_g = [O.rel_err(hs[l][b][::ts, ::cs][-(-v // ts):], golden[l][b, -(-v // ts):])  # stored row j is frame j * ts
             for l in range(NS) for b, v in enumerate(meta["valid"]) if -(-v // ts) < golden[l].shape[1]]
    pad_o = [O.rel_err(hs[l][b, v:], ref[l][b, v:]) for l in range(NS) for b, v in enumerate(meta["valid"]) if v < meta["shape"][1]]
    print(f"DECOAR2 {name}: golden {max(errs):.2e} norms {max(nerr):.2e} (< {FP32_TOL:.0e}), restatement per utterance {max(oerr):.2e}"
          f" (< {ORACLE_TOL:.0e}), padded rows: golden {max(pad_g, default=0):.2e} float64 {max(pad_o, default=0):.2e}")
    assert max(errs) < FP32_TOL, f"{name}: per-state rel-err against the golden {['%.2e' % e for e in errs]}"
    assert max(nerr) < FP32_TOL, f"{name}: per-state norm error {['%.2e' % e for e in nerr]}"
    assert max(oerr) < ORACLE_TOL, f"{name}: per (state, utterance) rel-err against float64 {['%.2e' % e for e in oerr]}"
    assert max(pad_g, default=0) < FP32_TOL, f"{name}: padded rows against the golden {['%.2e' % e for e in pad_g]}"
    assert max(pad_o, default=0) < ORACLE_TOL, f"{name}: padded rows against float64 {['%.2e' % e for e in pad_o]}"


@pytest.mark.parametrize("name", FIXTURES)
def test_c_abi_matches_the_reference_fixture(name, cases):
    meta, cfg, weights, wavs, golden, norms, ref, hs, enc = cases(name)
    NS = cfg.encoder_layers + 1
    assert enc.num_states() == NS and enc.status() == 0 and enc.downsample_rate() == 320
    n_max = max(meta["lengths"])
    assert [enc.num_frames(n) for n in meta["lengths"]] == meta["valid"] == [enc.valid_frames(n, n_max) for n in meta["lengths"]]
    assert enc.num_output_frames(n_max) == meta["shape"][1] == -(-max(meta["fbank_frames"]) // 2)
    _check_states(name, meta, cfg, wavs, golden, norms, ref, hs)
    again = _run(enc, wavs)
    assert np.array_equal(again.view(np.int32), hs.view(np.int32)), "a second forward of the same handle differs"


@pytest.mark.parametrize("name", FIXTURES)
def test_python_expert_matches_the_reference_fixture(name, cases, tmp_path):
    """``decoar2_local(ckpt)``: the checkpoint is written in the released layout with a tensor the encoder does not own, and read by
    the product reader, which takes every width from the tensors' shapes."""
    import torch

    import s3prl_amd.hub as hub
    from s3prl_amd.ckpt import save_checkpoint

    meta, cfg, weights, wavs, golden, norms, ref, hs_abi, _ = cases(name)
    NS = cfg.encoder_layers + 1
    path = str(tmp_path / f"{name}.pt")
    save_checkpoint(path, cfg, dict(weights, mask_emb=np.zeros(cfg.encoder_embed_dim, np.float32)))
    expert = hub.decoar2_local(path)
    assert expert.get_downsample_rates("hidden_states") == 320 and expert.cfg.to_dict() == cfg.to_dict()
    assert "mask_emb" not in expert._weights
    with torch.no_grad():
        out = expert([torch.from_numpy(w).cuda() for w in wavs])
    assert len(out["hidden_states"]) == NS and out["last_hidden_state"] is out["hidden_states"][-1]
    assert list(out["_hidden_states_info"]) == [f"self.model.encoder.layers[{i}]" for i in range(NS - 1)] + ["self.model.encoder"]
    hs = torch.stack(list(out["hidden_states"])).cpu().numpy()
    _check_states(name, meta, cfg, wavs, golden, norms, ref, hs)
    assert np.array_equal(hs.view(np.int32), hs_abi.view(np.int32)), "the expert and the C ABI run the same handle code"


@pytest.mark.parametrize("name", ("tiny_ragged_odd", "tiny_t1", "tiny_d192"))
def test_an_utterance_alone_equals_its_rows_in_the_batch_and_in_a_permuted_batch(name, cases):
    """Padded to the batch's n_max, every utterance on its own gives the rows it has inside the batch, bit for bit, padded rows
    included; and the batch in another order gives every utterance the same rows."""
    meta, cfg, weights, wavs, golden, norms, ref, hs, enc = cases(name)
    n_max = max(meta["lengths"])
    for b, w in enumerate(wavs):
        alone = _run(enc, [w], n_max=n_max)
        assert np.array_equal(alone[:, 0].view(np.int32), hs[:, b].view(np.int32)), f"{name}: utterance {b} alone differs from its batch rows"
    perm = list(range(len(wavs)))[::-1]
    got = _run(enc, [wavs[i] for i in perm])
    for j, i in enumerate(perm):
        assert np.array_equal(got[:, j].view(np.int32), hs[:, i].view(np.int32)), f"{name}: utterance {i} in slot {j} of the permuted batch"


def test_shards_equal_the_full_batch(cases):
    meta, cfg, weights, wavs, golden, norms, ref, hs, enc = cases("tiny_ragged_even")
    n_max = max(meta["lengths"])
    parts = [_run(enc, wavs[:1], n_max=n_max), _run(enc, wavs[1:], n_max=n_max)]
    assert np.array_equal(np.concatenate(parts, axis=1).view(np.int32), hs.view(np.int32))


def test_one_handle_at_several_lengths_equals_fresh_handles(cases):
    """The workspace and the staging ring are reused across shapes: growing, shrinking and one-model-frame batches on one handle."""
    from s3prl_amd.synth import synth_wavs

    meta, cfg, weights, wavs, golden, norms, ref, hs, enc = cases("tiny_ragged_odd")
    batches = [synth_wavs(lens, 190 + i) for i, lens in enumerate(([3000, 2000], [41999], [560], [6319, 3500, 4777, 801]))]
    reused = [_run(enc, b) for b in batches]
    for b, got in zip(batches, reused):
        fresh = _encoder(cfg, weights)
        want = _run(fresh, b)
        fresh.close()
        assert got.shape == want.shape and np.array_equal(got.view(np.int32), want.view(np.int32)), [len(x) for x in b]
    assert enc.status() == 0


def test_an_utterance_with_fewer_than_two_frames_is_refused_by_name(cases):
    import ctypes as C

    import torch

    from s3prl_amd import _lib
    from s3prl_amd.synth import synth_wavs

    meta, cfg, weights, wavs, golden, norms, ref, hs, enc = cases("tiny_ragged_odd")
    for short in (559, 400, 399):  # one frame, one frame, none
        with pytest.raises(ValueError, match="fewer than 2 analysis windows"):
            _run(enc, synth_wavs([4000, short], 3))
    # the C ABI says the same to a caller that did not come through HipEncoder
    held = [torch.from_numpy(w).cuda() for w in synth_wavs([4000, 559], 3)]
    out = torch.empty((cfg.encoder_layers + 1, 2, 12, cfg.encoder_embed_dim), device="cuda")
    rc = enc._lib.s3enc_forward(enc._h, (C.c_void_p * 2)(*[w.data_ptr() for w in held]), (C.c_int64 * 2)(4000, 559), 2, 0,
                                C.c_void_p(out.data_ptr()), out[0].numel(), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc != 0 and "fewer than 2 analysis windows (DeCoAR 2.0" in enc._lib.s3enc_last_error().decode()
    torch.cuda.synchronize()
    assert enc.status() == 0
    assert np.array_equal(_run(enc, wavs).view(np.int32), hs.view(np.int32)), "the handle still forwards after a refusal"


def test_feature_selection_is_refused_by_name(cases):
    from s3prl_amd import _lib

    enc = cases("tiny_equal")[-1]
    for sel in ("fairseq_layers", "fairseq_layers_before_residual"):
        with pytest.raises(_lib.S3EncError, match="feature_selection is not defined for DeCoAR 2.0"):
            enc.num_states(sel)
        with pytest.raises(_lib.S3EncError, match="feature_selection is not defined for DeCoAR 2.0"):
            _run(enc, cases("tiny_equal")[3], selection=sel)


@pytest.mark.parametrize("dtype", sorted(MODE_TOL))
def test_operand_modes_on_the_full_size_fixture(dtype, cases):
    """Every operand mode meets HuBERT-base's pretrained-like bound of that mode on the released shape (measured: fp32x3 5.0e-6, fp16x2
    3.6e-4, fp16 3.7e-4, bf16 3.2e-3), so all five are served; the front end and post_extract_proj are fp32 in each."""
    meta, cfg, weights, wavs, golden, norms, ref, hs32, _ = cases("pseudo")
    enc = _encoder(cfg, weights, dtype=dtype)
    try:
        hs = _run(enc, wavs)
        assert enc.status() == 0
    finally:
        enc.close()
    ts, cs = meta["t_stride"], meta["c_stride"]
    errs = [O.rel_err(hs[l][:, ::ts, ::cs], golden[l]) for l in range(hs.shape[0])]
    print(f"DECOAR2 pseudo / {dtype}: worst state {max(errs):.2e} (< {MODE_TOL[dtype]:.1e})")
    assert np.isfinite(hs).all()
    assert max(errs) < MODE_TOL[dtype], f"{dtype}: per-state rel-err {['%.2e' % e for e in errs]}"
