"""The plain signal features on the MI355X (`spectrogram`, `mfcc`, `mel`, `linear`, `stft_mag`: s3prl_amd/csrc/spectral_ops.hip) through
the C ABI and through the hub entries, against the float64 restatement tests/spectral_ref.py and the reference's own outputs
(tests/golden/spectral).

Bands (tests/spectral_ref.py holds the constants): OP_TOL = 2e-5 is the project's op bound.
  linear domain, every bin      |P - P_ref| <= 2 OP_TOL max_k P_ref per frame (OP_TOL alone for a magnitude); log outputs go through
                                exp, floored or clamped bins are compared as floored; the spectrogram's bin 0 as the energy, relative
                                to its own value; a mel band by the same bound times the sum of its weights
  log domain, well-conditioned  a bin holding at least 1e-4 of its frame's largest power: |d log P| <= 2 OP_TOL / sqrt(1e-4) = 4e-3,
                                half of it for a log magnitude; at most 5 % of an utterance's bins may be left out
  mfcc without CMVN             |dc_i| <= lifter_i sqrt(23) 2e-4: tests/test_fbank_gpu.py's 2e-4 for a log-mel through unit-norm DCT
                                columns; the deltas at their source's band
  CMVN                          the normalised output against the float64 CMVN of the device's OWN un-normalised output, 1e-5
  mfcc whole path               5e-3, fbank's band
  fixtures                      FP32_TOL = 1e-4 as a relative norm per utterance
Every test prints its worst figures (`SPECTRAL_BAND ...`)."""

import ctypes as C
import functools
import json
import os

import numpy as np
import pytest

import spectral_ref as R

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SPECTRAL_DIR = os.path.join(HERE, "golden", "spectral")
FP32_TOL = 1e-4
LOGMEL_BAND = 2e-4  # tests/test_fbank_gpu.py: a log-mel against float64
CMVN_TOL = 1e-5
WHOLE_TOL = 5e-3    # tests/test_fbank_gpu.py: the whole normalised path
PREPROC_CASES = ("plain", "short_first", "zero_tail", "all_zero")


def _config(kind, **kw):
    from s3prl_amd import _lib

    c = _lib.S3SpectralConfig()
    c.kind, c.sample_rate = _lib.SPECTRAL_KINDS[kind], 16000
    c.frame_length_ms, c.frame_shift_ms, c.preemphasis = 25.0, 10.0, 0.97
    c.num_mel_bins, c.num_ceps, c.cepstral_lifter = (80 if kind == "mel" else 23), 13, 22.0
    c.delta_order, c.delta_win_length, c.use_cmvn, c.cmvn_eps = (2 if kind == "mfcc" else 0), 5, 1, 1e-10
    c.log = 1
    c.n_fft, c.hop, c.win = (512, 320, 512) if kind == "stft_mag" else (400, 160, 400)
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def _device(wav, misaligned=False):
    """the waveform on the device; misaligned: 4 bytes behind a 16-byte line."""
    import torch

    buf = torch.zeros(len(wav) + 8, device="cuda")
    off = (-(buf.data_ptr() // 4) % 4) + (1 if misaligned else 0)
    view = buf[off:off + len(wav)]
    view.copy_(torch.from_numpy(np.ascontiguousarray(wav)))
    assert view.data_ptr() % 16 == (4 if misaligned else 0)
    return view


def run(c, wavs, misaligned=()):
    """s3enc_spectral_num_frames + s3enc_spectral_forward: (the (B, T, F) output on the host, the frame counts)."""
    import torch

    from s3prl_amd import _lib
    from s3prl_amd.upstream.baseline.expert import spectral_output_dim

    lib = _lib.load()
    dev = [_device(w, b in misaligned) for b, w in enumerate(wavs)]
    B = len(wavs)
    ptrs = (C.c_void_p * B)(*[w.data_ptr() for w in dev])
    lens = (C.c_int64 * B)(*[len(w) for w in wavs])
    frames = (C.c_int32 * B)()
    _lib.check(lib.s3enc_spectral_num_frames(C.byref(c), ptrs, lens, B, frames, 0, None), "s3enc_spectral_num_frames")
    out = torch.full((B, max(frames), spectral_output_dim(c)), float("nan"), device="cuda")
    _lib.check(lib.s3enc_spectral_forward(C.byref(c), ptrs, lens, B, C.c_void_p(out.data_ptr()), max(frames), 0, None),
               "s3enc_spectral_forward")
    torch.cuda.synchronize()
    return out.cpu().numpy(), list(frames)


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@functools.lru_cache(maxsize=None)
def kaldi_wavs(scale):
    from s3prl_amd.synth import synth_wavs

    return tuple(synth_wavs(R.KALDI_LENGTHS, R.KALDI_SEED, scale=scale))


@functools.lru_cache(maxsize=None)
def kaldi_run(kind, scale, cmvn):
    return run(_config(kind, use_cmvn=int(cmvn)), list(kaldi_wavs(scale)))


def _check_bins(tag, got_log, ref, floor, magnitude=False):
    """one utterance's (T, nbin) log output against the float64 power (magnitude: |X|): the linear-domain band over every bin, the
    log-domain one over the well-conditioned bins, and the fraction those leave out."""
    lin_tol, log_tol = (R.OP_TOL, R.LOG_TOL / 2) if magnitude else (2 * R.OP_TOL, R.LOG_TOL)
    floored = np.maximum(ref, floor)
    lin = np.abs(np.exp(got_log.astype(np.float64)) - floored) / (lin_tol * floored.max(axis=1, keepdims=True))
    out = R.left_out(ref ** 2 if magnitude else ref)
    dlog = np.abs(got_log - np.log(floored))[~out] / log_tol
    print(f"SPECTRAL_BAND {tag}: linear {lin.max():.3f} of its band, log {dlog.max():.3f} of its band, left out {out.mean():.4f}")
    assert lin.max() <= 1.0 and dlog.max() <= 1.0 and out.mean() <= R.MAX_LEFT_OUT


# ---- the kaldi paths ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [1.0, 1e-2])
def test_spectrogram_bins_and_energy(scale):
    got, frames = kaldi_run("spectrogram", scale, False)
    assert got.shape == (3, 11, 257) and frames == [2, 3, 11]
    for b, wav in enumerate(kaldi_wavs(scale)):
        T = frames[b]
        assert not got[b, T:].view(np.uint32).any(), "rows behind an utterance's frames must be exact zeros"
        power, energy = R.kaldi_power(wav)
        _check_bins(f"spectrogram x{scale} utt {b}", got[b, :T, 1:], power[:, 1:], R.EPS32)
        # bin 0 is the frame's energy, floored at 1: compared as the energy, relative to its own value
        e_ref = np.exp(energy)
        e_err = np.abs(np.exp(got[b, :T, 0].astype(np.float64)) - e_ref) / (2 * R.OP_TOL * e_ref)
        print(f"SPECTRAL_BAND spectrogram x{scale} utt {b}: energy {e_err.max():.3f} of its band")
        assert e_err.max() <= 1.0
        if scale == 1e-2:
            assert (energy == 0.0).all() and not got[b, :T, 0].view(np.uint32).any(), "the energy floor binds: exactly log(1)"
        else:
            assert (energy > 5.0).all()  # ~ log 400: it never does


@pytest.mark.parametrize("scale", [1.0, 1e-2])
def test_mfcc_stages_without_cmvn(scale):
    got, frames = kaldi_run("mfcc", scale, False)
    assert got.shape == (3, 11, 39) and frames == [2, 3, 11]
    band = R.lifter(13) * np.sqrt(23.0) * LOGMEL_BAND
    for b, wav in enumerate(kaldi_wavs(scale)):
        T = frames[b]
        assert not got[b, T:].view(np.uint32).any()
        ref = R.deltas(R.kaldi_mfcc(wav), 2)
        worst = [(np.abs(got[b, :T, lo:lo + 13] - ref[:, lo:lo + 13]) / band).max() for lo in (0, 13, 26)]
        print(f"SPECTRAL_BAND mfcc x{scale} utt {b}: c, delta, delta-delta {worst[0]:.3f} {worst[1]:.3f} {worst[2]:.3f} of their band")
        assert max(worst) <= 1.0


@pytest.mark.parametrize("kind", ["spectrogram", "mfcc"])
@pytest.mark.parametrize("scale", [1.0, 1e-2])
def test_kaldi_cmvn_is_the_float64_cmvn_of_the_devices_own_features(kind, scale):
    raw, frames = kaldi_run(kind, scale, False)
    got, frames2 = kaldi_run(kind, scale, True)
    assert frames == frames2 and got.shape == raw.shape
    for b, T in enumerate(frames):
        assert not got[b, T:].view(np.uint32).any()
        err = np.abs(got[b, :T] - R.cmvn(raw[b, :T])).max()
        print(f"SPECTRAL_BAND {kind} x{scale} utt {b}: cmvn {err:.2e}")
        assert err <= CMVN_TOL


def test_mfcc_whole_path_and_the_single_frame_nan():
    got, frames = kaldi_run("mfcc", 1.0, True)
    ref = R.kaldi_forward("mfcc", list(kaldi_wavs(1.0)), 2)
    assert got.shape == ref.shape
    for b, T in enumerate(frames):
        err = np.abs(got[b, :T] - ref[b, :T]).max()
        print(f"SPECTRAL_BAND mfcc utt {b}: whole path {err:.2e}")
        assert err <= WHOLE_TOL
    for kind in ("mfcc", "spectrogram"):
        one, frames = run(_config(kind), [kaldi_wavs(1.0)[2][:559]])
        assert frames == [1] and np.isnan(one).all(), "one frame under the CMVN is NaN, as in the reference and in fbank"


@pytest.mark.parametrize("kind", ["spectrogram", "mfcc", "stft_mag"])
def test_batch_independence_misaligned_pointer_and_b1(kind):
    if kind == "stft_mag":
        wavs, c = list(stft_wavs()), _config(kind)
        batch = stft_run(True)[0]
    else:
        wavs, c = list(kaldi_wavs(1.0)), _config(kind)
        batch = kaldi_run(kind, 1.0, True)[0]
    for b, w in enumerate(wavs):
        alone, frames = run(c, [w])
        assert _same_bits(alone[0], batch[b, :frames[0]]), f"utterance {b} alone and inside its batch must give the same bits"
        off, _ = run(c, [w], misaligned=(0,))
        assert _same_bits(off, alone), f"utterance {b} at a pointer 4 bytes off a 16-byte line"


# ---- stft_mag ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def stft_wavs():
    from s3prl_amd.synth import synth_wavs

    return tuple(synth_wavs(R.STFT_LENGTHS, R.STFT_SEED))


@functools.lru_cache(maxsize=None)
def stft_run(log):
    return run(_config("stft_mag", log=int(log)), list(stft_wavs()))


@pytest.mark.parametrize("log", [False, True])
def test_stft_mag_bins(log):
    got, frames = stft_run(log)
    assert got.shape == (5, 11, 257) and frames == [1, 1, 2, 4, 11]
    for b, wav in enumerate(stft_wavs()):
        T = frames[b]
        assert not got[b, T:].view(np.uint32).any()
        mag = np.abs(R.centred_stft(wav, 512, 320, 512))
        if log:
            _check_bins(f"stft_mag log utt {b}", got[b, :T], mag, 1e-8, magnitude=True)
        else:
            lin = np.abs(got[b, :T] - mag) / (R.OP_TOL * mag.max(axis=1, keepdims=True))
            print(f"SPECTRAL_BAND stft_mag utt {b}: linear {lin.max():.3f} of its band")
            assert lin.max() <= 1.0


@pytest.mark.parametrize("name", ["stft_mag_lin", "stft_mag_log"])
def test_stft_mag_against_the_reference(name):
    meta, ref = _fixture(name)
    got, frames = run(_config("stft_mag", log=int(meta["log"])), R.fixture_wavs(meta))
    assert frames == [11, 4, 1, 1] and got.shape == ref.shape
    _fixture_check(name, got, ref)
    for b, wav in enumerate(R.fixture_wavs(meta)):
        mag = np.abs(R.centred_stft(wav, 512, 320, 512))
        if meta["log"]:
            _check_bins(f"{name} utt {b}", got[b, :frames[b]], mag, 1e-8, magnitude=True)
        else:
            assert (np.abs(got[b, :frames[b]] - mag) / (R.OP_TOL * mag.max(axis=1, keepdims=True))).max() <= 1.0


# ---- the preprocessor paths ------------------------------------------------------------------------------------------------------
def _fixture(name):
    z = np.load(os.path.join(SPECTRAL_DIR, name + ".npz"))
    return json.loads(bytes(z["meta"]).decode()), z["out"]


def _fixture_check(name, got, ref):
    assert not (np.isnan(got) ^ np.isnan(ref)).any()
    for b in range(ref.shape[0]):
        norm = np.linalg.norm(ref[b].astype(np.float64))
        if norm == 0.0:  # the all-zero utterance: a constant log, an exact mean, exact zeros
            assert not got[b].view(np.uint32).any()
            continue
        err = np.linalg.norm(got[b].astype(np.float64) - ref[b]) / norm
        print(f"SPECTRAL_BAND {name} utt {b}: against the reference {err:.2e}")
        assert err <= FP32_TOL


@pytest.mark.parametrize("case", PREPROC_CASES)
@pytest.mark.parametrize("kind", ["linear", "mel"])
def test_preprocessor_paths_against_the_reference(kind, case):
    meta, ref = _fixture(f"{kind}_{case}")
    wavs = R.fixture_wavs(meta)
    got, frames = run(_config(kind), wavs)
    assert frames == meta["kept"] and got.shape == ref.shape
    _fixture_check(f"{kind}_{case}", got, ref)
    for b, (cnt, keep) in enumerate(zip(meta["counts"], meta["kept"])):
        assert not got[b, min(cnt, keep):].view(np.uint32).any(), "rows behind the CMVN's count and behind the rows kept are zeros"
    # the bins themselves, un-normalised: the same batch without the CMVN (no row is cut by a count then)
    raw, frames = run(_config(kind, use_cmvn=0), wavs)
    lengths = [len(w) for w in wavs]
    T, _, rows, kept = R.preproc_rules(lengths, R.trimmed_lengths(wavs), use_cmvn=False)
    assert frames == kept and raw.shape[1] == rows == T
    bank = R.htk_bank(80)
    for b, w in enumerate(wavs):
        row = np.zeros(max(lengths))
        row[:len(w)] = w
        power = (np.abs(R.centred_stft(row, 400, 160, 400)) ** 2)[:kept[b]]
        ref_lin = (power @ bank if kind == "mel" else power) + 1e-10
        width = bank.sum(axis=0)[None, :] if kind == "mel" else 1.0
        bound = 2 * R.OP_TOL * power.max(axis=1, keepdims=True) * width + 1e-10 * 4e-6  # (a silent frame: log(1e-10) = -23 rounded to fp32, 2e-6 of it)
        lin = np.abs(np.exp(raw[b, :kept[b]].astype(np.float64)) - ref_lin) / bound
        print(f"SPECTRAL_BAND {kind}_{case} utt {b}: linear {lin.max():.3f} of its band")
        assert lin.max() <= 1.0
        assert not raw[b, kept[b]:].view(np.uint32).any()
        # and the CMVN on top is the float64 CMVN of these
        cnt = min(meta["counts"][b], meta["kept"][b])
        if 1 < meta["counts"][b] <= kept[b] and np.abs(w).max() > 0:
            err = np.abs(got[b, :cnt] - R.cmvn(raw[b, :meta["counts"][b]])[:cnt]).max()
            print(f"SPECTRAL_BAND {kind}_{case} utt {b}: cmvn {err:.2e}")
            assert err <= CMVN_TOL


# ---- the hub ------------------------------------------------------------------------------------------------------------------
def test_hub_entries_run_the_same_code():
    import torch

    import s3prl_amd.hub as hub
    from s3prl_amd.upstream.log_stft.hubconf import LOG_STFT_MAG, STFT_MAG

    kaldi = [torch.from_numpy(w).cuda() for w in kaldi_wavs(1.0)]
    for name in ("spectrogram", "mfcc"):
        expert = getattr(hub, name)().cuda().eval()
        res = expert(kaldi)
        assert res["last_hidden_state"] is res["hidden_states"][0] and len(res["hidden_states"]) == 1
        assert _same_bits(res["hidden_states"][0].cpu().numpy(), kaldi_run(name, 1.0, True)[0])
        assert expert.get_downsample_rates("hidden_states") == 160
        with pytest.raises(ValueError):
            expert([torch.zeros(399).cuda()])
    for cfg, log in ((STFT_MAG, False), (LOG_STFT_MAG, True)):
        expert = hub.stft_mag(cfg).cuda().eval()
        res = expert([torch.from_numpy(w).cuda() for w in stft_wavs()])
        assert isinstance(res["last_hidden_state"], list) and res["last_hidden_state"][0] is res["hidden_states"][0]
        assert _same_bits(res["hidden_states"][0].cpu().numpy(), stft_run(log)[0])
        assert expert.get_downsample_rates("hidden_states") == 320
        with pytest.raises(ValueError):
            expert([torch.zeros(256).cuda()])
    for name in ("linear", "mel"):
        meta, ref = _fixture(f"{name}_zero_tail")
        expert = getattr(hub, name)().cuda().eval()
        res = expert([torch.from_numpy(w).cuda() for w in R.fixture_wavs(meta)])
        assert tuple(res["last_hidden_state"].shape) == ref.shape
        _fixture_check(f"hub {name}", res["hidden_states"][0].cpu().numpy(), ref)
        with pytest.raises(ValueError):
            expert([torch.ones(200).cuda()])
