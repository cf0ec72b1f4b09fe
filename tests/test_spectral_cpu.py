"""CPU checks of the plain signal features (`spectrogram`, `mfcc`, `mel`, `linear`, `stft_mag`): the float64 restatement
tests/spectral_ref.py against the reference's own outputs (tests/golden/spectral, written by make_golden_spectral.py) and, for the
two kaldi functions no torchaudio run can stand behind here, against independent code (transformers.audio_utils, scipy's DCT,
oracle/fbank_oracle.py); the hub names and signatures; every refusal; the frame-count rules."""

import glob
import inspect
import json
import os

import numpy as np
import pytest

import spectral_ref as R
from oracle import fbank_oracle as F

HERE = os.path.dirname(os.path.abspath(__file__))
SPECTRAL_DIR = os.path.join(HERE, "golden", "spectral")
RESTATEMENT_TOL = 1e-5  # tests/test_lighthubert_cpu.py's band for a float64 restatement against the reference's fp32 run
FIXTURES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(SPECTRAL_DIR, "*.npz")))


def load_fixture(name):
    z = np.load(os.path.join(SPECTRAL_DIR, name + ".npz"))
    return json.loads(bytes(z["meta"]).decode()), z["out"]


def restate(meta):
    if "kind" in meta:
        return R.preproc_forward(meta["kind"], R.fixture_wavs(meta))
    return R.stft_mag_forward(R.fixture_wavs(meta), log=meta["log"])


def test_the_fixture_set_is_complete():
    assert FIXTURES == sorted(["stft_mag_lin", "stft_mag_log"] + [f"{k}_{c}" for k in ("linear", "mel")
                                                                  for c in ("plain", "short_first", "zero_tail", "all_zero")])


@pytest.mark.parametrize("name", FIXTURES)
def test_restatement_matches_the_reference(name):
    meta, out = load_fixture(name)
    ref = restate(meta)
    assert ref.shape == out.shape
    for b in range(out.shape[0]):
        norm = np.linalg.norm(out[b].astype(np.float64))
        if norm == 0.0:
            # the all-zero utterance: the constant log(1e-10) = -23.03 under a CMVN whose std is its floor 1e-10.  The reference's
            # fp32 mean is exact; numpy's float64 mean may be one ulp(23.03) = 3.6e-15 off, which the floor turns into 3.6e-5
            assert np.abs(ref[b]).max() <= 2 * np.spacing(23.03) / 1e-10
            continue
        err = np.linalg.norm(ref[b] - out[b]) / norm
        print(f"SPECTRAL restatement {name} utt {b}: {err:.2e}")
        assert err < RESTATEMENT_TOL


def test_stft_fixture_shapes_and_padding():
    for name in ("stft_mag_lin", "stft_mag_log"):
        meta, out = load_fixture(name)
        assert meta["lengths"] == [3200, 1000, 319, 257] and out.shape == (4, 11, 257)
        for b, T in enumerate([11, 4, 1, 1]):
            assert not out[b, T:].any() and out[b, :T].any()
        assert meta["settings"]["spectrogram"] == dict(n_fft=512, hop_length=320, win_length=512, window="hann", center=True,
                                                       log=meta["log"])


def test_preprocessor_fixtures_hit_every_length_rule():
    rules = {c: load_fixture(f"linear_{c}")[0] for c in ("plain", "short_first", "zero_tail", "all_zero")}
    assert rules["plain"]["counts"] == [7, 6, 2] and rules["plain"]["kept"] == [7, 6, 2]
    assert rules["short_first"]["kept"] == [7, 7, 7]  # ratio 7 / 300: the clip at T binds for the two longer ones
    assert rules["zero_tail"]["trimmed"] == [830, 900, 300] and rules["zero_tail"]["T"] == 7 and rules["zero_tail"]["rows"] == 6
    assert rules["zero_tail"]["kept"] == [6, 5, 2]
    assert rules["all_zero"]["trimmed"] == [1000, 1000, 300]  # an all-zero row takes the padded batch length
    for kind in ("linear", "mel"):
        for c, meta in rules.items():
            out = load_fixture(f"{kind}_{c}")[1]
            assert out.shape == (3, max(meta["kept"]), 201 if kind == "linear" else 80)
            for b, (cnt, keep) in enumerate(zip(meta["counts"], meta["kept"])):
                assert not out[b, min(cnt, keep):].any()
        assert "stand-in" in load_fixture(f"{kind}_plain")[0]["stand_in"]


def test_frame_count_rules_and_bankers_rounding():
    # kaldi: snip_edges
    assert [F.num_frames(n) for n in (399, 400, 559, 560, 879, 2000)] == [0, 1, 1, 2, 3, 11]
    # stft_mag: 1 + n // 320
    assert [1 + n // 320 for n in (257, 319, 320, 1000, 3200)] == [1, 1, 2, 4, 11]
    assert R.stft_mag_forward([np.ones(257)]).shape == (1, 1, 257)
    with pytest.raises(ValueError):
        R.stft_mag_forward([np.ones(256)])
    # preprocessor: T = 1 + 1600 // 160 = 11, rate 1600 / 11; 800 / rate = 5.5 rounds to even 6?  No: 5.5 -> 6 is away from even 5?  Python: 6
    T, counts, rows, kept = R.preproc_rules([1600, 800], [1600, 800])
    assert (T, counts, rows) == (11, [11, round(800 / (1600 / 11))], 11)
    # halves to even: T = 5 rows over lengths[0] = 640 samples is 1 / 128 per sample; 320 -> 2.5 -> 2, 576 -> 4.5 -> 4, 448 -> 3.5 -> 4
    assert round(2.5) == 2 and round(3.5) == 4 and round(4.5) == 4
    T, counts, rows, kept = R.preproc_rules([640, 320, 576, 448], [640, 320, 576, 448])
    assert T == 5 and rows == 5 and kept == [5, 2, 4, 4]
    assert counts == [5, 2, 4, 4]  # the same halves in the CMVN's counts: rate = 640 / 5 = 128
    # without CMVN nothing is cut by the counts
    assert R.preproc_rules([1000, 900, 300], [830, 900, 300], use_cmvn=False) == (7, [7, 7, 7], 7, [7, 6, 2])


def test_kaldi_power_and_logmel_match_transformers():
    au = pytest.importorskip("transformers.audio_utils")
    rng = np.random.default_rng(0)
    window = au.window_function(400, "povey", periodic=False)
    mel23 = au.mel_filter_bank(num_frequency_bins=257, num_mel_filters=23, min_frequency=20, max_frequency=8000, sampling_rate=16000,
                               norm=None, mel_scale="kaldi", triangularize_in_mel_space=True)
    for n in (2000, 16000 + 137, 400):
        wav = rng.standard_normal(n)
        kw = dict(frame_length=400, hop_length=160, fft_length=512, power=2.0, center=False, preemphasis=0.97, remove_dc_offset=True,
                  dtype=np.float64)
        power = au.spectrogram(wav, window, **kw).T
        got, _ = R.kaldi_power(wav)
        assert got.shape == power.shape == (F.num_frames(n), 257)
        assert np.abs(got - power).max() <= 1e-6 * power.max()  # (its FFT buffer is complex64)
        logmel = au.spectrogram(wav, window, mel_filters=mel23, log_mel="log", mel_floor=1.192092955078125e-07, **kw).T
        assert np.abs(R.kaldi_logmel(wav) - logmel).max() < 1e-5


def test_logmel_in_front_of_the_dct_is_the_fbank_oracle_at_23_bins():
    wav = np.random.default_rng(1).standard_normal(3000)
    assert np.abs(R.kaldi_logmel(wav) - F.kaldi_fbank(wav, num_mel_bins=23)).max() < 1e-12


def test_dct_and_lifter_match_scipy():
    fft = pytest.importorskip("scipy.fft")
    x = np.random.default_rng(2).standard_normal((7, 23))
    ref = fft.dct(x, type=2, norm="ortho", axis=1)[:, :13]
    assert np.abs(x @ R.dct_matrix(13, 23) - ref).max() < 1e-12
    lift = R.lifter(13)
    assert lift[0] == 1.0 and abs(lift[11] - (1 + 11 * np.sin(np.pi * 11 / 22))) < 1e-12 and abs(lift[11] - 12.0) < 1e-12
    M = R.dct_matrix(23, 23)
    assert np.abs(M.T @ M - np.eye(23)).max() < 1e-12  # unit-norm columns: the GPU band sqrt(23) * 2e-4 rests on it


def test_spectrogram_energy_bin_and_floor():
    wav = np.random.default_rng(3).standard_normal(1000)
    s = R.kaldi_spectrogram(wav)
    frames, _ = R.kaldi_frames(wav)
    frames = frames - frames.mean(axis=1, keepdims=True)
    assert np.allclose(s[:, 0], np.log((frames ** 2).sum(axis=1))) and (s[:, 0] > 0).all()  # ~ log 400: the floor never binds
    quiet = R.kaldi_spectrogram(wav * 1e-2)
    assert (quiet[:, 0] == 0.0).all()  # 400 * 1e-4 < 1: floored at log(energy_floor = 1)
    assert R.kaldi_forward("spectrogram", [wav], 0).shape == (1, 4, 257)
    assert R.kaldi_forward("mfcc", [wav], 2).shape == (1, 4, 39)
    one = R.kaldi_forward("mfcc", [wav[:400]], 2)
    assert one.shape == (1, 1, 39) and np.isnan(one).all()  # one frame under the CMVN


def test_left_out_fraction_of_the_gpu_tests_inputs():
    """The log-domain band of tests/test_spectral_gpu.py covers the well-conditioned bins only; for the exact seeds it uses the
    float64 restatement alone leaves out 1.7-2.5 % (kaldi operand) and 0.3-3.5 % (hann STFT; the most in the one-frame
    utterances), under the 5 % the test allows."""
    from s3prl_amd.synth import synth_wavs

    for scale in (1.0, 1e-2):
        for wav in synth_wavs(R.KALDI_LENGTHS, R.KALDI_SEED, scale=scale):
            frac = R.left_out(R.kaldi_power(wav)[0]).mean()
            print(f"SPECTRAL left out, kaldi {len(wav)} x {scale}: {frac:.4f}")
            assert frac <= R.MAX_LEFT_OUT
    for wav in synth_wavs(R.STFT_LENGTHS, R.STFT_SEED):
        frac = R.left_out(np.abs(R.centred_stft(wav, 512, 320, 512)) ** 2).mean()
        print(f"SPECTRAL left out, stft {len(wav)}: {frac:.4f}")
        assert frac <= R.MAX_LEFT_OUT


# ---- the hub ------------------------------------------------------------------------------------------------------------------
def test_hub_names_and_signatures():
    import s3prl_amd.hub as hub

    ref = json.load(open(os.path.join(HERE, "golden", "reference_hub.json")))
    rec = json.load(open(os.path.join(SPECTRAL_DIR, "reference_hub_spectral.json")))
    names = [(n, params) for entries in rec["hubconfs"].values() for n, params in entries]
    assert sorted(n for n, _ in names) == ["linear", "mel", "mfcc", "spectrogram", "stft_mag"]
    for name, params in names:
        assert name in ref["options"] and name in ref["registered_ckpt_options"]
        assert name in hub.options() and name in hub.options(only_registered_ckpt=True)
        ours = inspect.signature(getattr(hub, name))
        assert [list(p) for p in params] == [[k, v.kind.name, repr(v.default)] for k, v in ours.parameters.items()], name
    for name in ("spectrogram", "mfcc", "mel", "linear"):
        expert = getattr(hub, name)()
        assert expert.output_dim == rec["output_dims"][name] and expert.get_downsample_rates("hidden_states") == 160
    from s3prl_amd.upstream.log_stft.hubconf import LOG_STFT_MAG, STFT_MAG

    for cfg in (STFT_MAG, LOG_STFT_MAG):
        expert = hub.stft_mag(cfg)
        assert expert.output_dim == 257 and expert.get_downsample_rates("hidden_states") == 320
        assert cfg == load_fixture("stft_mag_log" if cfg["spectrogram"]["log"] else "stft_mag_lin")[0]["settings"]
    # the hubconf's dicts are the reference's yaml settings, as the fixtures recorded them
    from s3prl_amd.upstream.baseline import hubconf as base

    assert base._preprocessor_config("linear") == load_fixture("linear_plain")[0]["settings"]
    assert base._preprocessor_config("mel") == load_fixture("mel_plain")[0]["settings"]
    # the fbank entries are what they were
    assert hub.fbank().output_dim == 240 and hub.baseline().output_dim == 240


def test_baseline_local_takes_a_yaml_file(tmp_path):
    import yaml

    import s3prl_amd.hub as hub
    from s3prl_amd.upstream.baseline import hubconf as base

    path = tmp_path / "mfcc.yaml"
    path.write_text(yaml.safe_dump(base._kaldi_config("mfcc", {"num_ceps": 13}, 2)))
    assert hub.baseline_local(str(path)).output_dim == 39
    path = tmp_path / "log_stft_mag.yaml"
    path.write_text(yaml.safe_dump({"feat_type": "spectrogram", "spectrogram": dict(n_fft=512, hop_length=320, win_length=512,
                                                                                   window="hann", center=True, log=True)}))
    assert hub.stft_mag(str(path)).output_dim == 257


def _kaldi(kind, **options):
    return {"kaldi": {"feat_type": kind, kind: dict(options)}, "delta": {"order": 0, "win_length": 5}, "cmvn": {"use_cmvn": True}}


def _preproc(top=None, **feat):
    return dict({"win_ms": 25, "hop_ms": 10, "n_freq": 201, "n_mels": 80,
                 "input": dict({"feat_type": "mel", "channel": 0, "log": True, "delta": 0, "cmvn": True}, **feat)}, **(top or {}))


@pytest.mark.parametrize("config, named", [
    (_kaldi("spectrogram", dither=1.0), "dither"),
    (_kaldi("spectrogram", snip_edges=False), "snip_edges"),
    (_kaldi("mfcc", use_energy=True), "use_energy"),
    (_kaldi("spectrogram", subtract_mean=True), "subtract_mean"),
    (_kaldi("mfcc", htk_compat=True), "htk_compat"),
    (_kaldi("mfcc", vtln_warp=1.1), "vtln_warp"),
    (_kaldi("spectrogram", window_type="hamming"), "window_type"),
    (_kaldi("spectrogram", raw_energy=False), "raw_energy"),
    (_kaldi("spectrogram", sample_frequency=8000.0), "sample_frequency"),
    (_kaldi("plp"), "plp"),
    (_preproc(feat_type="wav"), "feat_type"),
    (_preproc(feat_type="complx"), "feat_type"),
    (_preproc(feat_type="phase"), "feat_type"),
    (_preproc(feat_type="mfcc"), "feat_type"),
    (_preproc(delta=1), "delta"),
    (_preproc(log=False), "log"),
    (_preproc(top={"target": {"feat_type": "mel"}}), "target"),
    (_preproc(top={"sample_rate": 8000}), "sample_rate"),
    (_preproc(top={"hop_ms": 20}), "hop_ms"),
])
def test_baseline_refusals_name_the_option(config, named):
    import s3prl_amd.hub as hub

    with pytest.raises(NotImplementedError, match=named):
        hub.baseline_local(config)


def test_stated_kaldi_defaults_are_accepted():
    import s3prl_amd.hub as hub

    assert hub.baseline_local(_kaldi("spectrogram", dither=0.0, snip_edges=True, raw_energy=True, energy_floor=1.0)).output_dim == 257
    assert hub.baseline_local(_kaldi("mfcc", use_energy=False, num_mel_bins=23, cepstral_lifter=22.0)).output_dim == 13


@pytest.mark.parametrize("change, named", [(dict(window="hamming"), "window"), (dict(center=False), "center"),
                                           (dict(hop_length=322), "hop_length")])
def test_stft_mag_refusals_name_the_option(change, named):
    import s3prl_amd.hub as hub
    from s3prl_amd.upstream.log_stft.hubconf import STFT_MAG

    with pytest.raises(NotImplementedError, match=named):
        hub.stft_mag({"feat_type": "spectrogram", "spectrogram": dict(STFT_MAG["spectrogram"], **change)})
    with pytest.raises(NotImplementedError, match="sample_rate"):
        hub.stft_mag(dict(STFT_MAG, sample_rate=8000))


def test_no_cpu_fallback_and_the_c_entry_refuses_what_the_expert_does():
    import ctypes as C

    import torch

    import s3prl_amd.hub as hub
    from s3prl_amd import _lib

    for expert in (hub.mfcc(), hub.linear(), hub.stft_mag({"feat_type": "spectrogram", "spectrogram": dict(
            n_fft=512, hop_length=320, win_length=512, window="hann", center=True, log=True)})):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            expert([torch.zeros(4000)])
    lib = _lib.load()
    frames = (C.c_int32 * 2)()
    lens = (C.c_int64 * 2)(399, 2000)
    c = hub.spectrogram()._spectral
    assert lib.s3enc_spectral_num_frames(C.byref(c), None, lens, 2, frames, 0, None) == 0 and list(frames) == [0, 11]
    c = hub.stft_mag({"feat_type": "spectrogram", "spectrogram": dict(n_fft=512, hop_length=320, win_length=512, window="hann",
                                                                      center=True, log=False)})._c
    lens = (C.c_int64 * 2)(256, 257)
    assert lib.s3enc_spectral_num_frames(C.byref(c), None, lens, 2, frames, 0, None) == 0 and list(frames) == [0, 1]
    c.sample_rate = 8000
    assert lib.s3enc_spectral_num_frames(C.byref(c), None, lens, 2, frames, 0, None) != 0 and b"sample_rate" in lib.s3enc_last_error()
    c.sample_rate, c.kind = 16000, 9
    assert lib.s3enc_spectral_num_frames(C.byref(c), None, lens, 2, frames, 0, None) != 0 and b"unknown kind" in lib.s3enc_last_error()
    c = hub.mel()._spectral
    c.log = 0
    assert lib.s3enc_spectral_num_frames(C.byref(c), None, lens, 2, frames, 0, None) != 0 and b"log" in lib.s3enc_last_error()


def test_struct_layout_matches_header(tmp_path):
    import ctypes as C
    import subprocess

    from s3prl_amd import _lib

    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "s3enc.h"\nint main(void){printf("%zu %zu %zu %zu\\n", '
                   'sizeof(s3enc_spectral_config), offsetof(s3enc_spectral_config, cepstral_lifter), '
                   'offsetof(s3enc_spectral_config, log), offsetof(s3enc_spectral_config, win));return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(os.path.dirname(HERE), "include"), str(src), "-o", str(exe)],
                   check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    S = _lib.S3SpectralConfig
    assert got == [C.sizeof(S), S.cepstral_lifter.offset, S.log.offset, S.win.offset]
