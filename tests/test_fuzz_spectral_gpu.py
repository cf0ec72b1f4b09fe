"""Seeded sweep over a dozen tiny configurations of the plain signal features s3enc_spectral_forward accepts, against the float64
restatement (tests/spectral_ref.py) from the waveforms, at the bands of tests/test_spectral_gpu.py generalised to the drawn sizes
(sqrt(num_mel_bins) for the DCT's unit-norm columns).  It varies num_ceps, num_mel_bins, the lifter, frame_length / frame_shift
and the delta order 0-2 (kaldi kinds); n_fft / hop / win and log on / off (stft_mag); n_mels (mel); CMVN on / off.  The fixtures of
tests/test_spectral_gpu.py pin the released settings against the reference itself; this guards the generality the entry promises."""

import numpy as np
import pytest

import spectral_ref as R
from test_spectral_gpu import CMVN_TOL, LOGMEL_BAND, _check_bins, _config, run

pytestmark = pytest.mark.gpu

N_SEEDS = 12
KINDS = ("spectrogram", "mfcc", "stft_mag", "mel", "mfcc", "linear")


def case(seed):
    """(kind, the config's fields, waveforms): the kinds cycle so that each appears, the rest is drawn."""
    from s3prl_amd.synth import synth_wavs

    rng = np.random.default_rng(9900 + seed)
    kind = KINDS[seed % len(KINDS)]
    kw = dict(use_cmvn=int(rng.integers(0, 2)))
    if kind in ("spectrogram", "mfcc"):
        kw.update(frame_length_ms=float(rng.choice([20.0, 25.0, 32.0])), frame_shift_ms=float(rng.choice([5.0, 10.0])),
                  delta_order=int(rng.integers(0, 3)))
        if kind == "mfcc":
            nmel = int(rng.choice([13, 23, 40]))
            kw.update(num_mel_bins=nmel, num_ceps=int(rng.integers(1, nmel + 1)), cepstral_lifter=float(rng.choice([0.0, 22.0])))
        low = 2 * 512  # at least two frames, so that the CMVN has a standard deviation
    elif kind == "stft_mag":
        n_fft = int(rng.choice([256, 400, 512]))
        kw.update(n_fft=n_fft, hop=int(rng.choice([80, 160, 320])), win=int(rng.choice([n_fft, n_fft // 2, n_fft - 56])),
                  log=int(rng.integers(0, 2)))
        low = n_fft // 2 + 1
    else:
        kw.update(num_mel_bins=int(rng.choice([16, 40, 80])))
        low = 400
    lengths = [int(rng.integers(low, 3000)) for _ in range(int(rng.integers(1, 4)))]
    return kind, kw, synth_wavs(lengths, seed + 1, scale=float(rng.choice([1.0, 0.1])))


@pytest.mark.parametrize("seed", range(N_SEEDS))
def test_random_spectral_config_matches_float64(seed):
    kind, kw, wavs = case(seed)
    c = _config(kind, **dict(kw, use_cmvn=0))
    raw, frames = run(c, wavs)
    tag = f"fuzz {seed} {kind}"
    if kind in ("spectrogram", "mfcc"):
        fl, fs, order = kw["frame_length_ms"], kw["frame_shift_ms"], kw["delta_order"]
        for b, w in enumerate(wavs):
            T = frames[b]
            assert T == R.kaldi_frames(w, fl, fs)[0].shape[0] and not raw[b, T:].view(np.uint32).any()
            if kind == "spectrogram":
                power, energy = R.kaldi_power(w, fl, fs)
                nb = power.shape[1]
                _check_bins(f"{tag} utt {b}", raw[b, :T, 1:nb], power[:, 1:], R.EPS32)
                assert (np.abs(np.exp(raw[b, :T, 0].astype(np.float64)) - np.exp(energy)) <= 2 * R.OP_TOL * np.exp(energy)).all()
                ref = R.deltas(R.kaldi_spectrogram(w, fl, fs), order)
                # the deltas are linear in their source: the ill-conditioned bins aside they sit at the log band
                well = np.tile(~R.left_out(power).any(axis=0), order + 1)
                well[::nb] = True
                assert np.abs(raw[b, :T] - ref)[:, well].max() <= R.LOG_TOL
            else:
                nmel, nceps, Q = kw["num_mel_bins"], kw["num_ceps"], kw["cepstral_lifter"]
                ref = R.deltas(R.kaldi_mfcc(w, nceps, nmel, fl, fs, Q=Q), order)
                band = np.tile(R.lifter(nceps, Q) * np.sqrt(nmel) * LOGMEL_BAND, order + 1)
                worst = (np.abs(raw[b, :T] - ref) / band).max()
                print(f"SPECTRAL_BAND {tag} utt {b}: {worst:.3f} of its band")
                assert worst <= 1.0
    elif kind == "stft_mag":
        for b, w in enumerate(wavs):
            T = frames[b]
            assert T == 1 + len(w) // kw["hop"] and not raw[b, T:].view(np.uint32).any()
            mag = np.abs(R.centred_stft(w, kw["n_fft"], kw["hop"], kw["win"]))
            if kw["log"]:
                _check_bins(f"{tag} utt {b}", raw[b, :T], mag, 1e-8, magnitude=True)
            else:
                assert (np.abs(raw[b, :T] - mag) <= R.OP_TOL * mag.max(axis=1, keepdims=True)).all()
        return  # (no CMVN in this family)
    else:
        lengths = [len(w) for w in wavs]
        T, _, _, kept = R.preproc_rules(lengths, R.trimmed_lengths(wavs), use_cmvn=False)
        assert frames == kept
        bank = R.htk_bank(kw["num_mel_bins"])
        for b, w in enumerate(wavs):
            row = np.zeros(max(lengths))
            row[:len(w)] = w
            power = (np.abs(R.centred_stft(row, 400, 160, 400)) ** 2)[:kept[b]]
            ref = (power @ bank if kind == "mel" else power) + 1e-10
            bound = 2 * R.OP_TOL * power.max(axis=1, keepdims=True) * (bank.sum(axis=0)[None, :] if kind == "mel" else 1.0) + 4e-16
            assert (np.abs(np.exp(raw[b, :kept[b]].astype(np.float64)) - ref) <= bound).all()
    if kw["use_cmvn"]:
        got, frames2 = run(_config(kind, **kw), wavs)
        if kind in ("spectrogram", "mfcc"):
            assert frames2 == frames
            for b, T in enumerate(frames):
                assert np.abs(got[b, :T] - R.cmvn(raw[b, :T])).max() <= CMVN_TOL and not got[b, T:].view(np.uint32).any()
        else:
            lengths = [len(w) for w in wavs]
            _, counts, rows, kept = R.preproc_rules(lengths, R.trimmed_lengths(wavs))
            assert frames2 == kept and got.shape[1] == max(kept)
            for b, cnt in enumerate(counts):
                n = min(cnt, kept[b], frames[b])
                if 1 < cnt <= frames[b]:
                    assert np.abs(got[b, :n] - R.cmvn(raw[b, :cnt])[:n]).max() <= CMVN_TOL
                assert not got[b, min(cnt, kept[b]):].view(np.uint32).any()
