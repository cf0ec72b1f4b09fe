"""float64 restatement (numpy) of the five plain signal features: `spectrogram` and `mfcc` (torchaudio.compliance.kaldi behind
upstream/baseline/extracter.py:32-90), `linear` and `mel` (the OnlinePreprocessor, upstream/baseline/preprocessor.py:150-223, behind
upstream/baseline/expert.py:55-67) and `stft_mag` (upstream/log_stft/expert.py).  TEST INFRASTRUCTURE ONLY.

torchaudio is not installed, so the two kaldi functions are restated from their published definition (tests/test_spectral_cpu.py
pins them against transformers.audio_utils, scipy's DCT and oracle/fbank_oracle.py); the other three are pinned against fixtures
the reference's own code wrote (tests/golden/spectral)."""

import math

import numpy as np

from oracle import fbank_oracle as F

EPS32 = F.EPS32


# ---- kaldi -------------------------------------------------------------------------------------------------------------------
def kaldi_frames(wav, frame_length=25.0, frame_shift=10.0):
    """snip_edges frames, (T, size) float64, and the padded DFT length."""
    size, shift, padded = F.frame_params(frame_length, frame_shift)
    wav = np.asarray(wav, dtype=np.float64)
    T = F.num_frames(len(wav), size, shift)
    idx = shift * np.arange(T)[:, None] + np.arange(size)[None, :]
    return wav[idx].reshape(T, size), padded


def kaldi_power(wav, frame_length=25.0, frame_shift=10.0, preemph=0.97):
    """(T, padded / 2 + 1) power spectrum of the mean-removed, pre-emphasised, povey-windowed frames, and the frames' raw log
    energy (after the mean removal, before pre-emphasis and window) floored at log(1)."""
    frames, padded = kaldi_frames(wav, frame_length, frame_shift)
    frames = frames - frames.mean(axis=1, keepdims=True)
    energy = np.maximum(np.log(np.maximum((frames ** 2).sum(axis=1), EPS32)), 0.0)
    prev = np.concatenate([frames[:, :1], frames[:, :-1]], axis=1)
    spec = np.fft.rfft((frames - preemph * prev) * F.povey_window(frames.shape[1]), n=padded, axis=1)
    return spec.real ** 2 + spec.imag ** 2, energy


def kaldi_spectrogram(wav, frame_length=25.0, frame_shift=10.0, preemph=0.97):
    power, energy = kaldi_power(wav, frame_length, frame_shift, preemph)
    out = np.log(np.maximum(power, EPS32))
    out[:, 0] = energy
    return out


def dct_matrix(num_ceps, num_mel_bins):
    """create_dct(num_mel_bins, num_mel_bins, "ortho") with column 0 = sqrt(1 / num_mel_bins), first num_ceps columns."""
    n = np.arange(num_mel_bins, dtype=np.float64)[:, None]
    k = np.arange(num_ceps, dtype=np.float64)[None, :]
    M = np.cos(math.pi / num_mel_bins * (n + 0.5) * k) * math.sqrt(2.0 / num_mel_bins)
    M[:, 0] = math.sqrt(1.0 / num_mel_bins)
    return M


def lifter(num_ceps, Q=22.0):
    return 1.0 + 0.5 * Q * np.sin(math.pi * np.arange(num_ceps) / Q) if Q > 0 else np.ones(num_ceps)


def kaldi_logmel(wav, num_mel_bins=23, frame_length=25.0, frame_shift=10.0, preemph=0.97):
    power, _ = kaldi_power(wav, frame_length, frame_shift, preemph)
    banks = F.mel_banks(num_mel_bins, 2 * (power.shape[1] - 1), F.SAMPLE_RATE)
    return np.log(np.maximum(power @ banks.T, EPS32))


def kaldi_mfcc(wav, num_ceps=13, num_mel_bins=23, frame_length=25.0, frame_shift=10.0, preemph=0.97, Q=22.0):
    return kaldi_logmel(wav, num_mel_bins, frame_length, frame_shift, preemph) @ dct_matrix(num_ceps, num_mel_bins) * lifter(num_ceps, Q)


def cmvn(x, eps=1e-10):
    """per column over time, unbiased std, eps added to the std; one row -> nan (torch.std)."""
    x = np.asarray(x, dtype=np.float64)
    if x.shape[0] == 0:
        return x
    std = x.std(axis=0, ddof=1, keepdims=True) if x.shape[0] > 1 else np.full((1, x.shape[1]), np.nan)
    return (x - x.mean(axis=0, keepdims=True)) / (eps + std)


def deltas(x, order, win_length=5):
    feats = [x]
    for _ in range(order):
        feats.append(F.compute_deltas(feats[-1], win_length))
    return np.concatenate(feats, axis=-1)


def pad_batch(feats):
    T = max(f.shape[0] for f in feats)
    out = np.zeros((len(feats), T, feats[0].shape[1]))
    for b, f in enumerate(feats):
        out[b, :f.shape[0]] = f
    return out


def kaldi_forward(kind, wavs, order, use_cmvn=True, win_length=5, **kw):
    """get_extracter(...) per utterance + pad_sequence: kind "spectrogram" or "mfcc"."""
    fn = kaldi_spectrogram if kind == "spectrogram" else kaldi_mfcc
    feats = [deltas(fn(w, **kw), order, win_length) for w in wavs]
    return pad_batch([cmvn(f) if use_cmvn else f for f in feats])


# ---- stft_mag ----------------------------------------------------------------------------------------------------------------
def hann(n):
    return 0.5 - 0.5 * np.cos(2.0 * math.pi * np.arange(n) / n)


def centred_stft(row, n_fft, hop, win):
    """torch.stft(center = True, reflect, periodic hann(win) zero-padded to n_fft on both sides): (T, n_fft / 2 + 1) complex."""
    row = np.asarray(row, dtype=np.float64)
    if len(row) <= n_fft // 2:
        raise ValueError("reflect padding needs more than n_fft / 2 samples")
    x = np.pad(row, n_fft // 2, mode="reflect")
    T = 1 + len(row) // hop
    w = np.zeros(n_fft)
    w[(n_fft - win) // 2:(n_fft - win) // 2 + win] = hann(win)
    idx = hop * np.arange(T)[:, None] + np.arange(n_fft)[None, :]
    return np.fft.rfft(x[idx] * w, axis=1)


def stft_mag_forward(wavs, n_fft=512, hop=320, win=512, log=False):
    feats = [np.abs(centred_stft(w, n_fft, hop, win)) for w in wavs]
    return pad_batch([np.log(np.maximum(f, 1e-8)) if log else f for f in feats])


# ---- linear, mel: the OnlinePreprocessor behind the expert ---------------------------------------------------------------------
def htk_bank(n_mels, n_freq=201, f_max=8000.0):
    """torchaudio.functional.melscale_fbanks(n_freq, 0, f_max, n_mels, 16000, norm = None, "htk"): (n_freq, n_mels)."""
    hz2mel = lambda f: 2595.0 * np.log10(1.0 + f / 700.0)
    mel2hz = lambda m: 700.0 * (10.0 ** (m / 2595.0) - 1.0)
    f_pts = mel2hz(np.linspace(hz2mel(0.0), hz2mel(f_max), n_mels + 2))
    freqs = np.linspace(0.0, f_max, n_freq)
    slopes = f_pts[None, :] - freqs[:, None]
    d = np.diff(f_pts)
    return np.maximum(0.0, np.minimum(-slopes[:, :-2] / d[:-1], slopes[:, 2:] / d[1:]))


def trimmed_lengths(wavs):
    """preprocessor.py:164-171 on the zero-padded batch: 1 + the last non-zero index; an all-zero row keeps the batch length."""
    padded = max(len(w) for w in wavs)
    out = []
    for w in wavs:
        nz = np.flatnonzero(np.asarray(w))
        out.append(int(nz[-1]) + 1 if len(nz) else padded)
    return out


def preproc_rules(lengths, trimmed, use_cmvn=True):
    """(T, the CMVN's frame counts, the rows pad_sequence leaves, the rows the expert keeps): preprocessor.py:172-178 means to cut
    each row at its trimmed length but slices the channel axis of a (1, length) row, so the batch keeps its padded length and the
    trimmed lengths only reach the counts (preprocessor.py:204-215); expert.py:62-64 then keeps round(length * rows / lengths[0])."""
    mx = max(lengths)
    T = 1 + mx // 160
    rate = mx / T
    counts = [min(max(round(n / rate), 0), T) for n in trimmed] if use_cmvn else [T] * len(lengths)
    rows = max(counts)
    ratio = rows / lengths[0]
    kept = [min(round(n * ratio), rows) for n in lengths]
    return T, counts, rows, kept


def preproc_forward(kind, wavs, n_mels=80, use_cmvn=True):
    """kind "linear" (201 bins) or "mel" (n_mels HTK triangles): log(|X|^2 + 1e-10), CMVN, the expert's clipping."""
    lengths = [len(w) for w in wavs]
    T, counts, rows, kept = preproc_rules(lengths, trimmed_lengths(wavs), use_cmvn)
    feats = []
    for w, cnt, keep in zip(wavs, counts, kept):
        row = np.zeros(max(lengths))
        row[:len(w)] = np.asarray(w, dtype=np.float64)
        power = np.abs(centred_stft(row, 400, 160, 400)) ** 2
        f = np.log((power @ htk_bank(n_mels) if kind == "mel" else power) + 1e-10)
        if use_cmvn:
            f = np.concatenate([cmvn(f[:cnt]), np.zeros((T - cnt, f.shape[1]))], axis=0)
        feats.append(f[:keep])
    return pad_batch(feats)


# ---- the fixtures' inputs (tests/golden/spectral/*.npz meta -> waveforms) ----------------------------------------------------------
def fixture_wavs(meta):
    """synth_wavs(meta["lengths"], meta["wav_seed"]) in the order meta["order"], the last meta["zero_tail"][b] samples of utterance b
    (after re-ordering) set to exact zeros; zero_tail[b] = the whole length makes an all-zero utterance."""
    from s3prl_amd.synth import synth_wavs

    wavs = synth_wavs(meta["lengths"], meta["wav_seed"])
    wavs = [wavs[i].copy() for i in meta.get("order", range(len(wavs)))]
    for b, n in meta.get("zero_tail", {}).items():
        wavs[int(b)][len(wavs[int(b)]) - n:] = 0.0
    return wavs


# ---- what the CPU and the GPU tests share ------------------------------------------------------------------------------------------
OP_TOL = 2e-5                # the project's op bound
WELL = 1e-4                  # a bin is well-conditioned when its power is at least this fraction of its frame's largest
LOG_TOL = 2 * OP_TOL / math.sqrt(WELL)  # 4e-3: |d log P| of a well-conditioned bin; half of it for a log magnitude
MAX_LEFT_OUT = 0.05          # the log-domain check may leave out at most this fraction of an utterance's bins
KALDI_LENGTHS = [560, 879, 2000]  # tests/test_frontend_bits_gpu.py's FBANK_LENGTHS: two frames, three and a remainder, eleven
KALDI_SEED = 4400
STFT_LENGTHS = [257, 319, 320, 1000, 3200]
STFT_SEED = 4500


def left_out(power):
    """per frame, the bins under WELL of the frame's largest power: (T, nbin) bool."""
    return power < WELL * power.max(axis=1, keepdims=True)
