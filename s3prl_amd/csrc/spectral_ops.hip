// spectral_ops.hip — the entry points of the plain signal features (s3enc_spectral_*): `spectrogram` and `mfcc` of
// torchaudio.compliance.kaldi (upstream/baseline/extracter.py), `linear` and `mel` of the OnlinePreprocessor
// (upstream/baseline/preprocessor.py behind expert.py:55-67) and `stft_mag` (upstream/log_stft/expert.py).  Every spectrum is the
// overlapping-row exact-fp32 GEMM against a host-folded operand (fbank.hip's, logmel.hip's, or hann x DFT at n_fft); what stands
// behind the DFT is spectral.h's:
//   spectrogram  gemm -> launch_frame_energy (PCM -> log energy) -> spectrum_rows<POWER, LogFloor> (bin 0 = energy) -> delta -> cmvn
//   mfcc         gemm -> mel_dct_rows_kernel (|X|^2 -> 23 mel -> log -> DCT x lifter)                               -> delta -> cmvn
//   linear, mel  launch_last_nonzero -> (host: the CMVN's counts, the rows kept) -> launch_logmel without the level scaling -> rows kept
//   stft_mag     launch_reflect_pad_one per utterance -> one batched gemm -> spectrum_rows<MAGNITUDE, ClampLog | Identity>
#include <cmath>
#include <map>
#include <mutex>

#include "engine_internal.h"
#include "spectral.h"

namespace s3 {
namespace {

// grow-only device buffers per (device, stream), like fbank.hip's: re-use within a stream is stream-ordered
struct Grow {
    void* p = nullptr;
    size_t bytes = 0;
    hipError_t ensure(size_t n) {
        if (n <= bytes) return hipSuccess;
        if (p) (void)hipFree(p);  // device-synchronising: nothing in flight still uses it
        p = nullptr;
        bytes = 0;
        const hipError_t e = hipMalloc(&p, n + n / 4 + 64);
        if (e == hipSuccess) bytes = n + n / 4;
        return e;
    }
};
struct SpectralScratch {
    Grow spec, sig, energy, tbl, last, feat;
};
struct StftPlan {
    float* dft = nullptr;  // (2 (n_fft / 2 + 1), n_fft): the periodic hann(win) centred in n_fft x the DFT
};
struct DctPlan {
    float* m = nullptr;  // (num_ceps, num_mel_bins), the lifter folded in
};
std::mutex g_mu;
std::map<std::pair<int, uintptr_t>, SpectralScratch> g_scratch;
std::map<std::vector<long>, StftPlan> g_stft;
std::map<std::vector<long>, DctPlan> g_dct;

bool kaldi_kind(int k) { return k == S3ENC_SPECTRAL_SPECTROGRAM || k == S3ENC_SPECTRAL_MFCC; }
bool preproc_kind(int k) { return k == S3ENC_SPECTRAL_LINEAR || k == S3ENC_SPECTRAL_MEL; }

FbankParams kaldi_params(const s3enc_spectral_config& c) {
    FbankParams f;
    f.sample_rate = c.sample_rate;
    f.num_mel_bins = c.kind == S3ENC_SPECTRAL_MFCC ? c.num_mel_bins : 1;  // the spectrogram reads the operand only
    f.frame_length_ms = c.frame_length_ms;
    f.frame_shift_ms = c.frame_shift_ms;
    f.preemph = c.preemphasis;
    f.delta_order = c.delta_order;
    f.delta_win = c.delta_win_length;
    f.use_cmvn = c.use_cmvn;
    f.cmvn_eps = c.cmvn_eps;
    return f;
}

// null, or why the configuration is refused
const char* refusal(const s3enc_spectral_config& c) {
    if (c.sample_rate != 16000) return "sample_rate must be 16000";
    if (kaldi_kind(c.kind)) {
        const int size = (int)(c.sample_rate * c.frame_length_ms * 0.001), shift = (int)(c.sample_rate * c.frame_shift_ms * 0.001);
        if (size < 4 || size > 1024 || shift <= 0 || (size & 3) || (shift & 3)) return "the frame length and shift must be multiples of 4 samples, the length at most 1024";
        if (c.delta_order < 0 || c.delta_order > 2 || c.delta_win_length < 3 || !(c.delta_win_length & 1)) return "unsupported delta configuration";
        if (c.kind == S3ENC_SPECTRAL_MFCC) {
            if (c.num_mel_bins < 1 || c.num_mel_bins > 256) return "num_mel_bins must be in 1..256";
            if (c.num_ceps < 1 || c.num_ceps > c.num_mel_bins) return "num_ceps must be in 1..num_mel_bins";
            if (!(c.cepstral_lifter >= 0.f)) return "cepstral_lifter must not be negative";
        }
        return nullptr;
    }
    if (preproc_kind(c.kind)) {
        if (c.n_fft != 400 || c.hop != 160 || c.win != 400) return "linear and mel are built at n_fft 400, hop 160, win 400";
        if (!c.log) return "linear and mel without log are not implemented";
        if (c.kind == S3ENC_SPECTRAL_MEL && (c.num_mel_bins < 1 || c.num_mel_bins > 256)) return "num_mel_bins must be in 1..256";
        return nullptr;
    }
    if (c.kind == S3ENC_SPECTRAL_STFT_MAG) {
        if (c.n_fft < 8 || c.n_fft > 4096 || (c.n_fft & 3) || c.hop <= 0 || (c.hop & 3)) return "n_fft (8..4096) and hop must be multiples of 4";
        if (c.win < 1 || c.win > c.n_fft) return "win must be in 1..n_fft";
        return nullptr;
    }
    return "unknown kind";
}

int feature_dim(const s3enc_spectral_config& c) {
    if (c.kind == S3ENC_SPECTRAL_SPECTROGRAM) {
        int padded = 1;
        while (padded < (int)(c.sample_rate * c.frame_length_ms * 0.001)) padded <<= 1;
        return (padded / 2 + 1) * (c.delta_order + 1);
    }
    if (c.kind == S3ENC_SPECTRAL_MFCC) return c.num_ceps * (c.delta_order + 1);
    if (c.kind == S3ENC_SPECTRAL_LINEAR) return 201;
    if (c.kind == S3ENC_SPECTRAL_MEL) return c.num_mel_bins;
    return c.n_fft / 2 + 1;
}

hipError_t overlapping_gemm(const float* a, int lda, const float* W, long T, int N2, int K, float* spec, hipStream_t st) {
    GemmParams g{};
    g.A = a;
    g.lda = lda;  // overlapping rows: frame t starts at sample t * lda
    g.W = W;
    g.M = (int)T;
    g.N = N2;
    g.K = K;
    g.batches = 1;
    g.out32 = spec;
    g.ldo = N2;
    return launch_gemm(F32, g, st);
}

// one kaldi utterance: wav (device, n samples, T >= 1 frames) -> out (T rows of pitch F)
hipError_t kaldi_one(const s3enc_spectral_config& c, const FbankParams& f, const FbankOperand& op, const float* dct, SpectralScratch& sc,
                     const float* wav, long n, long T, float* out, int F, hipStream_t st) {
    const int N2 = 2 * op.nbin;
    hipError_t e = sc.spec.ensure((size_t)T * N2 * 4);
    if (e != hipSuccess) return e;
    const float* a = wav;
    if (((uintptr_t)wav) & 15) {  // the GEMM loads 16-byte vectors: stage a misaligned waveform once
        e = sc.sig.ensure((size_t)n * 4);
        if (e != hipSuccess) return e;
        e = hipMemcpyAsync(sc.sig.p, wav, (size_t)n * 4, hipMemcpyDeviceToDevice, st);
        if (e != hipSuccess) return e;
        a = (const float*)sc.sig.p;
    }
    e = overlapping_gemm(a, op.shift, op.dft, T, N2, op.size, (float*)sc.spec.p, st);
    if (e != hipSuccess) return e;
    int cols;
    if (c.kind == S3ENC_SPECTRAL_SPECTROGRAM) {
        cols = op.nbin;
        e = sc.energy.ensure((size_t)T * 4);
        if (e != hipSuccess) return e;
        launch_frame_energy(wav, T, op.size, op.shift, FLT_EPSILON, 0.f /* log(energy_floor = 1) */, (float*)sc.energy.p, st);
        launch_spectrum_rows<POWER>((const float*)sc.spec.p, op.nbin, T, 1, LogFloor{FLT_EPSILON}, (const float*)sc.energy.p, out, (long)F, 0L,
                                    st);
    } else {
        cols = c.num_ceps;
        hipLaunchKernelGGL((mel_dct_rows_kernel<LogFloor>), dim3((unsigned)T), dim3(128), (op.nbin + c.num_mel_bins) * sizeof(float), st,
                           (const float*)sc.spec.p, op.nbin, op.bank.bands, op.bank.wts, c.num_mel_bins, LogFloor{FLT_EPSILON}, dct,
                           c.num_ceps, out, (long)F);
    }
    if (c.delta_order > 0) launch_fbank_delta(out, T, cols, F, c.delta_order, c.delta_win_length, st);
    if (c.use_cmvn) launch_cmvn(out, nullptr, (int)T, F, 1, F, 0, c.cmvn_eps, st);
    return hipGetLastError();
}

// stft_mag: every utterance reflect-padded about its own ends into its row of sig (B, Lp), ONE batched GEMM over max T frames
// of every row (a per-utterance GEMM of a few hundred frames fills a quarter of the device and is bound by its latency), then the
// utterance's own T rows through the epilogue; the rows behind stay the zeros of the memset
hipError_t stft_batch(const s3enc_spectral_config& c, const float* dft, SpectralScratch& sc, const float* const* wavs, const int64_t* lengths,
                      int B, float* out, long T_max, hipStream_t st) {
    const int nbin = c.n_fft / 2 + 1, N2 = 2 * nbin;
    long n_max = 0;
    for (int b = 0; b < B; ++b) n_max = std::max(n_max, (long)lengths[b]);
    const long Tm = 1 + n_max / c.hop;
    const long Lp = (n_max + c.n_fft + 3) & ~3L;  // frame t reads [t hop, t hop + n_fft), t hop <= n_max
    hipError_t e = sc.spec.ensure((size_t)B * Tm * N2 * 4);
    if (e != hipSuccess) return e;
    e = sc.sig.ensure((size_t)B * Lp * 4);
    if (e != hipSuccess) return e;
    for (int b = 0; b < B; ++b) launch_reflect_pad_one(wavs[b], lengths[b], c.n_fft / 2, Lp, (float*)sc.sig.p + b * Lp, st);
    GemmParams g{};
    g.A = sc.sig.p;
    g.lda = c.hop;  // overlapping rows: frame t starts at padded sample t * hop
    g.a_bs = Lp;
    g.W = dft;
    g.M = (int)Tm;
    g.N = N2;
    g.K = c.n_fft;
    g.batches = B;
    g.out32 = (float*)sc.spec.p;
    g.ldo = N2;
    g.o_bs = Tm * N2;
    e = launch_gemm(F32, g, st);
    if (e != hipSuccess) return e;
    for (int b = 0; b < B; ++b) {
        const float* spec = (const float*)sc.spec.p + (size_t)b * Tm * N2;
        float* o = out + (size_t)b * T_max * nbin;
        const long T = 1 + lengths[b] / c.hop;
        if (c.log)
            launch_spectrum_rows<MAGNITUDE>(spec, nbin, T, 1, ClampLog{1e-8f}, nullptr, o, (long)nbin, 0L, st);
        else
            launch_spectrum_rows<MAGNITUDE>(spec, nbin, T, 1, Identity{}, nullptr, o, (long)nbin, 0L, st);
    }
    return hipGetLastError();
}

// linear / mel: the reference's length rules on the host (the stream is synchronised), the device table (pointers | lengths |
// counts) left in sc.tbl.  preprocessor.py:164-178 finds L'[b] = 1 + the last non-zero index (an all-zero row: the batch length) and
// means to cut each row there, but slices the CHANNEL axis of its (1, length) rows, so the batch keeps its length: the frames are
// those of the caller's zero-padded batch, T = 1 + max length / 160, and L' only sets the CMVN's counts round(L' / (max length / T)).
// With CMVN pad_sequence cuts the batch to the largest count, `rows`; the expert keeps min(round(length (rows / lengths[0])), rows)
struct PreprocRows {
    long max_len = 0, T = 0, rows = 0;
    std::vector<int> counts, kept;
};
int preproc_rows(const s3enc_spectral_config& c, const float* const* wavs, const int64_t* lengths, int B, SpectralScratch& sc, hipStream_t st,
                 PreprocRows& r) {
    for (int b = 0; b < B; ++b) r.max_len = std::max(r.max_len, (long)lengths[b]);
    r.T = logmel_num_frames(r.max_len);
    const size_t o_len = (size_t)B * 8, o_cnt = 2 * (size_t)B * 8;
    std::vector<char> host(o_cnt + (size_t)B * 4, 0);
    std::vector<long> trimmed(B, 0);
    for (int b = 0; b < B; ++b) {
        ((const float**)host.data())[b] = wavs[b];
        ((long*)(host.data() + o_len))[b] = (long)lengths[b];
        ((int*)(host.data() + o_cnt))[b] = (int)r.T;
    }
    HIP_TRY(sc.tbl.ensure(host.size()));
    HIP_TRY(sc.last.ensure((size_t)B * 8));
    HIP_TRY(hipMemcpyAsync(sc.tbl.p, host.data(), host.size(), hipMemcpyHostToDevice, st));
    r.counts.assign(B, (int)r.T);
    r.rows = r.T;
    if (c.use_cmvn) {
        launch_last_nonzero((const float* const*)sc.tbl.p, (const long*)((char*)sc.tbl.p + o_len), B, r.max_len, (long*)sc.last.p, st);
        HIP_TRY(hipMemcpyAsync(trimmed.data(), sc.last.p, (size_t)B * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        r.rows = 0;
        for (int b = 0; b < B; ++b) {
            r.counts[b] = logmel_frame_count(trimmed[b], r.max_len);
            r.rows = std::max(r.rows, (long)r.counts[b]);
            ((int*)(host.data() + o_cnt))[b] = r.counts[b];
        }
        HIP_TRY(hipMemcpyAsync(sc.tbl.p, host.data(), host.size(), hipMemcpyHostToDevice, st));
    }
    HIP_TRY(hipStreamSynchronize(st));  // `host` goes out of scope
    r.kept.resize(B);
    for (int b = 0; b < B; ++b) r.kept[b] = (int)preproc_rows_kept((long)lengths[b], (long)lengths[0], r.rows);
    return 0;
}

int check_batch(const char* who, const s3enc_spectral_config* cfg, const int64_t* lengths, int B) {
    if (!cfg || !lengths) return fail(std::string(who) + ": null argument");
    if (B <= 0 || B > 65535) return fail(std::string(who) + ": bad batch size");
    if (const char* why = refusal(*cfg)) return fail(std::string(who) + ": " + why);
    for (int b = 0; b < B; ++b)
        if (lengths[b] <= 0) return fail(std::string(who) + ": empty utterance");
    return 0;
}

}  // namespace
}  // namespace s3

using namespace s3;

extern "C" {

int s3enc_spectral_num_frames(const s3enc_spectral_config* cfg, const float* const* wavs, const int64_t* lengths, int32_t B,
                              int32_t* frames, int32_t device, void* stream) {
    if (!frames) return fail("s3enc_spectral_num_frames: null argument");
    if (int rc = check_batch("s3enc_spectral_num_frames", cfg, lengths, B)) return rc;
    if (kaldi_kind(cfg->kind)) {
        const FbankParams f = kaldi_params(*cfg);
        for (int b = 0; b < B; ++b) frames[b] = (int32_t)fbank_num_frames(lengths[b], f);
        return 0;
    }
    if (cfg->kind == S3ENC_SPECTRAL_STFT_MAG) {
        for (int b = 0; b < B; ++b) frames[b] = lengths[b] > cfg->n_fft / 2 ? (int32_t)(1 + lengths[b] / cfg->hop) : 0;
        return 0;
    }
    if (!wavs) return fail("s3enc_spectral_num_frames: linear and mel need the waveforms (the last non-zero sample decides)");
    for (int b = 0; b < B; ++b) {
        if (!wavs[b]) return fail("s3enc_spectral_num_frames: null waveform pointer");
        if (lengths[b] <= 200) return fail("s3enc_spectral_num_frames: an utterance of at most 200 samples has no reflect-padded centred frame");
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail("s3enc_spectral_num_frames: no HIP device (there is no CPU fallback)");
    DeviceGuard dg(device);
    if (!dg.ok) return fail("s3enc_spectral_num_frames: hipSetDevice failed");
    std::lock_guard<std::mutex> lock(g_mu);
    PreprocRows r;
    if (int rc = preproc_rows(*cfg, wavs, lengths, B, g_scratch[std::make_pair((int)device, (uintptr_t)stream)], (hipStream_t)stream, r)) return rc;
    for (int b = 0; b < B; ++b) frames[b] = r.kept[b];
    return 0;
}

int s3enc_spectral_forward(const s3enc_spectral_config* cfg, const float* const* wavs, const int64_t* lengths, int32_t B, float* out,
                           int64_t T_max, int32_t device, void* stream) {
    if (!wavs || !out) return fail("s3enc_spectral_forward: null argument");
    if (int rc = check_batch("s3enc_spectral_forward", cfg, lengths, B)) return rc;
    const s3enc_spectral_config& c = *cfg;
    for (int b = 0; b < B; ++b)
        if (!wavs[b]) return fail("s3enc_spectral_forward: null waveform pointer");
    if (preproc_kind(c.kind))
        for (int b = 0; b < B; ++b)
            if (lengths[b] <= 200) return fail("s3enc_spectral_forward: an utterance of at most 200 samples has no reflect-padded centred frame");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail("s3enc_spectral_forward: no HIP device (there is no CPU fallback)");
    DeviceGuard dg(device);
    if (!dg.ok) return fail("s3enc_spectral_forward: hipSetDevice failed");
    hipStream_t st = (hipStream_t)stream;
    const int F = feature_dim(c);
    if (T_max <= 0 || (long)B * T_max > 0x7fffffffL / (2 * F + 2)) return fail("s3enc_spectral_forward: bad T_max or batch too large");
    std::lock_guard<std::mutex> lock(g_mu);
    SpectralScratch& sc = g_scratch[std::make_pair((int)device, (uintptr_t)stream)];

    if (preproc_kind(c.kind)) {
        PreprocRows r;
        if (int rc = preproc_rows(c, wavs, lengths, B, sc, st, r)) return rc;
        if (r.rows > T_max) return fail("s3enc_spectral_forward: T_max is smaller than the batch's frame count");
        // all T frames of every utterance are written: into `out` itself when its pitch is T rows (no count cut the batch), else
        // into scratch; the expert keeps the first kept[b] rows (expert.py:62-64) and pad_sequence puts zeros behind
        const bool in_place = T_max == r.T;
        if (!in_place) {
            HIP_TRY(hipMemsetAsync(out, 0, (size_t)B * T_max * F * sizeof(float), st));
            HIP_TRY(sc.feat.ensure((size_t)B * r.T * F * 4));
        }
        HIP_TRY(sc.sig.ensure(logmel_sig_elems(B, r.max_len) * 4));
        HIP_TRY(sc.spec.ensure(logmel_spec_elems(B, r.max_len) * 4));
        LogmelParams p{};
        p.wavs = (const float* const*)sc.tbl.p;
        p.lens = (const long*)((char*)sc.tbl.p + (size_t)B * 8);
        p.counts = (const int*)((char*)sc.tbl.p + 2 * (size_t)B * 8);
        p.B = B;
        p.max_len = r.max_len;
        p.n_mels = c.num_mel_bins;
        p.cmvn = c.use_cmvn;
        p.sig = (float*)sc.sig.p;
        p.spec = (float*)sc.spec.p;
        p.out = in_place ? out : (float*)sc.feat.p;
        p.o_bs = r.T * F;
        p.no_level = 1;
        p.linear = c.kind == S3ENC_SPECTRAL_LINEAR;
        HIP_TRY(launch_logmel(p, st));
        for (int b = 0; b < B; ++b) {
            float* o = out + (size_t)b * T_max * F;
            if (in_place && r.kept[b] < r.T)
                HIP_TRY(hipMemsetAsync(o + (size_t)r.kept[b] * F, 0, (size_t)(r.T - r.kept[b]) * F * sizeof(float), st));
            if (!in_place && r.kept[b] > 0)
                HIP_TRY(hipMemcpyAsync(o, (const float*)sc.feat.p + (size_t)b * r.T * F, (size_t)r.kept[b] * F * sizeof(float),
                                       hipMemcpyDeviceToDevice, st));
        }
        return 0;
    }

    HIP_TRY(hipMemsetAsync(out, 0, (size_t)B * T_max * F * sizeof(float), st));
    if (kaldi_kind(c.kind)) {
        const FbankParams f = kaldi_params(c);
        FbankOperand op{};
        HIP_TRY(fbank_operand(f, &op));
        const float* dct = nullptr;
        if (c.kind == S3ENC_SPECTRAL_MFCC) {
            DctPlan& d = g_dct[std::vector<long>{device, c.num_ceps, c.num_mel_bins, (long)std::lround(c.cepstral_lifter * 1e6)}];
            if (!d.m) HIP_TRY(to_device(&d.m, dct_lifter(c.num_ceps, c.num_mel_bins, (double)c.cepstral_lifter)));
            dct = d.m;
        }
        for (int b = 0; b < B; ++b) {
            const long T = fbank_num_frames(lengths[b], f);
            if (T <= 0) return fail("s3enc_spectral_forward: an utterance is shorter than one analysis window");
            if (T > T_max) return fail("s3enc_spectral_forward: T_max is smaller than an utterance's frame count");
            HIP_TRY(kaldi_one(c, f, op, dct, sc, wavs[b], lengths[b], T, out + (size_t)b * T_max * F, F, st));
        }
        return 0;
    }

    StftPlan& pl = g_stft[std::vector<long>{device, c.n_fft, c.win}];
    if (!pl.dft) {
        // torch.stft pads a shorter window with zeros on both sides, (n_fft - win) / 2 in front
        std::vector<double> w(c.n_fft, 0.0);
        const std::vector<double> h = hann_periodic(c.win);
        for (int i = 0; i < c.win; ++i) w[(c.n_fft - c.win) / 2 + i] = h[i];
        HIP_TRY(to_device(&pl.dft, fold_dft(w.data(), c.n_fft, c.n_fft)));
    }
    long T_longest = 0;
    for (int b = 0; b < B; ++b) {
        if (lengths[b] <= c.n_fft / 2) return fail("s3enc_spectral_forward: an utterance of n_fft / 2 samples or fewer has no reflect padding");
        T_longest = std::max(T_longest, 1 + (long)lengths[b] / c.hop);
    }
    if (T_longest > T_max) return fail("s3enc_spectral_forward: T_max is smaller than an utterance's frame count");
    if ((long)B * T_longest > 0x7fffffffL / (2 * F + 2)) return fail("s3enc_spectral_forward: batch too large");
    HIP_TRY(stft_batch(c, pl.dft, sc, wavs, lengths, B, out, T_max, st));
    return 0;
}

}  // extern "C"
