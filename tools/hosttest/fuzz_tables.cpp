// Host-side property test of the kernels' table builders (no GPU), meant to run under AddressSanitizer + UBSan:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Imfcc-rust_amd/csrc \
//       tools/hosttest/fuzz_tables.cpp mfcc-rust_amd/csrc/ss_host.cpp -o /tmp/fuzz_tables && /tmp/fuzz_tables [cases] [seed]
// For pseudo-random valid configurations (sample rate, fft_points, frame length, filter / coefficient counts, band edges, mel
// scale / norm, window) it builds the host tables and every kernel's LDS block and checks what the kernels rely on:
//   * every filter of the bank sits on exactly one (slot, lane) and the weights the lane will multiply -- its row of the mel
//     block, starting at the P bin in the start table -- are, bit for bit, the dense bank's row (zero outside);
//   * no (slot, lane) reads past the P row the kernel keeps;
//   * the cosine rows equal the host DCT table in the layout the kernel indexes (twice-folded per-lane rows of the 4096 kernel).
// Then the same number of pseudo-random valid ss_kaldi_params (M 3..80, every served frame length, bands, windows, cepstra 1..32,
// lifter) for the Kaldi front end's block: the same bank checks inside P bins 0..259, the cosine rows against kaldi_dct in
// (slot, lane) order, the appended window against kaldi_window with zeros from flen to 512, and no valid configuration rejected.
// `fuzz_tables --digest [cases] [seed]` checks nothing and prints, for a fixed list of named configurations and then the same
// pseudo-random ones, one line per kernel block: every flag and integer of its struct, the table's size and a 64-bit FNV-1a hash of
// its bytes.  Two builds of ss_host.cpp compute the same tables exactly when these outputs are equal (the hashes depend on the
// host's cos / sin, so they compare builds on one machine and are pinned nowhere).
#include "ss_internal.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

static unsigned long long g_state = 1;
static unsigned rnd()
{
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return static_cast<unsigned>(g_state >> 33);
}
static double urand() { return rnd() / 2147483648.0; }

static int g_fail = 0;
#define CHECK(cond, ...)                                  \
    do {                                                  \
        if (!(cond)) {                                    \
            if (g_fail < 20) {                            \
                std::printf("FAIL %s: ", what.c_str());   \
                std::printf(__VA_ARGS__);                 \
                std::printf("\n");                        \
            }                                             \
            ++g_fail;                                     \
        }                                                 \
    } while (0)

// mel block check shared by all kernels: start / filt tables [S][LANES], weight rows [LANES][wpitch] at melw0
static void check_mel_block(const std::string &what, const ss::HostTables &t, const std::vector<float> &tab, int k_start, int k_filt, size_t melw0, int S,
                            int LANES, const int32_t *q4, int wpitch, int prow_bins)
{
    const size_t M = t.params.num_filters, F = t.d.n_bins;
    // k_filt < 0: one packed word per (slot, lane) at k_start -- first bin | filter index << 16 (the 4096-point layout)
    std::vector<int32_t> start_v(static_cast<size_t>(S) * LANES), filt_v(static_cast<size_t>(S) * LANES);
    for (size_t q = 0; q < start_v.size(); ++q) {
        const int32_t w = reinterpret_cast<const int32_t *>(tab.data() + k_start)[q];
        start_v[q] = k_filt < 0 ? (w & 0xffff) : w;
        filt_v[q] = k_filt < 0 ? (w >> 16) : reinterpret_cast<const int32_t *>(tab.data() + k_filt)[q];
    }
    const int32_t *start = start_v.data(), *filt = filt_v.data();
    CHECK(melw0 + static_cast<size_t>(LANES) * wpitch <= tab.size(), "mel block past the table (%zu + %d x %d > %zu)", melw0, LANES, wpitch, tab.size());
    if (melw0 + static_cast<size_t>(LANES) * wpitch > tab.size()) return;
    std::vector<int> seen(M, 0);
    int off = 0;
    for (int s = 0; s < S; ++s) {
        const int span = 4 * q4[s];
        CHECK(off + span <= wpitch, "slot %d: taps %d..%d past the row pitch %d", s, off, off + span, wpitch);
        for (int j = 0; j < LANES; ++j) {
            const int st = start[s * LANES + j], m = filt[s * LANES + j];
            CHECK(st >= 0 && st + span <= prow_bins, "slot %d lane %d reads P bins %d..%d of %d", s, j, st, st + span, prow_bins);
            CHECK(m >= -1 && m < static_cast<int>(M), "slot %d lane %d: filter index %d", s, j, m);
            if (m < 0 || m >= static_cast<int>(M) || st < 0) continue;
            ++seen[m];
            const float *row = tab.data() + melw0 + static_cast<size_t>(j) * wpitch + off;
            for (size_t b = 0; b < F; ++b) {
                const float want = t.fb_dense[m * F + b];
                const long i = static_cast<long>(b) - st;
                const float got = i >= 0 && i < span ? row[i] : 0.f;
                if (std::memcmp(&want, &got, 4) != 0 && !(want == 0.f && got == 0.f)) {
                    CHECK(false, "filter %d bin %zu: table %.9g, bank %.9g (slot %d lane %d start %d)", m, b, got, want, s, j, st);
                    break;
                }
            }
        }
        off += span;
    }
    for (size_t m = 0; m < M; ++m) CHECK(seen[m] == 1, "filter %zu placed %d times", m, seen[m]);
}

static ss_params random_params()
{
    static const unsigned rates[] = {8000, 11025, 16000, 22050, 32000, 44100, 48000};
    static const unsigned ffts[] = {256, 512, 512, 1024, 2048, 2048, 4096, 4096, 400, 128, 8192};
    ss_params p;
    const unsigned sr = rates[rnd() % 7];
    ss_params_default(&p, sr);
    p.fft_points = ffts[rnd() % 11];
    const double fl = (0.25 + 0.75 * urand()) * p.fft_points / sr;
    p.frame_length = static_cast<float>(rnd() % 4 == 0 ? static_cast<double>(p.fft_points) / sr : fl);
    p.frame_stride = static_cast<float>(p.frame_length * (rnd() % 3 == 0 ? 1.0 : 0.1 + 0.6 * urand()));
    static const unsigned fcounts[] = {1, 2, 5, 13, 20, 23, 26, 32, 40, 40, 48, 64, 80, 100, 101, 128, 128, 130, 200, 252, 255, 256, 256, 300};
    p.num_filters = fcounts[rnd() % 24];
    p.num_cepstral = 1 + rnd() % (p.num_filters < 64 ? p.num_filters : 64);
    if (rnd() % 3 == 0) p.low_frequency = static_cast<float>(urand() * sr / 8);
    if (rnd() % 2 == 0) p.high_frequency = static_cast<float>(sr / 2.0 * (0.3 + 0.7 * urand()));
    p.mel_scale = rnd() % 4 == 0 ? 1 + rnd() % 2 : 0;
    p.mel_norm = p.mel_scale && rnd() % 2 ? 1 : 0;
    p.mfcc_window = rnd() % 3;
    p.spectrum_exponent = 1 + rnd() % 2;
    p.dc_elimination = rnd() % 2;
    p.framing = rnd() % 8 == 0 ? SS_FRAMING_CENTER : SS_FRAMING_CONTRACT;
    return p;
}

// ---- the Kaldi front end's block (ss_kaldi_c256): its own parameter structure, so its own draws and its own checks ----

// valid by the header's rules and served (256 < flen <= 512, M 3..80, cepstra 1..32): build_kaldi512 may reject none of these
static ss_kaldi_params random_kaldi_params()
{
    static const unsigned rates[] = {11025, 12000, 16000, 22050};
    ss_kaldi_params p;
    const unsigned sr = rates[rnd() % 4];
    ss_kaldi_params_default(&p, sr);
    static const unsigned edges[] = {257, 320, 321, 400, 416, 417, 511, 512};
    const unsigned flen = rnd() % 3 == 0 ? edges[rnd() % 8] : 257 + rnd() % 256;
    p.frame_length_ms = static_cast<float>((flen + 0.5) * 1000.0 / sr);
    p.frame_shift_ms = static_cast<float>((1 + rnd() % 600 + 0.5) * 1000.0 / sr);
    p.num_mel_bins = rnd() % 4 == 0 ? 3 + rnd() % 6 : 3 + rnd() % 78;
    p.num_ceps = 1 + rnd() % (p.num_mel_bins < 32 ? p.num_mel_bins : 32);
    p.low_freq = rnd() % 3 == 0 ? 0.0f : static_cast<float>(urand() * sr / 8);
    switch (rnd() % 3) {
    case 0: p.high_freq = 0.0f; break;
    case 1: p.high_freq = static_cast<float>(-urand() * sr / 8); break;
    default: p.high_freq = static_cast<float>(p.low_freq + 50.0 + urand() * (sr / 2.0 - p.low_freq - 50.0)); break;
    }
    p.window_type = static_cast<int32_t>(rnd() % 5);
    p.blackman_coeff = static_cast<float>(0.35 + 0.1 * urand());
    p.cepstral_lifter = rnd() % 3 == 0 ? 0.0f : static_cast<float>(1.0 + 40.0 * urand());
    p.use_power = rnd() % 2;
    return p;
}

// true: the block was built.  The bank reaches (slot, lane) bit for bit inside P bins 0 .. 259, the cosine rows are kaldi_dct in
// (slot, lane) order (zero where the pair has no filter), the appended window is kaldi_window with zeros from flen to 512.
static bool check_kaldi_block(const std::string &what, const ss_kaldi_params &p)
{
    namespace L = ss::mfcc512w_layout;
    ss::KaldiSizes s;
    const int rc = ss::kaldi_validate(p, &s);
    CHECK(rc == SS_OK, "a valid draw fails kaldi_validate with %d", rc);
    if (rc != SS_OK) return false;
    ss::KaldiTables f;
    ss::build_kaldi512(p, f);
    CHECK(f.ok, "build_kaldi512 rejects a valid configuration (pitch %d)", f.wpitch);
    if (!f.ok) return false;
    const size_t M = p.num_mel_bins, Cc = p.num_ceps, F = 257, flen = s.flen;
    CHECK(f.s.flen == s.flen && f.s.shift == s.shift && f.s.padded == 512, "sizes %u %u %u", f.s.flen, f.s.shift, f.s.padded);
    CHECK(f.wpitch > 0 && f.wpitch <= 320 && f.wpitch % 4 == 0, "weight pitch %d", f.wpitch);
    const size_t win0 = static_cast<size_t>(L::kMelW) + 16 * static_cast<size_t>(f.wpitch);
    CHECK(f.tab.size() == win0 + 512, "table of %zu floats, want %zu", f.tab.size(), win0 + 512);
    if (f.tab.size() != win0 + 512) return true;
    // the dense bank, widened to the 257 bins of a P row: the Nyquist column carries no weight
    ss::HostTables t;
    t.params.num_filters = static_cast<uint32_t>(M);
    t.d.n_bins = static_cast<uint32_t>(F);
    std::vector<float> dense(M * 256);
    ss::kaldi_mel_bank(p, s, dense.data());
    t.fb_dense.assign(M * F, 0.0f);
    for (size_t b = 0; b < M; ++b) std::copy(dense.begin() + b * 256, dense.begin() + (b + 1) * 256, t.fb_dense.begin() + b * F);
    check_mel_block(what, t, f.tab, L::kStart, L::kFilt, L::kMelW, 5, 16, f.q4, f.wpitch, 260);
    std::vector<float> dct(Cc * M);
    ss::kaldi_dct(p, dct.data());
    const int32_t *filt = reinterpret_cast<const int32_t *>(f.tab.data() + L::kFilt);
    for (size_t c = 0; c < 32; ++c)
        for (size_t q = 0; q < 80; ++q) {
            const int32_t m = filt[q];
            const float want = c < Cc && m >= 0 && m < static_cast<int32_t>(M) ? dct[c * M + m] : 0.f, got = f.tab[L::kCos + c * L::kCosPitch + q];
            CHECK(std::memcmp(&want, &got, 4) == 0 || (want == 0.f && got == 0.f), "cosine row %zu slot-lane %zu (filter %d): %.9g, kaldi_dct %.9g", c, q, m, got, want);
        }
    std::vector<float> w(flen);
    ss::kaldi_window(p, s, w.data());
    for (size_t i = 0; i < 512; ++i) {
        const float want = i < flen ? w[i] : 0.f, got = f.tab[win0 + i];
        CHECK(std::memcmp(&want, &got, 4) == 0, "window sample %zu: %.9g, kaldi_window %.9g (flen %zu)", i, got, want, flen);
    }
    return true;
}

static std::string kaldi_name(int it, const ss_kaldi_params &p)
{
    char name[256];
    std::snprintf(name, sizeof name, "kaldi case %d (sr %u flen-ms %.4f M %u C %u lo %.1f hi %.1f win %d lifter %.2f)", it, p.sample_rate, p.frame_length_ms,
                  p.num_mel_bins, p.num_ceps, p.low_freq, p.high_freq, p.window_type, p.cepstral_lifter);
    return name;
}

// ---- digest mode ----

// one line per block; a field the block's struct does not have prints as -1
struct Digest {
    int ok = -1, stft_only = -1, windowed = -1, fullp = -1, paired = -1, tight = -1, dct_fold2 = -1, cos_floats = -1, win_floats = -1;
};

template <class Tables, int NQ>
static void digest_line(const char *cfg, const char *block, const Tables &f, const int32_t (&q4)[NQ], Digest d)
{
    unsigned long long h = 1469598103934665603ull;  // FNV-1a over the raw bytes of tab
    const unsigned char *b = reinterpret_cast<const unsigned char *>(f.tab.data());
    for (size_t i = 0; i < f.tab.size() * sizeof(float); ++i) h = (h ^ b[i]) * 1099511628211ull;
    std::printf("%s | %s ok %d stft_only %d windowed %d fullp %d paired %d tight %d dct_fold2 %d cos_floats %d win_floats %d wpitch %d q4", cfg, block, f.ok,
                d.stft_only, d.windowed, d.fullp, d.paired, d.tight, d.dct_fold2, d.cos_floats, d.win_floats, f.wpitch);
    for (int s = 0; s < NQ; ++s) std::printf(" %d", q4[s]);
    std::printf(" size %zu fnv %016llx\n", f.tab.size(), h);
}

static void digest_config(const char *cfg, const ss_params &p)
{
    ss::HostTables t;
    const int rc = ss::build_tables(p, t);
    if (rc != 0) {
        std::printf("%s | rejected %d\n", cfg, rc);
        return;
    }
    Digest d;
    {
        ss::Fast512Tables f;
        ss::build_fast512(t, f);
        d = Digest{};
        d.fullp = f.fullp, d.paired = f.paired, d.tight = f.tight, d.win_floats = f.win_floats;
        digest_line(cfg, "fast512", f, f.q4, d);
    }
    {
        ss::Mfcc512wTables f;
        ss::build_mfcc512w(t, f);
        d = Digest{};
        d.windowed = f.windowed;
        digest_line(cfg, "mfcc512w", f, f.q4, d);
    }
    {
        ss::Mel512Tables f;
        ss::build_mel512(t, f);
        d = Digest{};
        d.stft_only = f.stft_only, d.fullp = f.fullp;
        digest_line(cfg, "mel512", f, f.q4, d);
    }
    {
        ss::Mfcc256Tables f;
        ss::build_mfcc256(t, f);
        d = Digest{};
        d.windowed = f.windowed;
        digest_line(cfg, "mfcc256", f, f.q4, d);
    }
    for (int mel = 0; mel < 2; ++mel) {
        ss::Mfcc1024Tables f;
        if (mel) ss::build_mel1024(t, f);
        else ss::build_mfcc1024(t, f);
        d = Digest{};
        d.stft_only = f.stft_only, d.windowed = f.windowed, d.fullp = f.fullp;
        digest_line(cfg, mel ? "mel1024" : "mfcc1024", f, f.q4, d);
    }
    {
        ss::Mfcc2048Tables f;
        ss::build_mfcc2048(t, f);
        d = Digest{};
        d.windowed = f.windowed, d.fullp = f.fullp;
        digest_line(cfg, "mfcc2048", f, f.q4, d);
    }
    {
        ss::Mel2048Tables f;
        ss::build_mel2048(t, f);
        d = Digest{};
        d.stft_only = f.stft_only, d.fullp = f.fullp;
        digest_line(cfg, "mel2048", f, f.q4, d);
    }
    for (int mel = 0; mel < 2; ++mel) {
        ss::Mfcc4096Tables f;
        if (mel) ss::build_mel4096(t, f);
        else ss::build_mfcc4096(t, f);
        d = Digest{};
        d.stft_only = f.stft_only, d.dct_fold2 = f.dct_fold2, d.cos_floats = f.cos_floats;
        digest_line(cfg, mel ? "mel4096" : "mfcc4096", f, f.q4, d);
    }
}

// The shapes the benchmark and the dedicated kernels' tests run, which random draws rarely hit.  frame_length 0 = half the
// transform (the STFT path needs fft_points >= 2 * frame_size); high_frequency 0 = fs / 2.
struct Named {
    const char *name;
    unsigned sr, fft;
    double frame_length, frame_stride;
    unsigned filters, ceps;
    double high;
    int mel_scale, window;
};
static const Named kNamed[] = {
    {"cfg2", 16000, 512, 0.02, 0.01, 40, 13, 0, 0, 0},
    {"cfg3", 16000, 2048, 0.032, 0.032, 128, 13, 8000.0, 0, 0},
    {"cfg5", 44100, 4096, 4096 / 44100.0, 1024 / 44100.0, 256, 40, 22050.0, 0, 0},
    {"cfg2 hann", 16000, 512, 0.02, 0.01, 40, 13, 0, 0, SS_WINDOW_HANN},
    {"cfg2 vorbis", 16000, 512, 0.02, 0.01, 40, 13, 0, 0, SS_WINDOW_VORBIS},
    {"cfg2 slaney to fs/2", 16000, 512, 0.02, 0.01, 40, 13, 0, SS_MEL_SLANEY, 0},
    {"cfg2 htk to fs/2", 16000, 512, 0.02, 0.01, 40, 13, 0, SS_MEL_HTK, 0},
    {"512 x 80 filters x 32", 16000, 512, 0.02, 0.01, 80, 32, 0, 0, 0},
    {"512 x 80 filters x 32 hann", 16000, 512, 0.02, 0.01, 80, 32, 0, 0, SS_WINDOW_HANN},
    {"512 stft", 16000, 512, 0, 0, 40, 13, 0, 0, 0},
    {"512 stft 80 filters", 16000, 512, 0, 0, 80, 13, 0, 0, 0},
    {"512 stft slaney to fs/2", 16000, 512, 0, 0, 64, 13, 0, SS_MEL_SLANEY, 0},
    {"512 stft 100 filters", 16000, 512, 0, 0, 100, 13, 0, 0, 0},
    {"256 at 8 kHz", 8000, 256, 0.02, 0.01, 40, 13, 0, 0, 0},
    {"256 at 8 kHz vorbis", 8000, 256, 0.02, 0.01, 32, 20, 0, 0, SS_WINDOW_VORBIS},
    {"1024 x 128", 16000, 1024, 0, 0, 128, 20, 0, 0, 0},
    {"1024 x 128 hann", 16000, 1024, 0, 0, 128, 20, 0, 0, SS_WINDOW_HANN},
    {"1024 x 128 slaney to fs/2", 16000, 1024, 0, 0, 128, 20, 0, SS_MEL_SLANEY, 0},
    {"1024 x 200 filters", 16000, 1024, 0, 0, 200, 20, 0, 0, 0},
    {"2048 x 128", 16000, 2048, 0, 0, 128, 20, 0, 0, 0},
    {"2048 x 128 vorbis", 16000, 2048, 0, 0, 128, 20, 0, 0, SS_WINDOW_VORBIS},
    {"2048 x 128 slaney to fs/2", 16000, 2048, 0, 0, 128, 20, 0, SS_MEL_SLANEY, 0},
    {"2048 x 128 htk to fs/2", 22050, 2048, 0, 0, 128, 40, 0, SS_MEL_HTK, 0},
    {"2048 x 300 filters", 16000, 2048, 0, 0, 300, 20, 0, 0, 0},
    {"4096 x 255", 44100, 4096, 0, 0, 255, 40, 0, 0, 0},
    {"4096 x 256 x 44", 44100, 4096, 0, 0, 256, 44, 0, 0, 0},
    {"4096 x 256 slaney", 44100, 4096, 0, 0, 256, 40, 11025.0, SS_MEL_SLANEY, 0},
    {"4096 x 300 filters", 44100, 4096, 0, 0, 300, 40, 0, 0, 0},
};

static int digest_main(int cases)
{
    for (const Named &n : kNamed) {
        ss_params p;
        ss_params_default(&p, n.sr);
        p.fft_points = n.fft;
        p.frame_length = static_cast<float>(n.frame_length > 0 ? n.frame_length : n.fft / 2.0 / n.sr);
        p.frame_stride = static_cast<float>(n.frame_stride > 0 ? n.frame_stride : n.fft / 2.0 / n.sr);
        p.num_filters = n.filters;
        p.num_cepstral = n.ceps;
        if (n.high > 0) p.high_frequency = static_cast<float>(n.high);
        p.mel_scale = n.mel_scale;
        p.mfcc_window = n.window;
        digest_config(n.name, p);
    }
    for (int it = 0; it < cases; ++it) {
        const ss_params p = random_params();
        char name[32];
        std::snprintf(name, sizeof name, "case %d", it);
        digest_config(name, p);
    }
    // the Kaldi front end's block: the defaults at the everyday shapes, then pseudo-random draws
    static const struct { const char *name; unsigned sr; float ms; unsigned M, C; } kKaldiNamed[] = {
        {"kaldi 16k 25ms 80", 16000, 25.0f, 80, 13}, {"kaldi 16k 25ms 23", 16000, 25.0f, 23, 13}, {"kaldi 16k 20ms 40 x 32", 16000, 20.0f, 40, 32},
        {"kaldi 16k 32ms 80", 16000, 32.0f, 80, 20}, {"kaldi 11k 25ms 40", 11025, 25.0f, 40, 13}, {"kaldi 16k 25ms 3", 16000, 25.0f, 3, 3}};
    auto kaldi_line = [](const char *name, const ss_kaldi_params &p) {
        ss::KaldiTables f;
        ss::build_kaldi512(p, f);
        digest_line(name, "kaldi512", f, f.q4, Digest{});
    };
    for (const auto &n : kKaldiNamed) {
        ss_kaldi_params p;
        ss_kaldi_params_default(&p, n.sr);
        p.frame_length_ms = n.ms;
        p.num_mel_bins = n.M;
        p.num_ceps = n.C;
        kaldi_line(n.name, p);
    }
    for (int it = 0; it < cases; ++it) {
        const ss_kaldi_params p = random_kaldi_params();
        kaldi_line(kaldi_name(it, p).c_str(), p);
    }
    return 0;
}

int main(int argc, char **argv)
{
    const bool digest = argc > 1 && std::strcmp(argv[1], "--digest") == 0;
    if (digest) --argc, ++argv;
    const int cases = argc > 1 ? std::atoi(argv[1]) : 600;
    g_state = argc > 2 ? std::strtoull(argv[2], nullptr, 10) : 12345;
    if (digest) return digest_main(cases);
    int built[10] = {0};
    int valid = 0;
    for (int it = 0; it < cases; ++it) {
        const ss_params p = random_params();
        const unsigned sr = p.sample_rate;
        ss::HostTables t;
        if (ss::build_tables(p, t) != 0) continue;  // rejected configurations (band edges, frame longer than fft_points ...) are fine
        ++valid;
        char name[256];
        std::snprintf(name, sizeof name, "case %d (sr %u fft %u flen %u step %u M %u C %u lo %.1f hi %.1f scale %d norm %d win %d)", it, sr, p.fft_points, t.d.flen,
                      t.d.step, p.num_filters, p.num_cepstral, p.low_frequency, p.high_frequency, p.mel_scale, p.mel_norm, p.mfcc_window);
        const size_t M = p.num_filters, Cc = p.num_cepstral;
        {
            ss::Fast512Tables f;
            ss::build_fast512(t, f);
            if (f.ok) {
                ++built[0];
                namespace L = ss::fast512_layout;
                check_mel_block(std::string(name) + " fast512", t, f.tab, L::kStart, L::kFilt, L::kMelW, 3, 16, f.q4, f.wpitch, f.fullp ? 260 : 132);
            }
        }
        {
            ss::Mfcc512wTables f;
            ss::build_mfcc512w(t, f);
            if (f.ok) {
                ++built[1];
                namespace L = ss::mfcc512w_layout;
                check_mel_block(std::string(name) + " mfcc512w", t, f.tab, L::kStart, L::kFilt, L::kMelW, 5, 16, f.q4, f.wpitch, 260);
            }
        }
        {
            ss::Mel512Tables f;
            ss::build_mel512(t, f);
            if (f.ok) {
                ++built[2];
                namespace L = ss::mel512_layout;
                check_mel_block(std::string(name) + " mel512", t, f.tab, L::kStart, L::kFilt, L::kMelW, 5, 16, f.q4, f.wpitch, f.fullp ? 260 : 132);
            }
        }
        {
            ss::Mfcc256Tables f;
            ss::build_mfcc256(t, f);
            if (f.ok) {
                ++built[3];
                namespace L = ss::mfcc256_layout;
                check_mel_block(std::string(name) + " mfcc256", t, f.tab, L::kStart, L::kFilt, L::kMelW, 3, 16, f.q4, f.wpitch, 132);
            }
        }
        for (int mel = 0; mel < 2; ++mel) {
            ss::Mfcc1024Tables f;
            if (mel) ss::build_mel1024(t, f);
            else ss::build_mfcc1024(t, f);
            if (f.ok) {
                ++built[4 + mel];
                namespace L = ss::mfcc1024_layout;
                check_mel_block(std::string(name) + (mel ? " mel1024" : " mfcc1024"), t, f.tab, L::kStart, L::kFilt, L::kMelW, 4, 32, f.q4, f.wpitch, f.fullp ? 516 : 260);
            }
        }
        {
            ss::Mfcc2048Tables f;
            ss::build_mfcc2048(t, f);
            if (f.ok) {
                ++built[6];
                namespace L = ss::mfcc2048_layout;
                check_mel_block(std::string(name) + " mfcc2048", t, f.tab, L::kStart, L::kFilt, L::kMelW, 4, 32, f.q4, f.wpitch, f.fullp ? 1028 : 516);
            }
        }
        {
            ss::Mel2048Tables f;
            ss::build_mel2048(t, f);
            if (f.ok) {
                ++built[7];
                namespace L = ss::mel2048_layout;
                check_mel_block(std::string(name) + " mel2048", t, f.tab, L::kStart, L::kFilt, L::kMelW, 4, 32, f.q4, f.wpitch, f.fullp ? 1028 : 516);
            }
        }
        for (int mel = 0; mel < 2; ++mel) {
            ss::Mfcc4096Tables f;
            if (mel) ss::build_mel4096(t, f);
            else ss::build_mfcc4096(t, f);
            if (!f.ok) continue;
            ++built[8 + mel];
            namespace L = ss::mfcc4096_layout;
            const std::string what = std::string(name) + (mel ? " mel4096" : " mfcc4096");
            check_mel_block(what, t, f.tab, L::kStart, -1, static_cast<size_t>(L::kCos) + f.cos_floats, 4, 64, f.q4, f.wpitch, 1028);
            if (mel) continue;
            // cosine block: what the kernel's DCT stage multiplies must be the host DCT table
            if (f.dct_fold2) {
                CHECK(M % 4 == 0 && Cc <= 43, "fold2 for M %zu C %zu", M, Cc);
                const size_t ne = (Cc + 1) / 2, no = Cc / 2, nep = (ne + 1) & ~size_t(1);
                CHECK(nep + 2 * no <= 64, "lanes: %zu + 2 x %zu", nep, no);
                std::vector<int> cover(Cc * (M / 2), 0);
                for (size_t lane = 0; lane < 64; ++lane) {
                    const float *row = f.tab.data() + L::kCos + lane * L::kCosLanePitch;
                    size_t c = 0, m0 = 0, n = 0;
                    if (lane < ne) {
                        c = 2 * lane, m0 = 0, n = M / 4;
                    } else if (lane >= nep && (lane - nep) / 2 < no) {
                        c = 2 * ((lane - nep) / 2) + 1, m0 = 64 * ((lane - nep) & 1);
                        n = M / 2 > m0 ? (M / 2 - m0 < 64 ? M / 2 - m0 : 64) : 0;
                    }
                    for (size_t i = 0; i < 64; ++i) {
                        const float want = i < n ? t.dct[c * M + m0 + i] : 0.f;
                        CHECK(std::memcmp(&want, &row[i], 4) == 0 || (want == 0.f && row[i] == 0.f), "lane %zu term %zu: %.9g, DCT table %.9g", lane, i, row[i], want);
                        if (i < n && (c & 1)) ++cover[c * (M / 2) + m0 + i];
                    }
                }
                for (size_t c = 1; c < Cc; c += 2)
                    for (size_t m = 0; m < M / 2; ++m) CHECK(cover[c * (M / 2) + m] == 1, "odd coefficient %zu term %zu covered %d times", c, m, cover[c * (M / 2) + m]);
            } else {
                for (size_t c = 0; c < Cc; ++c)
                    for (size_t m = 0; m < (M + 1) / 2; ++m) {
                        const float want = t.dct[c * M + m], got = f.tab[L::kCos + c * L::kCosPitch + m];
                        CHECK(std::memcmp(&want, &got, 4) == 0, "cos row %zu term %zu", c, m);
                    }
            }
        }
    }
    int kaldi_built = 0;  // after the others: their draws stay what they were
    for (int it = 0; it < cases; ++it) {
        const ss_kaldi_params p = random_kaldi_params();
        kaldi_built += check_kaldi_block(kaldi_name(it, p), p);
    }
    {
        const std::string what = "kaldi";
        CHECK(kaldi_built == cases, "%d of %d valid Kaldi configurations built", kaldi_built, cases);
    }
    std::printf("%d configurations, %d valid; blocks built: fast512 %d, mfcc512w %d, mel512 %d, mfcc256 %d, mfcc1024 %d, mel1024 %d, mfcc2048 %d, mel2048 %d, mfcc4096 %d, mel4096 %d; "
                "kaldi512 %d of %d\n",
                cases, valid, built[0], built[1], built[2], built[3], built[4], built[5], built[6], built[7], built[8], built[9], kaldi_built, cases);
    std::printf(g_fail ? "%d check(s) FAILED\n" : "all checks passed\n", g_fail);
    return g_fail ? 1 : 0;
}
