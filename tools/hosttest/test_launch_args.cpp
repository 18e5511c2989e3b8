// Host-side check of the argument-block builders in mfcc-rust_amd/csrc/ss_launch_args.h (no GPU): for every builder and every
// flavour of call site in ss_api.hip (dense, streaming, packed; mel from the 2048 / 1024 / 4096-point tables; stft output; the
// 256-point and the wide-bank 512-point family) the block it returns is compared byte for byte with one written out field by
// field, the way each call site filled its block by hand before the builders existed.  The table descriptions and the FrontArgs
// carry a distinct value in every field, so a swapped or dropped field shows.  dct_scales is checked against its three formulas.
// tests/test_launch_args.py builds it with AddressSanitizer + UBSan and runs it:
//   hipcc --offload-host-only -x hip -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -fno-sanitize-recover=all
//       -Iinclude -Imfcc-rust_amd/csrc tools/hosttest/test_launch_args.cpp -o /tmp/la && /tmp/la
#include "ss_launch_args.h"

#include <cstdio>
#include <cstring>

static int g_failed = 0;
#define CHECK(cond, ...)                           \
    do {                                           \
        if (!(cond)) {                             \
            if (++g_failed <= 20) {                \
                std::printf("FAILED %s: ", #cond); \
                std::printf(__VA_ARGS__);          \
                std::printf("\n");                 \
            }                                      \
        }                                          \
    } while (0)

// a distinct small value per call
static uint32_t g_next = 3;
static uint32_t nv() { return g_next += 7; }
template <typename T>
static T *np()
{
    return reinterpret_cast<T *>(static_cast<uintptr_t>(0x10000u + 64u * nv()));
}

// The comparison is a memcmp over the whole struct, padding included: `want` starts from memset zeros, the builders start from
// `T f{}` and return by value.  That the padding bytes agree rests on the compiler zeroing the whole object in that
// value-initialisation and copying it whole (clang does both); if a check fails at an offset that belongs to no field -- between
// spectrum_exponent and tab of the MFCC blocks, say -- it is this assumption that broke, not a builder.
template <typename T>
static T zeroed()
{
    T v;
    std::memset(&v, 0, sizeof v);
    return v;
}
template <typename T>
static void same(const T &got, const T &want, const char *what)
{
    const unsigned char *g = reinterpret_cast<const unsigned char *>(&got), *w = reinterpret_cast<const unsigned char *>(&want);
    size_t first = sizeof(T);
    for (size_t i = sizeof(T); i-- > 0;)
        if (g[i] != w[i]) first = i;
    CHECK(std::memcmp(&got, &want, sizeof(T)) == 0, "%s: first differing byte at offset %zu of %zu", what, first, sizeof(T));
}

// every field of a FrontArgs distinct and non-zero (the framing / output switches: what the caller asks for)
static ss::FrontArgs front(int out_kind, int frame_mode, int pad_reflect)
{
    ss::FrontArgs a = zeroed<ss::FrontArgs>();
    a.x = np<const float>();
    a.ld = 100000ull + nv();
    a.n_samples = nv();
    a.batch = nv();
    a.flen = nv();
    a.step = nv();
    a.n_frames = nv();
    a.frame_mode = frame_mode;
    a.pad_reflect = pad_reflect;
    a.preemph = 0.5f + static_cast<float>(nv());
    a.preemph_shift = nv();
    a.hop = nv();
    a.n_pad = nv();
    a.rows = nv();
    a.real_rows = nv();
    a.window = np<const float>();
    a.scale = 0.25f + static_cast<float>(nv());
    a.spectrum_exponent = static_cast<int32_t>(nv());
    a.tw_c = np<const float2>();
    a.tw_n = np<const float2>();
    a.blu_c = np<const float2>();
    a.blu_b = np<const float2>();
    a.blu_n = nv();
    a.f_start = np<const int32_t>();
    a.f_len = np<const int32_t>();
    a.f_off = np<const int32_t>();
    a.f_w = np<const float>();
    a.n_filters = nv();
    a.dct = np<const float>();
    a.n_ceps = nv();
    a.dct_scale_k = 0.125f + static_cast<float>(nv());
    a.dct_scale_0 = 0.125f + static_cast<float>(nv());
    a.dct_scale_00 = 0.125f + static_cast<float>(nv());
    a.dc_elimination = static_cast<int32_t>(nv());
    a.out_kind = out_kind;
    a.out0 = np<float>();
    a.out1 = np<float>();
    return a;
}
// what a packed / pool call leaves unset in its FrontArgs: it has no row stride and no per-clip shape
static void no_shape(ss::FrontArgs &a)
{
    a.ld = 0;
    a.n_samples = a.batch = a.n_frames = a.rows = a.real_rows = 0;
}

template <typename Tables>
static void fill_q4(Tables &t)
{
    for (int32_t &q : t.q4) q = static_cast<int32_t>(nv());
    t.wpitch = static_cast<int32_t>(nv());
}

// ---- Fast512Args ------------------------------------------------------------------------------------------------------------
static ss::Fast512Tables fast_tables(bool fullp, bool paired, bool tight)
{
    ss::Fast512Tables t;
    t.ok = true;
    fill_q4(t);
    t.fullp = fullp;
    t.paired = paired;
    t.tight = tight;
    t.win_floats = static_cast<int32_t>(nv());
    return t;
}
// launch_frames' block (dense MFCC / mfe / power)
static ss::Fast512Args fast_dense(const ss::Fast512Tables &t, const float *tab, const ss::FrontArgs &a)
{
    ss::Fast512Args f = zeroed<ss::Fast512Args>();
    f.x = a.x;
    f.ld = a.ld;
    f.n_samples = a.n_samples;
    f.batch = a.batch;
    f.flen = a.flen;
    f.step = a.step;
    f.n_frames = a.n_frames;
    f.scale = a.scale;
    f.spectrum_exponent = a.spectrum_exponent;
    f.tab = tab;
    f.mel_wpitch = t.wpitch;
    for (int s = 0; s < 3; ++s) f.mel_q4[s] = t.q4[s];
    f.n_filters = a.n_filters;
    f.n_ceps = a.n_ceps;
    f.dct_scale_k = a.dct_scale_k;
    f.dct_scale_0 = a.dct_scale_0;
    f.dct_scale_00 = a.dct_scale_00;
    f.dc_elimination = a.dc_elimination;
    f.out = a.out0;
    f.out_energy = a.out1;
    f.out_mfe = a.out_kind == ss::OUT_MFE ? 1 : (a.out_kind == ss::OUT_POWER ? 2 : 0);
    f.win_floats = a.window ? t.win_floats : 0;
    f.preemph = a.preemph;
    f.preemph_shift = a.preemph_shift;
    f.center = a.frame_mode == ss::FRAME_CENTER;
    f.pad_reflect = a.pad_reflect;
    f.fullp = t.fullp;
    f.paired = t.paired ? (t.tight ? 2 : 1) : 0;
    return f;
}
// the streaming block (dense streams and the pool): the fields the hand-written fill set
static ss::Fast512Args fast_stream(const ss::Fast512Tables &t, const float *tab, const ss::FrontArgs &a)
{
    ss::Fast512Args f = zeroed<ss::Fast512Args>();
    f.x = a.x;
    f.ld = a.ld;
    f.n_samples = a.n_samples;
    f.batch = a.batch;
    f.flen = a.flen;
    f.step = a.step;
    f.n_frames = a.n_frames;
    f.scale = a.scale;
    f.spectrum_exponent = a.spectrum_exponent;
    f.tab = tab;
    f.mel_wpitch = t.wpitch;
    for (int s = 0; s < 3; ++s) f.mel_q4[s] = t.q4[s];
    f.n_filters = a.n_filters;
    f.n_ceps = a.n_ceps;
    f.dct_scale_k = a.dct_scale_k;
    f.dct_scale_0 = a.dct_scale_0;
    f.dct_scale_00 = a.dct_scale_00;
    f.dc_elimination = a.dc_elimination;
    f.out = a.out0;
    f.out_energy = a.out1;
    f.out_mfe = a.out_kind == ss::OUT_MFE ? 1 : 0;
    f.paired = t.paired ? (t.tight ? 2 : 1) : 0;
    return f;
}
// launch_packed's block (MFCC only; no row stride, no per-clip shape, no energy output)
static ss::Fast512Args fast_packed(const ss::Fast512Tables &t, const float *tab, const ss::FrontArgs &a)
{
    ss::Fast512Args f = zeroed<ss::Fast512Args>();
    f.x = a.x;
    f.flen = a.flen;
    f.step = a.step;
    f.scale = a.scale;
    f.spectrum_exponent = a.spectrum_exponent;
    f.tab = tab;
    f.mel_wpitch = t.wpitch;
    for (int s = 0; s < 3; ++s) f.mel_q4[s] = t.q4[s];
    f.n_filters = a.n_filters;
    f.n_ceps = a.n_ceps;
    f.dct_scale_k = a.dct_scale_k;
    f.dct_scale_0 = a.dct_scale_0;
    f.dct_scale_00 = a.dct_scale_00;
    f.dc_elimination = a.dc_elimination;
    f.out = a.out0;
    f.win_floats = a.window ? t.win_floats : 0;
    f.preemph = a.preemph;
    f.preemph_shift = a.preemph_shift;
    f.center = a.frame_mode == ss::FRAME_CENTER;
    f.pad_reflect = a.pad_reflect;
    f.fullp = t.fullp;
    f.paired = t.paired ? (t.tight ? 2 : 1) : 0;
    return f;
}

static void check_fast512()
{
    const float *tab = np<const float>();
    // dense: MFCC / mfe / power, with and without window and centred frames, the three `paired` codes
    for (int out_kind : {ss::OUT_MFCC, ss::OUT_MFE, ss::OUT_POWER})
        for (int variant = 0; variant < 3; ++variant) {
            const ss::Fast512Tables t = fast_tables(variant == 2, variant >= 1, variant == 1);
            ss::FrontArgs a = front(out_kind, variant == 2 ? ss::FRAME_CENTER : ss::FRAME_NORMAL, variant == 2);
            if (variant == 0) a.window = nullptr;
            same(ss::fast512_args(t, tab, a), fast_dense(t, tab, a), "Fast512Args, dense");
        }
    // streaming, pad_mode = REFLECT: what frame_stream_fast_candidate lets through (no window, no pre-emphasis, contract frames,
    // a bank within the reference's bins).  The hand-written fill left pad_reflect and preemph_shift at zero where the builder
    // now copies them from the FrontArgs; the streaming builds of ss_mfcc_c256 read neither (a.pad_reflect: load_quad's CENTER
    // branch; a.preemph_shift: its PRE branch -- the STRM / STRP builds are !CENTER && !PRE by their static_assert).  Every other
    // byte is the hand-written block's.
    for (int out_kind : {ss::OUT_MFCC, ss::OUT_MFE}) {
        const ss::Fast512Tables t = fast_tables(false, true, true);
        ss::FrontArgs a = front(out_kind, ss::FRAME_NORMAL, 1);
        a.window = nullptr;
        a.preemph = 0.0f;
        ss::Fast512Args want = fast_stream(t, tab, a);
        CHECK(want.pad_reflect == 0 && want.preemph_shift == 0 && a.pad_reflect == 1 && a.preemph_shift != 0, "the known disagreement is exercised");
        want.pad_reflect = a.pad_reflect;
        want.preemph_shift = a.preemph_shift;
        same(ss::fast512_args(t, tab, a), want, "Fast512Args, streaming");
        no_shape(a);  // the pool: the packed chunks have no row stride and no per-stream shape
        want = fast_stream(t, tab, a);
        want.pad_reflect = a.pad_reflect;
        want.preemph_shift = a.preemph_shift;
        same(ss::fast512_args(t, tab, a), want, "Fast512Args, pool");
    }
    // packed: MFCC, out1 null
    for (int frame_mode : {ss::FRAME_NORMAL, ss::FRAME_CENTER, ss::FRAME_PADDED}) {
        const ss::Fast512Tables t = fast_tables(false, true, false);
        ss::FrontArgs a = front(ss::OUT_MFCC, frame_mode, frame_mode == ss::FRAME_CENTER);
        no_shape(a);
        a.out1 = nullptr;
        a.dct_scale_k = a.dct_scale_00 = 0.0f;  // the reference scaling: formed per clip on the device
        same(ss::fast512_args(t, tab, a), fast_packed(t, tab, a), "Fast512Args, packed");
    }
}

// ---- Mel2048Args ------------------------------------------------------------------------------------------------------------
// launch_stft's block from (tab, wpitch, q4, fullp) of the family that serves the call
static ss::Mel2048Args mel_dense(const float *tab, int32_t wpitch, const int32_t *q4, bool fullp, const ss::FrontArgs &a)
{
    ss::Mel2048Args m = zeroed<ss::Mel2048Args>();
    m.x = a.x;
    m.ld = a.ld;
    m.n_samples = a.n_samples;
    m.batch = a.batch;
    m.hop = a.hop;
    m.n_pad = a.n_pad;
    m.rows = a.rows;
    m.real_rows = a.real_rows;
    m.scale = a.scale;
    m.tab = tab;
    m.fullp = fullp;
    m.mel_wpitch = wpitch;
    for (int s = 0; s < 4; ++s) m.mel_q4[s] = q4[s];
    m.n_filters = a.n_filters;
    m.out = a.out0;
    m.out_stft = a.out_kind == ss::OUT_STFT;
    return m;
}
// the packed and pool blocks: x / out = the packed blocks, no shape, mel output only (out_stft stays 0)
static ss::Mel2048Args mel_packed(const ss::Mel2048Tables &t, const float *tab, const ss::FrontArgs &a)
{
    ss::Mel2048Args m = zeroed<ss::Mel2048Args>();
    m.x = a.x;
    m.hop = a.hop;
    m.n_pad = a.n_pad;
    m.scale = a.scale;
    m.tab = tab;
    m.fullp = t.fullp;
    m.mel_wpitch = t.wpitch;
    for (int s = 0; s < 4; ++s) m.mel_q4[s] = t.q4[s];
    m.n_filters = a.n_filters;
    m.out = a.out0;
    return m;
}

static void check_mel2048()
{
    const float *tab = np<const float>();
    for (int out_kind : {ss::OUT_MEL, ss::OUT_STFT})
        for (bool fullp : {false, true}) {
            const ss::FrontArgs a = front(out_kind, 0, 0);
            ss::Mel2048Tables t2;
            fill_q4(t2);
            t2.fullp = fullp;
            unsigned *ctl = np<unsigned>();
            unsigned long long *stamps = np<unsigned long long>();
            ss::Mel2048Args got = ss::mel2048_args(ss::mel_view(t2, tab), a);
            got.ctl = ctl;  // the caller's two lines behind the builder
            got.stamps = stamps;
            ss::Mel2048Args want = mel_dense(tab, t2.wpitch, t2.q4, t2.fullp, a);
            want.ctl = ctl;
            want.stamps = stamps;
            same(got, want, "Mel2048Args, 2048-point tables");
            ss::Mfcc1024Tables t1;
            fill_q4(t1);
            t1.fullp = fullp;
            same(ss::mel2048_args(ss::mel_view(t1, tab), a), mel_dense(tab, t1.wpitch, t1.q4, t1.fullp, a), "Mel2048Args, 1024-point tables");
            ss::Mfcc4096Tables t4;  // (no build for banks past (F+1)/2: fullp stays 0)
            fill_q4(t4);
            same(ss::mel2048_args(ss::mel_view(t4, tab), a), mel_dense(tab, t4.wpitch, t4.q4, false, a), "Mel2048Args, 4096-point tables");
        }
    // streaming (dense streams): mel output only, so out_stft = 0 as the hand-written fill left it; continuous mode: n_pad = 0
    {
        ss::FrontArgs a = front(ss::OUT_MEL, 0, 0);
        a.n_pad = 0;
        ss::Mel2048Tables t2;
        fill_q4(t2);
        ss::Mel2048Args want = mel_dense(tab, t2.wpitch, t2.q4, t2.fullp, a);
        CHECK(want.out_stft == 0, "a streaming mel block has out_stft = 0");
        same(ss::mel2048_args(ss::mel_view(t2, tab), a), want, "Mel2048Args, streaming");
    }
    // packed clips (n_pad from the configuration) and the pool (n_pad = 0)
    for (bool pool : {false, true}) {
        ss::FrontArgs a = front(ss::OUT_MEL, 0, 0);
        no_shape(a);
        if (pool) a.n_pad = 0;
        ss::Mel2048Tables t2;
        fill_q4(t2);
        same(ss::mel2048_args(ss::mel_view(t2, tab), a), mel_packed(t2, tab, a), pool ? "Mel2048Args, pool" : "Mel2048Args, packed");
    }
}

// ---- Mel512Args -------------------------------------------------------------------------------------------------------------
static void check_mel512()
{
    const float *tab = np<const float>();
    for (int out_kind : {ss::OUT_MEL, ss::OUT_STFT}) {
        const ss::FrontArgs a = front(out_kind, 0, 0);
        ss::Mel512Tables t;
        fill_q4(t);
        t.fullp = out_kind == ss::OUT_MEL;
        ss::Mel512Args m = zeroed<ss::Mel512Args>();
        m.x = a.x;
        m.ld = a.ld;
        m.n_samples = a.n_samples;
        m.batch = a.batch;
        m.hop = a.hop;
        m.n_pad = a.n_pad;
        m.rows = a.rows;
        m.real_rows = a.real_rows;
        m.scale = a.scale;
        m.tab = tab;
        m.mel_wpitch = t.wpitch;
        for (int s = 0; s < 5; ++s) m.mel_q4[s] = t.q4[s];
        m.fullp = t.fullp;
        m.n_filters = a.n_filters;
        m.out = a.out0;
        m.out_stft = a.out_kind == ss::OUT_STFT;
        same(ss::mel512_args(t, tab, a), m, "Mel512Args");
    }
}

// ---- Mfcc256Args: the wide-bank 512-point family (five slots, centred frames) and the 256-point one (three slots) -----------------
template <typename Tables, int SLOTS>
static ss::Mfcc256Args mfcc256_common(const Tables &t, const float *tab, const ss::FrontArgs &a)
{
    ss::Mfcc256Args f = zeroed<ss::Mfcc256Args>();
    f.preemph = a.preemph;
    f.preemph_shift = a.preemph_shift;
    f.x = a.x;
    f.ld = a.ld;
    f.n_samples = a.n_samples;
    f.batch = a.batch;
    f.flen = a.flen;
    f.step = a.step;
    f.n_frames = a.n_frames;
    f.scale = a.scale;
    f.spectrum_exponent = a.spectrum_exponent;
    f.tab = tab;
    f.mel_wpitch = t.wpitch;
    for (int s = 0; s < SLOTS; ++s) f.mel_q4[s] = t.q4[s];
    f.n_filters = a.n_filters;
    f.n_ceps = a.n_ceps;
    f.dct_scale_k = a.dct_scale_k;
    f.dct_scale_0 = a.dct_scale_0;
    f.dct_scale_00 = a.dct_scale_00;
    f.dc_elimination = a.dc_elimination;
    f.windowed = t.windowed;
    f.out_mfe = a.out_kind == ss::OUT_MFE;
    f.out = a.out0;
    f.out_energy = a.out1;
    return f;
}

static void check_mfcc256()
{
    const float *tab = np<const float>();
    for (int out_kind : {ss::OUT_MFCC, ss::OUT_MFE})
        for (int frame_mode : {ss::FRAME_NORMAL, ss::FRAME_CENTER})
            for (int pad_reflect : {0, 1}) {
                const ss::FrontArgs a = front(out_kind, frame_mode, pad_reflect);
                ss::Mfcc512wTables tw;
                fill_q4(tw);
                tw.windowed = out_kind == ss::OUT_MFE;
                ss::Mfcc256Args want = mfcc256_common<ss::Mfcc512wTables, 5>(tw, tab, a);
                want.center = frame_mode == ss::FRAME_CENTER;  // the wide-bank site's two extra lines
                want.pad_reflect = a.pad_reflect;
                same(ss::mfcc256_args(tw, tab, a), want, "Mfcc256Args, wide-bank 512-point family");
                if (frame_mode != ss::FRAME_NORMAL) continue;  // the 256-point rung takes contract frames only
                ss::Mfcc256Tables t;
                fill_q4(t);
                t.windowed = out_kind == ss::OUT_MFCC;
                // the 256-point site left center and pad_reflect at zero: center is zero for contract frames either way, and
                // pad_reflect now follows the FrontArgs -- ss_mfcc256.hip reads neither field (it has no centred build)
                want = mfcc256_common<ss::Mfcc256Tables, 3>(t, tab, a);
                CHECK(want.center == 0 && want.pad_reflect == 0 && want.mel_q4[3] == 0 && want.mel_q4[4] == 0, "the 256-point block's unset fields");
                want.pad_reflect = a.pad_reflect;
                same(ss::mfcc256_args(t, tab, a), want, "Mfcc256Args, 256-point family");
            }
}

// ---- Mfcc2048Args: the 2048 and the 1024-point family -----------------------------------------------------------------------------
template <typename Tables>
static void check_mfcc2048_family(const char *what)
{
    const float *tab = np<const float>();
    for (int out_kind : {ss::OUT_MFCC, ss::OUT_MFE})
        for (int frame_mode : {ss::FRAME_NORMAL, ss::FRAME_CENTER}) {
            const ss::FrontArgs a = front(out_kind, frame_mode, frame_mode == ss::FRAME_CENTER);
            Tables t;
            fill_q4(t);
            t.windowed = out_kind == ss::OUT_MFCC;
            t.fullp = frame_mode == ss::FRAME_NORMAL;
            ss::Mfcc2048Args f = zeroed<ss::Mfcc2048Args>();
            f.preemph = a.preemph;
            f.preemph_shift = a.preemph_shift;
            f.x = a.x;
            f.ld = a.ld;
            f.n_samples = a.n_samples;
            f.batch = a.batch;
            f.flen = a.flen;
            f.step = a.step;
            f.n_frames = a.n_frames;
            f.scale = a.scale;
            f.spectrum_exponent = a.spectrum_exponent;
            f.tab = tab;
            f.mel_wpitch = t.wpitch;
            for (int s = 0; s < 4; ++s) f.mel_q4[s] = t.q4[s];
            f.n_filters = a.n_filters;
            f.n_ceps = a.n_ceps;
            f.dct_scale_k = a.dct_scale_k;
            f.dct_scale_0 = a.dct_scale_0;
            f.dct_scale_00 = a.dct_scale_00;
            f.dc_elimination = a.dc_elimination;
            f.windowed = t.windowed;
            f.out_mfe = a.out_kind == ss::OUT_MFE;
            f.center = a.frame_mode == ss::FRAME_CENTER;
            f.pad_reflect = a.pad_reflect;
            f.fullp = t.fullp;
            f.out = a.out0;
            f.out_energy = a.out1;
            same(ss::mfcc2048_args(t, tab, a), f, what);
        }
}

// ---- Mfcc4096Args -----------------------------------------------------------------------------------------------------------
static void check_mfcc4096()
{
    const float *tab = np<const float>();
    for (int out_kind : {ss::OUT_MFCC, ss::OUT_MFE})
        for (bool fold2 : {false, true}) {
            ss::FrontArgs a = front(out_kind, ss::FRAME_NORMAL, 0);
            if (fold2) a.window = nullptr;
            ss::Mfcc4096Tables t;
            fill_q4(t);
            t.cos_floats = static_cast<int32_t>(nv());
            t.dct_fold2 = fold2;
            unsigned long long *stamps = np<unsigned long long>();
            ss::Mfcc4096Args f = zeroed<ss::Mfcc4096Args>();
            f.preemph = a.preemph;
            f.preemph_shift = a.preemph_shift;
            f.x = a.x;
            f.ld = a.ld;
            f.n_samples = a.n_samples;
            f.batch = a.batch;
            f.flen = a.flen;
            f.step = a.step;
            f.n_frames = a.n_frames;
            f.scale = a.scale;
            f.spectrum_exponent = a.spectrum_exponent;
            f.tab = tab;
            f.mel_wpitch = t.wpitch;
            for (int s = 0; s < 4; ++s) f.mel_q4[s] = t.q4[s];
            f.cos_floats = t.cos_floats;
            f.dct_fold2 = t.dct_fold2 ? 1 : 0;
            f.n_filters = a.n_filters;
            f.n_ceps = a.n_ceps;
            f.dct_scale_k = a.dct_scale_k;
            f.dct_scale_0 = a.dct_scale_0;
            f.dct_scale_00 = a.dct_scale_00;
            f.dc_elimination = a.dc_elimination;
            f.out = a.out0;
            f.out_energy = a.out1;
            f.out_mfe = a.out_kind == ss::OUT_MFE;
            f.window = a.window;
            f.stamps = stamps;
            ss::Mfcc4096Args got = ss::mfcc4096_args(t, tab, a);
            got.stamps = stamps;  // the caller's line behind the builder
            same(got, f, "Mfcc4096Args");
        }
}

// ---- dct_scales ---------------------------------------------------------------------------------------------------------------
static bool bits_equal(float a, float b) { return std::memcmp(&a, &b, sizeof a) == 0; }

static void check_dct_scales()
{
    for (uint32_t filters : {1u, 26u, 40u, 80u, 128u})
        for (float gain : {2.0f, 1.0f, 0.7f}) {
            ss_params p{};
            p.num_filters = filters;
            p.dct2_gain = gain;
            const float g = p.dct2_gain;
            const float M = static_cast<float>(p.num_filters);
            // ortho: scipy's scaling over the axis length, whatever the frame count
            p.dct_norm = SS_DCT_ORTHO;
            {
                const ss::DctScales s = ss::dct_scales_per_clip(p);
                CHECK(bits_equal(s.k, g * (1.0f / sqrtf(2.0f * M))) && bits_equal(s.s0, g * (1.0f / sqrtf(4.0f * M))) && bits_equal(s.s00, s.s0),
                      "ortho per clip, %u filters", filters);
            }
            for (size_t frames : {size_t(1), size_t(2), size_t(98)}) {
                const ss::DctScales s = ss::dct_scales(p, frames);
                CHECK(bits_equal(s.k, g * (1.0f / sqrtf(2.0f * M))) && bits_equal(s.s0, g * (1.0f / sqrtf(4.0f * M))) && bits_equal(s.s00, s.s0),
                      "ortho, %u filters, %zu frames", filters, frames);
            }
            // reference with T frames: n = T * M as f32 (feature.rs:126-131)
            p.dct_norm = SS_DCT_REFERENCE;
            for (size_t T : {size_t(1), size_t(2), size_t(98), size_t(100000), size_t(1) << 31}) {
                const ss::DctScales s = ss::dct_scales(p, T);
                const float nn = static_cast<float>(T * p.num_filters);
                CHECK(bits_equal(s.k, g * (1.0f / sqrtf(2.0f * nn))) && bits_equal(s.s0, g) && bits_equal(s.s00, g * (1.0f / sqrtf(4.0f * nn))),
                      "reference, %u filters, %zu frames", filters, T);
            }
            // reference with the per-clip multipliers left to the device (packed clips): only column 0's gain
            const ss::DctScales s = ss::dct_scales_per_clip(p);
            CHECK(bits_equal(s.k, 0.0f) && bits_equal(s.s0, g) && bits_equal(s.s00, 0.0f), "reference per clip, %u filters", filters);
        }
}

int main()
{
    check_fast512();
    check_mel2048();
    check_mel512();
    check_mfcc256();
    check_mfcc2048_family<ss::Mfcc2048Tables>("Mfcc2048Args, 2048-point family");
    check_mfcc2048_family<ss::Mfcc1024Tables>("Mfcc2048Args, 1024-point family");
    check_mfcc4096();
    check_dct_scales();
    if (g_failed) {
        std::printf("%d checks FAILED\n", g_failed);
        return 1;
    }
    std::printf("all checks passed\n");
    return 0;
}
