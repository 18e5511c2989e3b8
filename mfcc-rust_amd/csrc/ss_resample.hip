// Polyphase windowed-sinc resampling ahead of the feature calls: ss_resample* on dense batches, ss_resample_packed* on packed
// variable-length clips and ss_resample_stream_packed* / ss_resample_stream_flush* over a pool of stream states, float and 16-bit
// PCM input.  The definition (include/speechsauce_amd.h) is torchaudio's default filter (sinc_interp_hann) formed in f64 on the host
// and rounded once to f32, and one serial fmaf chain per output over the phase's run of taps in ascending order, samples outside the
// clip being +0.0f whose fma is executed.  So an output's bits depend on the samples under its taps and on the handle only: not on
// the tile it was computed in, the clip's place in the block, the entry's place in the call or how a stream was cut into calls.
// The reference crate has no resampler, so this file restates nothing of it.  The PCM scale rule is that of ss_api.hip, restated
// here so that the existing objects build exactly as before.
#include "ss_device.h"
#include "ss_hip_staging.h"
#include "ss_host_checks.h"
#include "ss_internal.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <numeric>
#include <string>
#include <vector>

namespace ss {

namespace {

constexpr unsigned kMaxRatio = 1024;       // o and n
constexpr unsigned kMaxTaps = 256;         // longest run of taps of a phase
constexpr size_t kMaxTableBytes = 40960;   // the compact table [n x taps] of floats: 40 KiB
constexpr unsigned kLanes = 256;           // threads of a workgroup
constexpr unsigned kChains = 4;            // outputs (fma chains) a lane runs at once
constexpr unsigned kUniPhases = 4;         // up to this n a lane walks the phases of its periods (compute_tile)
constexpr unsigned kLdsBytes = 65536;      // LDS a workgroup may ask for
constexpr unsigned kCuLdsBytes = 163840;   // ... of a CU's
constexpr unsigned kMaxTileOutputs = 8192;

// What the kernels know about a handle.  The device table is [first, count][n] (int32 pairs) followed by h [n x pitch] floats,
// pitch = taps | 1: rows zero-padded on the right, an odd pitch so that the lanes of a wave -- consecutive phases -- read their taps
// from different LDS banks.
struct Geom {
    unsigned o, n;         // orig_rate / g, new_rate / g
    unsigned width, taps, pitch;
    unsigned lookback;     // max_i(width - first[i]): samples a period's outputs reach to the left of its first sample
    unsigned lookahead;    // max_i(first[i] + count[i] - 1 - width): ... and to the right of it
    unsigned latency;      // D = ceil((lookahead + 1) / o) periods
    unsigned tile;         // J: periods (of o samples in, n outputs out) per tile
    unsigned groups;       // G = ceil(J / kChains): a lane's chains are the periods grp, grp + G, grp + 2G, ... of its phase
    unsigned tab_words;    // 2n + n * pitch
    unsigned hist;         // D * o + lookback: samples a pool row keeps
};

// ---- samples ----
__device__ __forceinline__ float sample_of(const float *p, float) { return *p; }
__device__ __forceinline__ float sample_of(const int16_t *p, float scale) { return static_cast<float>(*p) * scale; }  // exact: scale is a power of two

struct __attribute__((aligned(4))) Float4U {  // four samples at a clip's own alignment
    float v[4];
};
struct __attribute__((aligned(8))) Short4A {  // four PCM samples at an 8-byte boundary
    int16_t v[4];
};

// One tile's outputs from its staged samples.  s_x[0] is the sample `lookback` to the left of the tile's first period.  A lane runs
// the chains of periods grp + G * r, r < kChains, of one phase together: one h read per tap feeds all of them, and the chains
// overlap each other's latency (each chain is serial by definition).  Periods at or past `jt` and outputs at or past `limit` do not
// exist; a chain without an output runs on period 0's samples (staged for every phase) and is not stored.  Outputs below `warm` are
// the forced +0.0 of a stream's warm-up.
//   UNI (n <= kUniPhases: 48 k -> 16 k, 16 k -> 8 k, 8 k -> 16 k): a lane owns periods and walks their phases one after the other, so
//   the phase, its run and every tap are wave-uniform: `tab` is the table in global memory, read by the scalar unit, and the only
//   LDS traffic is one sample per fma, the lanes o floats apart.
//   otherwise: task q = (phase i, group grp), phases fastest: `tab` is the table in LDS, the lanes of a wave write consecutive
//   outputs and read h rows an odd pitch apart.
template <bool UNI>
__device__ __forceinline__ void compute_tile(const float *s_x, const unsigned *tab, const Geom &g, unsigned jt, unsigned long long limit,
                                             unsigned long long warm, float *dst)
{
    const unsigned G = g.groups, tasks = (UNI ? 1u : g.n) * G;
    const float *h_all = reinterpret_cast<const float *>(tab + 2 * g.n);
    for (unsigned q = threadIdx.x; q < tasks; q += kLanes) {
        const unsigned grp = UNI ? q : q / g.n;
        for (unsigned u = 0; u < (UNI ? g.n : 1u); ++u) {  // uniform
            const unsigned i = UNI ? u : q % g.n;
            const unsigned first = tab[2 * i], count = tab[2 * i + 1];
            const float *h = h_all + i * g.pitch;
            const float *xp[kChains];
            float acc[kChains];
            bool live[kChains];
            unsigned long long m[kChains];
#pragma unroll
            for (unsigned r = 0; r < kChains; ++r) {
                const unsigned j = grp + G * r;
                m[r] = static_cast<unsigned long long>(j) * g.n + i;
                live[r] = j < jt && m[r] < limit;
                xp[r] = s_x + (live[r] ? j * g.o : 0u) + (first + g.lookback - g.width);
                acc[r] = 0.0f;
            }
#pragma unroll 4
            for (unsigned k = 0; k < count; ++k) {
                const float hk = h[k];
#pragma unroll
                for (unsigned r = 0; r < kChains; ++r) acc[r] = fmaf(hk, xp[r][k], acc[r]);
            }
#pragma unroll
            for (unsigned r = 0; r < kChains; ++r)
                if (live[r]) dst[m[r]] = m[r] < warm ? 0.0f : acc[r];
        }
    }
}

__device__ __forceinline__ void stage_table(unsigned *s_tab, const unsigned *tab, unsigned words)
{
    for (unsigned i = threadIdx.x; i < words; i += kLanes) s_tab[i] = tab[i];
}

// ---- dense batches and packed clips ----
// Clip b owns x[so[b] .. so[b+1]) and out[oo[b] .. oo[b+1]) (dense: rows b of x and out).  Workgroup (b, y) takes the tiles y, y +
// gridDim.y, ... of clip b: the tile's input span -- J periods plus lookback on the left and lookahead on the right, zeros where
// the clip has no sample -- goes to LDS once, then every output of the tile walks its taps there.
__device__ __forceinline__ unsigned long long out_len_of(unsigned long long len, const Geom &g) { return (len * g.n + g.o - 1) / g.o; }

template <typename T, bool UNI>
__device__ __forceinline__ void resample_clip(const T *src, float *dst, unsigned len, unsigned out_len, const unsigned *tab, const Geom &g, float scale)
{
    extern __shared__ __attribute__((aligned(16))) float s_x[];
    const unsigned span_cap = ((g.tile - 1) * g.o + g.lookback + g.lookahead + 1 + 3) & ~3u;
    const unsigned *use_tab = tab;
    if (!UNI) {
        unsigned *s_tab = reinterpret_cast<unsigned *>(s_x + span_cap);
        stage_table(s_tab, tab, g.tab_words);  // the first tile's barrier publishes it
        use_tab = s_tab;
    }
    const unsigned periods = (out_len + g.n - 1) / g.n;
    const unsigned n_tiles = (periods + g.tile - 1) / g.tile;
    for (unsigned t = blockIdx.y; t < n_tiles; t += gridDim.y) {  // uniform per workgroup
        const unsigned j0 = t * g.tile, jt = min(g.tile, periods - j0);
        const long long s0 = static_cast<long long>(j0) * g.o - g.lookback;  // the clip's sample under s_x[0]
        const unsigned slen = (jt - 1) * g.o + g.lookback + g.lookahead + 1;
        if constexpr (sizeof(T) == 4) {
            for (unsigned i = 4 * threadIdx.x; i < slen; i += 4 * kLanes) {
                const long long s = s0 + i;
                if (s >= 0 && s + 3 < static_cast<long long>(len) && i + 3 < slen) {  // four floats in one load where the clip has all four
                    const Float4U v = *reinterpret_cast<const Float4U *>(src + s);
                    *reinterpret_cast<float4 *>(s_x + i) = make_float4(v.v[0], v.v[1], v.v[2], v.v[3]);
                    continue;
                }
#pragma unroll
                for (unsigned e = 0; e < 4; ++e)
                    if (i + e < slen) s_x[i + e] = (s + e >= 0 && s + e < static_cast<long long>(len)) ? sample_of(src + (s + e), scale) : 0.0f;
            }
        } else {
            // PCM: groups of four samples cut at the 8-byte boundaries of the buffer, so that a group the clip holds in full is ONE
            // aligned 8-byte load whatever the clip's own (2-byte) alignment; `a` samples of group 0 lie in front of s_x[0]
            const unsigned a = static_cast<unsigned>((reinterpret_cast<uintptr_t>(src) + static_cast<uintptr_t>(2 * s0)) >> 1) & 3u;
            const unsigned n_groups = (slen + a + 3) / 4;
            for (unsigned q = threadIdx.x; q < n_groups; q += kLanes) {
                const long long i0 = 4ll * q - a, s = s0 + i0;
                if (i0 >= 0 && i0 + 3 < static_cast<long long>(slen) && s >= 0 && s + 3 < static_cast<long long>(len)) {
                    const Short4A v = *reinterpret_cast<const Short4A *>(src + s);
#pragma unroll
                    for (unsigned e = 0; e < 4; ++e) s_x[i0 + e] = static_cast<float>(v.v[e]) * scale;
                    continue;
                }
#pragma unroll
                for (unsigned e = 0; e < 4; ++e)
                    if (i0 + e >= 0 && i0 + e < static_cast<long long>(slen))
                        s_x[i0 + e] = (s + e >= 0 && s + e < static_cast<long long>(len)) ? sample_of(src + (s + e), scale) : 0.0f;
            }
        }
        __syncthreads();
        const unsigned long long m0 = static_cast<unsigned long long>(j0) * g.n;
        compute_tile<UNI>(s_x, use_tab, g, jt, out_len - m0, 0, dst + m0);
        __syncthreads();  // the next tile overwrites the staged samples
    }
}

template <typename T, bool PACKED, bool UNI>
__global__ __launch_bounds__(kLanes) void ss_resample_kernel(const T *__restrict__ x, const long long *__restrict__ so, const long long *__restrict__ oo,
                                                             float *__restrict__ out, const unsigned *__restrict__ tab, const Geom g,
                                                             unsigned long long total_in, unsigned long long total_out, unsigned n_samples,
                                                             unsigned long long ld, unsigned long long ld_out, float scale)
{
    if (PACKED) {
        const long long lo = so[blockIdx.x], hi = so[blockIdx.x + 1], olo = oo[blockIdx.x], ohi = oo[blockIdx.x + 1];
        if (!(lo >= 0 && lo <= hi && static_cast<unsigned long long>(hi) <= total_in && hi - lo < (1ll << 31))) return;
        const unsigned long long ol = out_len_of(static_cast<unsigned long long>(hi - lo), g);
        if (!(olo >= 0 && ohi >= olo && static_cast<unsigned long long>(ohi) <= total_out && static_cast<unsigned long long>(ohi - olo) == ol &&
              ol < (1ull << 31)))
            return;
        if (ol == 0) return;
        resample_clip<T, UNI>(x + lo, out + olo, static_cast<unsigned>(hi - lo), static_cast<unsigned>(ol), tab, g, scale);
    } else {
        resample_clip<T, UNI>(x + blockIdx.x * ld, out + blockIdx.x * ld_out, n_samples, static_cast<unsigned>(out_len_of(n_samples, g)), tab, g, scale);
    }
}

// ---- pool of stream states ----
// Entry i owns x[so[i] .. so[i+1]), P = (so[i+1] - so[i]) / o whole periods, out[so[i] / o * n .. so[i+1] / o * n) and pool row
// slots[i]: hist = D * o + lookback floats, the stream's last samples (oldest first, right-aligned, zeros in front) and, in the last
// float, min(periods seen, D).  The row followed by the entry's samples is one clip whose sample 0 sits at index `lookback`: output
// k of the entry is the clip's output k, whose taps end at or before the entry's last sample because D * o > lookahead.  The
// zeros in front of a young stream's samples are the clip's zero padding; only the first (D - count) * n outputs, which lie before
// the stream's output 0, are forced to +0.0.  The flush build brings D periods of zeros.
template <typename T, bool FLUSH, bool UNI>
__global__ __launch_bounds__(kLanes) void ss_resample_stream_kernel(const T *__restrict__ x, const long long *__restrict__ so, const int *__restrict__ slots,
                                                                    float *__restrict__ out, float *pool, const unsigned *__restrict__ tab, const Geom g,
                                                                    unsigned long long total_in, unsigned pool_streams, float scale)
{
    extern __shared__ __attribute__((aligned(16))) float s_x[];
    const unsigned D = g.latency, H = g.hist;
    const int slot = slots[blockIdx.x];
    if (slot < 0 || static_cast<unsigned>(slot) >= pool_streams) return;
    unsigned long long first_period = 0;
    unsigned P = D;
    const T *src = x;
    if (FLUSH) {
        first_period = static_cast<unsigned long long>(blockIdx.x) * D;
    } else {
        const long long lo = so[blockIdx.x], hi = so[blockIdx.x + 1];
        if (!(lo >= 0 && lo < hi && static_cast<unsigned long long>(hi) <= total_in)) return;  // (an empty entry leaves its pool row as it is)
        if (lo % g.o != 0 || hi % g.o != 0 || (hi - lo) / g.o >= (1ll << 20)) return;          // whole periods only
        first_period = static_cast<unsigned long long>(lo) / g.o;
        P = static_cast<unsigned>((hi - lo) / g.o);
        src = x + lo;
    }
    float *state = pool + static_cast<size_t>(slot) * (H + 1);
    const float cw = state[H];
    const unsigned count = (cw >= 0.0f && cw <= static_cast<float>(D) && cw == floorf(cw)) ? static_cast<unsigned>(cw) : 0u;
    const unsigned long long n_in = static_cast<unsigned long long>(P) * g.o, n_out = static_cast<unsigned long long>(P) * g.n;
    const unsigned long long warm = static_cast<unsigned long long>(D - count) * g.n;
    float *dst = out + first_period * g.n;

    const unsigned span_cap = ((g.tile - 1) * g.o + g.lookback + g.lookahead + 1 + 3) & ~3u;
    const unsigned *use_tab = tab;
    if (!UNI) {
        unsigned *s_tab = reinterpret_cast<unsigned *>(s_x + span_cap);
        stage_table(s_tab, tab, g.tab_words);
        use_tab = s_tab;
    }
    // sample v of the row-plus-entry clip, v counted from the row's first float
    auto sample = [&](unsigned long long v) -> float {
        if (v < H) return state[v];
        if (FLUSH || v - H >= n_in) return 0.0f;
        return sample_of(src + (v - H), scale);
    };
    const unsigned n_tiles = (P + g.tile - 1) / g.tile;
    for (unsigned t = 0; t < n_tiles; ++t) {
        const unsigned j0 = t * g.tile, jt = min(g.tile, P - j0);
        const unsigned long long v0 = static_cast<unsigned long long>(j0) * g.o;  // s_x[0]: clip sample j0 * o - lookback, index j0 * o of the row
        const unsigned slen = (jt - 1) * g.o + g.lookback + g.lookahead + 1;
        for (unsigned i = threadIdx.x; i < slen; i += kLanes) s_x[i] = sample(v0 + i);
        __syncthreads();
        const unsigned long long m0 = static_cast<unsigned long long>(j0) * g.n;
        compute_tile<UNI>(s_x, use_tab, g, jt, n_out - m0, warm > m0 ? warm - m0 : 0, dst + m0);
        __syncthreads();  // the next tile overwrites the staged samples; after the last one nobody reads the pool row's old contents
    }
    if (FLUSH) {
        for (unsigned i = threadIdx.x; i <= H; i += kLanes) state[i] = 0.0f;
    } else {
        // The new row is samples n_in .. n_in + H of the clip: a kept sample moves towards the front of the row it is read from, so
        // the row is rewritten in ascending steps of kLanes floats, every step read in full before it is written: a later step reads
        // only what lies behind everything written so far.
        for (unsigned base = 0; base < H; base += kLanes) {
            const unsigned at = base + threadIdx.x;
            const float v = at < H ? sample(n_in + at) : 0.0f;
            __syncthreads();
            if (at < H) state[at] = v;
        }
        if (threadIdx.x == 0) state[H] = static_cast<float>(min(count + P, D));
    }
}

// ---- host side ----

// a power of two in [2^-64, 2^64]: the product with an int16 is exact (and never subnormal)
int check_pcm_scale(float scale)
{
    int e = 0;
    const bool ok = std::isfinite(scale) && scale > 0.0f && std::frexp(scale, &e) == 0.5f && e - 1 >= -64 && e - 1 <= 64;
    return ok ? SS_OK : fail(SS_ERR_ARG, "scale must be a power of two in [2^-64, 2^64]");
}

// The C ABI carries rolloff as a float; the filter is formed in f64 from the decimal the caller wrote: the double nearest to the
// float's seven-significant-digit decimal (0.99f -> 0.99), so that the table is torchaudio's for rolloff = 0.99.
double rolloff_f64(float rolloff)
{
    char buf[40];
    std::snprintf(buf, sizeof buf, "%.7g", static_cast<double>(rolloff));
    return std::strtod(buf, nullptr);
}

struct Filter {
    Geom g{};
    std::vector<float> h;             // [n x taps], rows zero-padded on the right
    std::vector<int32_t> first, count;
};

// The specification of include/speechsauce_amd.h, in f64, rounded once.  `table`: also fill h / first / count (sizes alone need
// only the runs).
int build_filter(uint32_t orig_rate, uint32_t new_rate, uint32_t lpw, float rolloff_f, bool table, Filter &f)
{
    if (orig_rate == 0 || new_rate == 0) return fail(SS_ERR_ARG, "a sample rate of 0");
    if (orig_rate == new_rate) return fail(SS_ERR_ARG, "orig_rate == new_rate: nothing to resample");
    if (lpw < 1 || lpw > 64) return fail(SS_ERR_ARG, "lowpass_filter_width must be in 1 .. 64");
    if (!(rolloff_f > 0.0f && rolloff_f <= 1.0f)) return fail(SS_ERR_ARG, "rolloff must be in (0, 1]");
    const uint32_t gc = std::gcd(orig_rate, new_rate);
    const uint32_t o = orig_rate / gc, n = new_rate / gc;
    if (o > kMaxRatio || n > kMaxRatio)
        return fail(SS_ERR_ARG, "orig_rate / gcd and new_rate / gcd must be at most 1024 (" + std::to_string(o) + " / " + std::to_string(n) + ")");
    const double rolloff = rolloff_f64(rolloff_f);
    const double base = static_cast<double>(std::min(o, n)) * rolloff;
    const double w = std::ceil(static_cast<double>(lpw) * o / base);
    if (!(w <= 4.0 * kMaxTaps)) return fail(SS_ERR_UNSUPPORTED, "more than 256 taps per output");  // (a run is about 2 * width taps)
    const int width = static_cast<int>(w);
    const int K = 2 * width + static_cast<int>(o);
    const double PI = 3.14159265358979323846;
    auto tap_time = [&](uint32_t i, int k) { return (-static_cast<double>(i) / n + static_cast<double>(k - width) / o) * base; };
    f.first.assign(n, 0);
    f.count.assign(n, 0);
    int taps = 0, lookback = 0, lookahead = 0;
    for (uint32_t i = 0; i < n; ++i) {
        int first = -1, count = 0;
        for (int k = 0; k < K; ++k)
            if (std::fabs(tap_time(i, k)) < static_cast<double>(lpw)) {
                if (first < 0) first = k;
                ++count;
            }
        if (first < 0) first = 0;  // (cannot happen: the tap at time -i / n * base lies inside)
        f.first[i] = first;
        f.count[i] = count;
        taps = std::max(taps, count);
        lookback = std::max(lookback, width - first);
        lookahead = std::max(lookahead, first + count - 1 - width);
    }
    if (taps > static_cast<int>(kMaxTaps)) return fail(SS_ERR_UNSUPPORTED, "more than 256 taps per output (" + std::to_string(taps) + ")");
    if (static_cast<size_t>(n) * taps * sizeof(float) > kMaxTableBytes)
        return fail(SS_ERR_UNSUPPORTED, "the filter table of " + std::to_string(static_cast<size_t>(n) * taps * sizeof(float)) + " bytes exceeds 40960");
    Geom &g = f.g;
    g.o = o;
    g.n = n;
    g.width = static_cast<unsigned>(width);
    g.taps = static_cast<unsigned>(taps);
    g.pitch = g.taps | 1u;
    g.lookback = static_cast<unsigned>(std::max(lookback, 0));
    g.lookahead = static_cast<unsigned>(std::max(lookahead, 0));
    g.latency = (g.lookahead + 1 + o - 1) / o;
    g.tab_words = 2 * n + n * g.pitch;
    g.hist = g.latency * o + g.lookback;
    // The tile: J periods, scored by the lanes it keeps busy, the share of its staged span that is not halo and the share of a CU's 32
    // waves its LDS (the table, where the lanes own phases, and the span) leaves resident: measured, residency buys more than full
    // lanes (44.1 -> 16 kHz runs faster on tiles of 4 periods at 5 workgroups per CU than on 12 periods at 3).  J == 1 always fits:
    // its span is at most lookback + lookahead + 1 floats.
    const bool uni = n <= kUniPhases;
    const unsigned tab_bytes = uni ? 0u : g.tab_words * 4u;
    double best = -1.0;
    g.tile = 0;
    for (unsigned J = 1; J == 1 || static_cast<unsigned long long>(J) * n <= kMaxTileOutputs; ++J) {
        const unsigned long long span = static_cast<unsigned long long>(J - 1) * o + g.lookback + g.lookahead + 1;
        const unsigned long long lds = tab_bytes + 4ull * ((span + 3) & ~3ull);
        if (lds > kLdsBytes) break;
        const unsigned G = (J + kChains - 1) / kChains;
        const unsigned long long tasks = static_cast<unsigned long long>(uni ? 1u : n) * G, slots = (tasks + kLanes - 1) / kLanes * kLanes * kChains;
        const double busy = static_cast<double>(J) * (uni ? 1u : n) / static_cast<double>(slots);
        const double body = std::min(1.0, static_cast<double>(J) * o / static_cast<double>(span));
        const double waves = std::min(1.0, 4.0 * static_cast<double>(kCuLdsBytes / lds) / 32.0);
        const double score = busy * body * waves;
        if (score >= best) {
            best = score;
            g.tile = J;
        }
    }
    if (!g.tile) return fail(SS_ERR_UNSUPPORTED, "the filter table and one period's samples do not fit the LDS");  // (not reachable inside the limits above)
    g.groups = (g.tile + kChains - 1) / kChains;
    if (!table) return SS_OK;
    f.h.assign(static_cast<size_t>(n) * taps, 0.0f);
    for (uint32_t i = 0; i < n; ++i)
        for (int c = 0; c < f.count[i]; ++c) {
            const double t = tap_time(i, f.first[i] + c);
            const double sinc = t == 0.0 ? 1.0 : std::sin(PI * t) / (PI * t);
            const double win = std::cos(PI * t / (2.0 * lpw));
            f.h[static_cast<size_t>(i) * taps + c] = static_cast<float>(sinc * (win * win) * (base / o));
        }
    return SS_OK;
}

void fill_info(const Geom &g, ss_resample_info *info)
{
    info->o = g.o;
    info->n = g.n;
    info->width = g.width;
    info->taps = g.taps;
    info->lookback = g.lookback;
    info->lookahead = g.lookahead;
    info->latency_periods = g.latency;
    info->tile_outputs = g.tile * g.n;
}

}  // namespace

}  // namespace ss

// The handle: the filter, and its device copy (made by the first device call, on the device that is current then).
struct ss_resampler {
    ss::Filter f;
    std::vector<uint32_t> tab;  // the device table's words: [first, count][n], h [n x pitch]
    std::mutex mu;
    unsigned *d_tab = nullptr;
    int device = -1;
};

namespace ss {

namespace {

int device_table(const ss_resampler *rs_c, const unsigned **d_tab)
{
    ss_resampler *rs = const_cast<ss_resampler *>(rs_c);  // the lazy upload is the handle's one mutable part
    std::lock_guard<std::mutex> lock(rs->mu);
    int dev = -1;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return no_device();
    if (!rs->d_tab) {
        void *p = nullptr;
        e = hipMalloc(&p, rs->tab.size() * sizeof(uint32_t));
        if (e == hipSuccess) e = hipMemcpy(p, rs->tab.data(), rs->tab.size() * sizeof(uint32_t), hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            if (p) (void)hipFree(p);
            return hip_fail(e, "resampler table upload");
        }
        rs->d_tab = static_cast<unsigned *>(p);
        rs->device = dev;
    } else if (dev != rs->device) {
        return fail(SS_ERR_ARG, "the resampler's table lives on device " + std::to_string(rs->device) + ", the current device is " + std::to_string(dev));
    }
    *d_tab = rs->d_tab;
    return SS_OK;
}

unsigned lds_bytes(const Geom &g)
{
    const unsigned span_cap = ((g.tile - 1) * g.o + g.lookback + g.lookahead + 1 + 3) & ~3u;
    return 4u * (span_cap + (g.n <= kUniPhases ? 0u : g.tab_words));
}

template <typename T>
constexpr const char *kernel_name(bool packed)
{
    return sizeof(T) == 4 ? (packed ? "ss_resample_kernel<packed,f32>" : "ss_resample_kernel<dense,f32>")
                          : (packed ? "ss_resample_kernel<packed,i16>" : "ss_resample_kernel<dense,i16>");
}

template <typename T, bool PACKED>
int launch_clips(const ss_resampler *rs, const T *d_x, size_t n_clips, const int64_t *d_so, const int64_t *d_oo, size_t total_in, size_t total_out,
                 size_t n_samples, size_t ld, size_t ld_out, float scale, float *d_out, void *stream)
{
    const unsigned *d_tab = nullptr;
    const int rc = device_table(rs, &d_tab);
    if (rc) return rc;
    const Geom &g = rs->f.g;
    const unsigned long long longest_out = PACKED ? total_out : (static_cast<unsigned long long>(n_samples) * g.n + g.o - 1) / g.o;
    const unsigned long long tile_out = static_cast<unsigned long long>(g.tile) * g.n;
    const dim3 grid(static_cast<unsigned>(n_clips), packed_split(n_clips, (longest_out + tile_out - 1) / tile_out));
    auto kernel = g.n <= kUniPhases ? ss_resample_kernel<T, PACKED, true> : ss_resample_kernel<T, PACKED, false>;
    hipLaunchKernelGGL(kernel, grid, dim3(kLanes), lds_bytes(g), static_cast<hipStream_t>(stream), d_x, reinterpret_cast<const long long *>(d_so),
                       reinterpret_cast<const long long *>(d_oo), d_out, d_tab, g, static_cast<unsigned long long>(total_in),
                       static_cast<unsigned long long>(total_out), static_cast<unsigned>(n_samples), static_cast<unsigned long long>(ld),
                       static_cast<unsigned long long>(ld_out), scale);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "ss_resample_kernel");
    note_kernel(kernel_name<T>(PACKED));
    return SS_OK;
}

template <typename T>
int pcm_rule(const T *, float) { return SS_OK; }
template <>
int pcm_rule<int16_t>(const int16_t *x, float scale)
{
    if (reinterpret_cast<uintptr_t>(x) & 1u) return fail(SS_ERR_ARG, "the PCM buffer must be 2-byte aligned");
    return check_pcm_scale(scale);
}

// ---- dense ----
template <typename T>
int check_dense(const ss_resampler *rs, const T *x, size_t batch, size_t n_samples, size_t ld, float scale, const float *out, size_t ld_out, size_t &out_len)
{
    if (!rs) return fail(SS_ERR_ARG, "null resampler");
    if (!x || !out) return fail(SS_ERR_ARG, "null buffer");
    const int rc = pcm_rule(x, scale);
    if (rc) return rc;
    if (batch >= (1ull << 31) || n_samples >= (1ull << 31)) return fail(SS_ERR_ARG, "batch and n_samples must be below 2^31");
    const Geom &g = rs->f.g;
    out_len = (n_samples * g.n + g.o - 1) / g.o;
    if (out_len >= (1ull << 31)) return fail(SS_ERR_ARG, "a clip's output must be shorter than 2^31 samples");
    if (ld < n_samples) return fail(SS_ERR_ARG, "ld < n_samples");
    if (ld_out < out_len) return fail(SS_ERR_ARG, "ld_out < ss_resample_len(n_samples)");
    // what the call touches: the last row ends n_samples (out_len) behind its start, not a whole stride -- a block of (batch - 1) *
    // ld + n_samples floats is a whole batch, and what the allocator put behind it is not part of it
    const size_t x_span = batch ? (batch - 1) * ld + n_samples : 0, out_span = batch ? (batch - 1) * ld_out + out_len : 0;
    if (ranges_overlap(x, x_span * sizeof(T), out, out_span * sizeof(float))) return fail(SS_ERR_ARG, "out overlaps x: the call is not in place");
    return SS_OK;
}

template <typename T>
int dense_device(const ss_resampler *rs, const T *d_x, size_t batch, size_t n_samples, size_t ld, float scale, float *d_out, size_t ld_out, void *stream)
{
    if (batch == 0) return SS_OK;
    size_t out_len = 0;
    const int rc = check_dense(rs, d_x, batch, n_samples, ld, scale, d_out, ld_out, out_len);
    if (rc) return rc;
    if (out_len == 0) return SS_OK;
    return launch_clips<T, false>(rs, d_x, batch, nullptr, nullptr, 0, 0, n_samples, ld, ld_out, scale, d_out, stream);
}

// host-pointer form (synchronous): the rows go up compact, the output rows come down to the caller's ld_out
template <typename T>
int dense_host(const ss_resampler *rs, const T *x, size_t batch, size_t n_samples, size_t ld, float scale, float *out, size_t ld_out)
{
    if (batch == 0) return SS_OK;
    size_t out_len = 0;
    int rc = check_dense(rs, x, batch, n_samples, ld, scale, out, ld_out, out_len);
    if (rc) return rc;
    if (out_len == 0) return SS_OK;
    if (!have_device()) return no_device();
    HostStage st("ss_resample");
    T *d_in = st.room<T>(batch * n_samples * sizeof(T));
    float *d_out = st.room<float>(batch * out_len * sizeof(float));
    st.up_rows(d_in, x, ld * sizeof(T), n_samples * sizeof(T), batch);
    if (st.ok()) st.ran(dense_device<T>(rs, d_in, batch, n_samples, n_samples, scale, d_out, out_len, nullptr));
    st.sync();
    st.down_rows(out, ld_out * sizeof(float), d_out, out_len * sizeof(float), batch);
    return st.status();
}

// ---- packed ----
template <typename T>
int check_packed(const ss_resampler *rs, const T *x, const void *so, const void *oo, size_t n_clips, size_t total_in, size_t total_out, float scale,
                 const float *out)
{
    if (!rs) return fail(SS_ERR_ARG, "null resampler");
    if (!x || !so || !oo || !out) return fail(SS_ERR_ARG, "null buffer");
    const int rc = pcm_rule(x, scale);
    if (rc) return rc;
    if (n_clips >= (1ull << 31)) return fail(SS_ERR_ARG, "n_clips must be below 2^31");
    if (total_in >= (1ull << 62) || total_out >= (1ull << 62)) return fail(SS_ERR_ARG, "block too large");
    if (ranges_overlap(x, total_in * sizeof(T), out, total_out * sizeof(float))) return fail(SS_ERR_ARG, "out overlaps x: the call is not in place");
    return SS_OK;
}

template <typename T>
int packed_device(const ss_resampler *rs, const T *d_x, size_t n_clips, const int64_t *d_so, float scale, const int64_t *d_oo, size_t total_in,
                  size_t total_out, float *d_out, void *stream)
{
    if (n_clips == 0) return SS_OK;
    const int rc = check_packed(rs, d_x, d_so, d_oo, n_clips, total_in, total_out, scale, d_out);
    if (rc) return rc;
    if (total_out == 0) return SS_OK;  // no clip can own an output
    return launch_clips<T, true>(rs, d_x, n_clips, d_so, d_oo, total_in, total_out, 0, 0, 0, scale, d_out, stream);
}

// the two tables of a host-pointer call, checked before the device is touched
int check_clip_tables(const Geom &g, const int64_t *so, const int64_t *oo, size_t n_clips)
{
    if (so[0] != 0) return fail(SS_ERR_ARG, "sample_offsets[0] must be 0 (clip 0)");
    if (oo[0] != 0) return fail(SS_ERR_ARG, "out_offsets[0] must be 0 (clip 0)");
    for (size_t b = 0; b < n_clips; ++b) {
        if (so[b + 1] < so[b]) return fail(SS_ERR_ARG, "decreasing sample offsets at clip " + std::to_string(b));
        const uint64_t len = static_cast<uint64_t>(so[b + 1] - so[b]);
        if (len >= (1ull << 31)) return fail(SS_ERR_ARG, "clip " + std::to_string(b) + " is longer than 2^31 - 1 samples");
        const uint64_t want = (len * g.n + g.o - 1) / g.o;
        if (want >= (1ull << 31)) return fail(SS_ERR_ARG, "clip " + std::to_string(b) + ": its output is longer than 2^31 - 1 samples");
        if (oo[b + 1] < oo[b] || static_cast<uint64_t>(oo[b + 1] - oo[b]) != want)
            return fail(SS_ERR_ARG, "clip " + std::to_string(b) + ": its output span holds " + std::to_string(oo[b + 1] - oo[b]) + " samples, not the " +
                                        std::to_string(want) + " of ss_resample_len");
    }
    return SS_OK;
}

template <typename T>
int packed_host(const ss_resampler *rs, const T *x, size_t n_clips, const int64_t *so, float scale, const int64_t *oo, float *out)
{
    if (n_clips == 0) return SS_OK;
    int rc = check_packed(rs, x, so, oo, n_clips, 0, 0, scale, out);
    if (rc || (rc = check_clip_tables(rs->f.g, so, oo, n_clips))) return rc;
    const size_t total_in = static_cast<size_t>(so[n_clips]), total_out = static_cast<size_t>(oo[n_clips]);
    if (ranges_overlap(x, total_in * sizeof(T), out, total_out * sizeof(float))) return fail(SS_ERR_ARG, "out overlaps x: the call is not in place");
    if (total_out == 0) return SS_OK;
    if (!have_device()) return no_device();
    const size_t tbytes = (n_clips + 1) * sizeof(int64_t);
    HostStage st("ss_resample_packed");
    const T *d_in = st.up(x, total_in * sizeof(T));
    float *d_out = st.room<float>(total_out * sizeof(float));
    const int64_t *d_so = st.up(so, tbytes), *d_oo = st.up(oo, tbytes);
    if (st.ok()) st.ran(packed_device<T>(rs, d_in, n_clips, d_so, scale, d_oo, total_in, total_out, d_out, nullptr));
    st.sync();
    st.down(out, d_out, total_out * sizeof(float));
    return st.status();
}

// ---- pool ----
// what the pool calls reject before the device is touched (the tables apart).  The flush has no x and no offsets; its outputs are
// n_active * D * n.
template <typename T>
int check_stream(bool flush, const ss_resampler *rs, const T *x, const void *so, const void *slots, size_t n_active, size_t total_in, size_t pool_streams,
                 float scale, const float *pool, const float *out)
{
    if (!rs) return fail(SS_ERR_ARG, "null resampler");
    if ((!flush && (!x || !so)) || !slots || !pool || !out) return fail(SS_ERR_ARG, "null buffer");
    if (!flush) {
        const int rc = pcm_rule(x, scale);
        if (rc) return rc;
    }
    if (n_active >= (1ull << 31) || pool_streams >= (1ull << 31) || total_in >= (1ull << 40))
        return fail(SS_ERR_ARG, "n_active and pool_streams must be below 2^31, total_in below 2^40");
    if (pool_streams == 0) return fail(SS_ERR_ARG, "the pool has no rows");
    const Geom &g = rs->f.g;
    const size_t in_bytes = flush ? 0 : total_in * sizeof(T);
    const size_t out_bytes = (flush ? n_active * g.latency * g.n : total_in / g.o * g.n) * sizeof(float);
    const size_t pbytes = pool_streams * (static_cast<size_t>(g.hist) + 1) * sizeof(float);
    if (!flush && ranges_overlap(x, in_bytes, out, out_bytes)) return fail(SS_ERR_ARG, "out overlaps x: the call is not in place");
    if ((!flush && ranges_overlap(pool, pbytes, x, in_bytes)) || ranges_overlap(pool, pbytes, out, out_bytes)) return fail(SS_ERR_ARG, "the pool overlaps x or out");
    return SS_OK;
}

template <typename T, bool FLUSH>
int stream_launch(const ss_resampler *rs, const T *d_x, size_t n_active, const int64_t *d_so, size_t total_in, const int32_t *d_slots, size_t pool_streams,
                  float scale, float *d_pool, float *d_out, void *stream)
{
    const unsigned *d_tab = nullptr;
    const int rc = device_table(rs, &d_tab);
    if (rc) return rc;
    const Geom &g = rs->f.g;
    // one launch, one workgroup per entry: the grid depends on n_active only
    auto kernel = g.n <= kUniPhases ? ss_resample_stream_kernel<T, FLUSH, true> : ss_resample_stream_kernel<T, FLUSH, false>;
    hipLaunchKernelGGL(kernel, dim3(static_cast<unsigned>(n_active)), dim3(kLanes), lds_bytes(g), static_cast<hipStream_t>(stream), d_x,
                       reinterpret_cast<const long long *>(d_so), reinterpret_cast<const int *>(d_slots), d_out, d_pool, d_tab, g,
                       static_cast<unsigned long long>(total_in), static_cast<unsigned>(pool_streams), scale);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "ss_resample_stream_kernel");
    note_kernel(FLUSH ? "ss_resample_stream_kernel<flush>" : sizeof(T) == 4 ? "ss_resample_stream_kernel<f32>" : "ss_resample_stream_kernel<i16>");
    return SS_OK;
}

template <typename T>
int stream_device(const ss_resampler *rs, const T *d_x, size_t n_active, const int64_t *d_so, size_t total_in, const int32_t *d_slots, size_t pool_streams,
                  float scale, float *d_pool, float *d_out, void *stream)
{
    if (n_active == 0) return SS_OK;
    const int rc = check_stream(false, rs, d_x, d_so, d_slots, n_active, total_in, pool_streams, scale, d_pool, d_out);
    if (rc) return rc;
    if (total_in == 0) return SS_OK;  // no entry can own a sample
    return stream_launch<T, false>(rs, d_x, n_active, d_so, total_in, d_slots, pool_streams, scale, d_pool, d_out, stream);
}

// Host staging of both pool calls: x (none for the flush) and the offsets go up with the n_active named pool rows, gathered into a
// compact block whose row i is entry i's (the device call runs on slots 0 .. n_active - 1); the outputs and the pool rows come down.
// The caller's pool is written only once everything before it succeeded.
template <typename T>
int stream_via_device(bool flush, const ss_resampler *rs, const T *x, size_t n_active, const int64_t *so, const int32_t *slots, size_t n_in, size_t n_out,
                      float scale, float *pool, float *out)
{
    if (!have_device()) return no_device();
    PoolRows named;
    named.gather(pool, slots, n_active, static_cast<size_t>(rs->f.g.hist) + 1);
    const size_t obytes = n_out * sizeof(float);
    HostStage st("ss_resample_stream");
    float *d_out = st.room<float>(obytes);
    const auto d_named = st.up_pool(named);
    const T *d_x = flush ? nullptr : st.up(x, n_in * sizeof(T));
    const int64_t *d_so = flush ? nullptr : st.up(so, (n_active + 1) * sizeof(int64_t));
    if (st.ok())
        st.ran(flush ? stream_launch<float, true>(rs, nullptr, n_active, nullptr, 0, d_named.slots, n_active, 1.0f, d_named.rows, d_out, nullptr)
                     : stream_device<T>(rs, d_x, n_active, d_so, n_in, d_named.slots, n_active, scale, d_named.rows, d_out, nullptr));
    st.sync();
    st.down_pool(named, d_named);
    st.down(out, d_out, obytes);
    st.scatter(named, pool, slots);
    return st.status();
}

template <typename T>
int stream_host(const ss_resampler *rs, const T *x, size_t n_active, const int64_t *so, const int32_t *slots, size_t pool_streams, float scale, float *pool,
                float *out)
{
    if (n_active == 0) return SS_OK;
    if (!rs) return fail(SS_ERR_ARG, "null resampler");
    if (!so) return fail(SS_ERR_ARG, "null buffer");
    if (n_active >= (1ull << 31)) return fail(SS_ERR_ARG, "n_active and pool_streams must be below 2^31, total_in below 2^40");
    const Geom &g = rs->f.g;
    if (so[0] != 0) return fail(SS_ERR_ARG, "sample_offsets[0] must be 0 (entry 0)");
    for (size_t i = 0; i < n_active; ++i) {
        if (so[i + 1] < so[i]) return fail(SS_ERR_ARG, "decreasing sample offsets at entry " + std::to_string(i));
        if ((so[i + 1] - so[i]) % g.o != 0)
            return fail(SS_ERR_ARG, "entry " + std::to_string(i) + " brings " + std::to_string(so[i + 1] - so[i]) + " samples, not whole periods of " +
                                        std::to_string(g.o));
    }
    const size_t n_in = static_cast<size_t>(so[n_active]);
    int rc = check_stream(false, rs, x, so, slots, n_active, n_in, pool_streams, scale, pool, out);
    if (rc || (rc = check_slots(slots, n_active, pool_streams))) return rc;
    if (n_in == 0) return SS_OK;  // empty entries only: nothing moves
    return stream_via_device<T>(false, rs, x, n_active, so, slots, n_in, n_in / g.o * g.n, scale, pool, out);
}

}  // namespace

}  // namespace ss

extern "C" {

int ss_resample_sizes(uint32_t orig_rate, uint32_t new_rate, uint32_t lowpass_filter_width, float rolloff, ss_resample_info *info)
{
    if (!info) return ss::fail(SS_ERR_ARG, "null output");
    ss::Filter f;
    const int rc = ss::build_filter(orig_rate, new_rate, lowpass_filter_width, rolloff, false, f);
    if (rc) return rc;
    ss::fill_info(f.g, info);
    return SS_OK;
}

int ss_resample_taps(uint32_t orig_rate, uint32_t new_rate, uint32_t lowpass_filter_width, float rolloff, float *h, int32_t *first, int32_t *count)
{
    if (!h) return ss::fail(SS_ERR_ARG, "null output");
    ss::Filter f;
    const int rc = ss::build_filter(orig_rate, new_rate, lowpass_filter_width, rolloff, true, f);
    if (rc) return rc;
    std::memcpy(h, f.h.data(), f.h.size() * sizeof(float));
    if (first) std::memcpy(first, f.first.data(), f.first.size() * sizeof(int32_t));
    if (count) std::memcpy(count, f.count.data(), f.count.size() * sizeof(int32_t));
    return SS_OK;
}

int ss_resample_len(uint32_t orig_rate, uint32_t new_rate, size_t n_samples, size_t *out_len)
{
    if (!out_len) return ss::fail(SS_ERR_ARG, "null output");
    if (orig_rate == 0 || new_rate == 0) return ss::fail(SS_ERR_ARG, "a sample rate of 0");
    if (n_samples >= (1ull << 62) / new_rate) return ss::fail(SS_ERR_ARG, "n_samples too large");
    const uint64_t gc = std::gcd(orig_rate, new_rate), o = orig_rate / gc, n = new_rate / gc;
    *out_len = static_cast<size_t>((n_samples * n + o - 1) / o);
    return SS_OK;
}

int ss_resample_packed_offsets(uint32_t orig_rate, uint32_t new_rate, size_t n_clips, const int64_t *sample_offsets, int64_t *out_offsets)
{
    if (!sample_offsets || !out_offsets) return ss::fail(SS_ERR_ARG, "null buffer");
    if (orig_rate == 0 || new_rate == 0) return ss::fail(SS_ERR_ARG, "a sample rate of 0");
    if (sample_offsets[0] != 0) return ss::fail(SS_ERR_ARG, "sample_offsets[0] must be 0 (clip 0)");
    const uint64_t gc = std::gcd(orig_rate, new_rate), o = orig_rate / gc, n = new_rate / gc;
    for (size_t b = 0; b < n_clips; ++b) {
        if (sample_offsets[b + 1] < sample_offsets[b]) return ss::fail(SS_ERR_ARG, "decreasing sample offsets at clip " + std::to_string(b));
        if (static_cast<uint64_t>(sample_offsets[b + 1] - sample_offsets[b]) >= (1ull << 31))
            return ss::fail(SS_ERR_ARG, "clip " + std::to_string(b) + " is longer than 2^31 - 1 samples");
    }
    out_offsets[0] = 0;
    for (size_t b = 0; b < n_clips; ++b) {
        const uint64_t len = static_cast<uint64_t>(sample_offsets[b + 1] - sample_offsets[b]);
        out_offsets[b + 1] = out_offsets[b] + static_cast<int64_t>((len * n + o - 1) / o);
    }
    return SS_OK;
}

int ss_resampler_create(uint32_t orig_rate, uint32_t new_rate, uint32_t lowpass_filter_width, float rolloff, ss_resampler **out)
{
    if (!out) return ss::fail(SS_ERR_ARG, "null output");
    *out = nullptr;
    ss_resampler *rs = new ss_resampler;
    const int rc = ss::build_filter(orig_rate, new_rate, lowpass_filter_width, rolloff, true, rs->f);
    if (rc) {
        delete rs;
        return rc;
    }
    const ss::Geom &g = rs->f.g;
    rs->tab.assign(g.tab_words, 0u);
    float *h = reinterpret_cast<float *>(rs->tab.data() + 2 * g.n);
    for (unsigned i = 0; i < g.n; ++i) {
        rs->tab[2 * i] = static_cast<uint32_t>(rs->f.first[i]);
        rs->tab[2 * i + 1] = static_cast<uint32_t>(rs->f.count[i]);
        std::memcpy(h + static_cast<size_t>(i) * g.pitch, rs->f.h.data() + static_cast<size_t>(i) * g.taps, g.taps * sizeof(float));
    }
    *out = rs;
    return SS_OK;
}

void ss_resampler_destroy(ss_resampler *rs)
{
    if (!rs) return;
    if (rs->d_tab) (void)hipFree(rs->d_tab);
    delete rs;
}

int ss_resampler_info(const ss_resampler *rs, ss_resample_info *info)
{
    if (!rs || !info) return ss::fail(SS_ERR_ARG, "null argument");
    ss::fill_info(rs->f.g, info);
    return SS_OK;
}

int ss_resample_device(const ss_resampler *rs, const float *d_x, size_t batch, size_t n_samples, size_t ld, float *d_out, size_t ld_out, void *stream)
{
    return ss::dense_device<float>(rs, d_x, batch, n_samples, ld, 1.0f, d_out, ld_out, stream);
}

int ss_resample(const ss_resampler *rs, const float *x, size_t batch, size_t n_samples, size_t ld, float *out, size_t ld_out)
{
    return ss::dense_host<float>(rs, x, batch, n_samples, ld, 1.0f, out, ld_out);
}

int ss_resample_i16_device(const ss_resampler *rs, const int16_t *d_x, size_t batch, size_t n_samples, size_t ld, float scale, float *d_out, size_t ld_out,
                           void *stream)
{
    return ss::dense_device<int16_t>(rs, d_x, batch, n_samples, ld, scale, d_out, ld_out, stream);
}

int ss_resample_i16(const ss_resampler *rs, const int16_t *x, size_t batch, size_t n_samples, size_t ld, float scale, float *out, size_t ld_out)
{
    return ss::dense_host<int16_t>(rs, x, batch, n_samples, ld, scale, out, ld_out);
}

int ss_resample_packed_device(const ss_resampler *rs, const float *d_x, size_t n_clips, const int64_t *d_sample_offsets, const int64_t *d_out_offsets,
                              size_t total_in, size_t total_out, float *d_out, void *stream)
{
    return ss::packed_device<float>(rs, d_x, n_clips, d_sample_offsets, 1.0f, d_out_offsets, total_in, total_out, d_out, stream);
}

int ss_resample_packed(const ss_resampler *rs, const float *x, size_t n_clips, const int64_t *sample_offsets, const int64_t *out_offsets, float *out)
{
    return ss::packed_host<float>(rs, x, n_clips, sample_offsets, 1.0f, out_offsets, out);
}

int ss_resample_packed_i16_device(const ss_resampler *rs, const int16_t *d_x, size_t n_clips, const int64_t *d_sample_offsets, float scale,
                                  const int64_t *d_out_offsets, size_t total_in, size_t total_out, float *d_out, void *stream)
{
    return ss::packed_device<int16_t>(rs, d_x, n_clips, d_sample_offsets, scale, d_out_offsets, total_in, total_out, d_out, stream);
}

int ss_resample_packed_i16(const ss_resampler *rs, const int16_t *x, size_t n_clips, const int64_t *sample_offsets, float scale, const int64_t *out_offsets,
                           float *out)
{
    return ss::packed_host<int16_t>(rs, x, n_clips, sample_offsets, scale, out_offsets, out);
}

int ss_resample_stream_state_len(const ss_resampler *rs, size_t *state_len)
{
    if (!rs || !state_len) return ss::fail(SS_ERR_ARG, "null argument");
    *state_len = static_cast<size_t>(rs->f.g.hist) + 1;
    return SS_OK;
}

int ss_resample_stream_packed_device(const ss_resampler *rs, const float *d_x, size_t n_active, const int64_t *d_sample_offsets, size_t total_in,
                                     const int32_t *d_slots, size_t pool_streams, float *d_pool, float *d_out, void *stream)
{
    return ss::stream_device<float>(rs, d_x, n_active, d_sample_offsets, total_in, d_slots, pool_streams, 1.0f, d_pool, d_out, stream);
}

int ss_resample_stream_packed(const ss_resampler *rs, const float *x, size_t n_active, const int64_t *sample_offsets, const int32_t *slots,
                              size_t pool_streams, float *pool, float *out)
{
    return ss::stream_host<float>(rs, x, n_active, sample_offsets, slots, pool_streams, 1.0f, pool, out);
}

int ss_resample_stream_packed_i16_device(const ss_resampler *rs, const int16_t *d_x, size_t n_active, const int64_t *d_sample_offsets, size_t total_in,
                                         const int32_t *d_slots, size_t pool_streams, float scale, float *d_pool, float *d_out, void *stream)
{
    return ss::stream_device<int16_t>(rs, d_x, n_active, d_sample_offsets, total_in, d_slots, pool_streams, scale, d_pool, d_out, stream);
}

int ss_resample_stream_packed_i16(const ss_resampler *rs, const int16_t *x, size_t n_active, const int64_t *sample_offsets, const int32_t *slots,
                                  size_t pool_streams, float scale, float *pool, float *out)
{
    return ss::stream_host<int16_t>(rs, x, n_active, sample_offsets, slots, pool_streams, scale, pool, out);
}

int ss_resample_stream_flush_device(const ss_resampler *rs, size_t n_active, const int32_t *d_slots, size_t pool_streams, float *d_pool, float *d_out,
                                    void *stream)
{
    if (n_active == 0) return SS_OK;
    const int rc = ss::check_stream<float>(true, rs, nullptr, nullptr, d_slots, n_active, 0, pool_streams, 1.0f, d_pool, d_out);
    if (rc) return rc;
    return ss::stream_launch<float, true>(rs, nullptr, n_active, nullptr, 0, d_slots, pool_streams, 1.0f, d_pool, d_out, stream);
}

int ss_resample_stream_flush(const ss_resampler *rs, size_t n_active, const int32_t *slots, size_t pool_streams, float *pool, float *out)
{
    if (n_active == 0) return SS_OK;
    int rc = ss::check_stream<float>(true, rs, nullptr, nullptr, slots, n_active, 0, pool_streams, 1.0f, pool, out);
    if (rc || (rc = ss::check_slots(slots, n_active, pool_streams))) return rc;
    const ss::Geom &g = rs->f.g;
    return ss::stream_via_device<float>(true, rs, nullptr, n_active, nullptr, slots, 0, n_active * g.latency * g.n, 1.0f, pool, out);
}

}  // extern "C"
