// Kernel argument block and launcher declarations shared by ss_kernels.hip and ss_api.hip.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <type_traits>

#include "speechsauce_amd.h"
#include "ss_launch_plan.h"

// Product / lab builds.  The shipped library is the PRODUCT build: kernel selection is a pure function of the configuration
// and the call -- no environment knob is read anywhere, and the timing-attribution switches of the headline kernel
// (SS_ABLATE) are compiled out.  `make lab` (-DSS_LAB=1) builds libspeechsauce_amd_lab.so with the A/B knobs (SS_RES,
// SS_WAVES, SS_MEL_WAVES, SS_HOST_CHUNK_MB, SS_HOST_SMALL_KB, SS_DEBUG_TIMES, SS_DEBUG_ROWS) and the stage-removal builds
// tools/ablate.sh drives, and the process-wide test aids of include/speechsauce_amd_debug.h (LDS poisoning, kernel-selection
// overrides, fault injection, the stamp buffer): those exist in the lab library ONLY.
#ifndef SS_LAB
#define SS_LAB 0
#endif
#if !SS_LAB
#define SS_PRODUCT 1
#endif

namespace ss {

// Process-wide test aids set through include/speechsauce_amd_debug.h (ss_api.hip, lab builds); constants in the product build
#if SS_LAB
bool dbg_force_generic();        // ss_debug_force_generic: every configuration on the generic kernel
bool dbg_mel_tile_off();         // ss_debug_mel_tile(0): eight waves, direct stores instead of the whole-line tile
int dbg_mel_build();             // 0 automatic, 1 = the above, 2 eight-wave builds only, 3 the twelve-wave build where it exists
unsigned dbg_tile_spin_limit();  // polls before a tile hand-off counts as a protocol error (ss_debug_tile_fault: 0)
#else
constexpr bool dbg_force_generic() { return false; }
constexpr bool dbg_mel_tile_off() { return false; }
constexpr int dbg_mel_build() { return 0; }
constexpr unsigned dbg_tile_spin_limit() { return 1u << 24; }
#endif

enum OutKind : int32_t {
    OUT_MFCC = 0,   // [frames x num_cepstral]                    feature.rs:99-148
    OUT_MFE = 1,    // feat [frames x M] + energy [frames]        feature.rs:200-233
    OUT_POWER = 2,  // P [frames x F]                             processing.rs:179-181
    OUT_MEL = 3,    // [clips x M x R]                            feature.rs:151-174
    OUT_STFT = 4    // [clips x R x F x 2]                        functions.rs:86-123
};

enum FrameMode : int32_t { FRAME_NORMAL = 0, FRAME_ZERO = 1, FRAME_FIRST = 2, FRAME_CENTER = 3, FRAME_PADDED = 4 };

struct FrontArgs {
    // input: `batch` clips of `n_samples`, row stride `ld` elements
    const float *x;
    unsigned long long ld;
    uint32_t n_samples;
    uint32_t batch;
    // MFCC framing (processing.rs:65-129)
    uint32_t flen, step, n_frames;
    int32_t frame_mode;
    int32_t pad_reflect;  // FRAME_CENTER: 1 = np.pad 'reflect' outside the clip, 0 = zeros
    float preemph;
    uint32_t preemph_shift;
    // STFT framing (functions.rs:86-170)
    uint32_t hop, n_pad, rows, real_rows;
    const float *window;  // MFCC: [flen] or null; STFT: [n_fft]
    float scale;          // MFCC: 1/N (processing.rs:180); STFT: wnorm (config.rs:178)
    int32_t spectrum_exponent;
    // FFT tables
    const float2 *tw_c;  // exp(-2 pi i t / C), t < C
    const float2 *tw_n;  // exp(-2 pi i k / N), k <= C/2
    // chirp-z mode (fft_points not a power of two): the FFT is a complex one of C = blu_len points
    const float2 *blu_c;  // exp(-i pi n^2 / N), n < N
    const float2 *blu_b;  // FFT_C of the wrapped conjugate chirp
    uint32_t blu_n;       // N = fft_points (0: packed power-of-two mode)
    // sparse mel bank
    const int32_t *f_start, *f_len, *f_off;
    const float *f_w;
    uint32_t n_filters;
    // DCT
    const float *dct;  // [n_ceps x n_filters]
    uint32_t n_ceps;
    float dct_scale_k;   // multiplier of columns >= 1 (gain * norm)
    float dct_scale_0;   // multiplier of column 0, row t > 0
    float dct_scale_00;  // multiplier of element [0,0] of each clip
    int32_t dc_elimination;
    // outputs
    int32_t out_kind;
    float *out0;
    float *out1;
};

struct LaunchInfo {
    const char *kernel_name;
    unsigned grid, block;
    size_t lds_bytes;
    bool db_fused = false;  // the launch was a dB build (DbArgs below): the output already holds decibels
};

// The launch step of the fused kernels: `waves` waves per workgroup, `lds` bytes of dynamic LDS (the attribute lifts the 48 KiB a
// kernel gets without it), what ran reported through `info`.
template <typename Kern, typename... Args>
hipError_t launch_kernel(Kern kern, const char *name, unsigned grid, int waves, size_t lds, hipStream_t stream, LaunchInfo *info, const Args &...args)
{
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds));
    if (e != hipSuccess) return e;
    if (info) *info = LaunchInfo{name, grid, static_cast<unsigned>(waves * 64), lds};
    hipLaunchKernelGGL(kern, dim3(grid), dim3(waves * 64), lds, stream, args...);
    return hipGetLastError();
}

// Generic front-end (any power-of-two fft_points in [32, 4096]; with a.blu_n != 0 the chirp-z build for other lengths, log2c then
// being the length of its complex FFT).
struct DbArgs;  // (below: the dB builds of the mel output)
hipError_t launch_front_generic(const FrontArgs &a, uint32_t log2c, hipStream_t stream, int num_cus, LaunchInfo *info, const DbArgs *db = nullptr);

// Packed variable-length clips (ss_mfcc_packed_device / ss_mfe_packed_device): clip b is x[so[b] : so[b+1]], its frames are rows
// fo[b] .. fo[b+1] of the output.  Both tables are device arrays the host may never have seen, so the kernels recompute every
// clip's frame count from `so` (the host's ss::num_frames in f32, bit for bit) and skip -- and report through `err` -- a clip whose
// rows disagree with it or end past total_frames.  The per-clip DCT scales (feature.rs:126-131, n = T_b * M) are formed on the
// device with correctly rounded operations: the same bits as the host's for an equal-length batch of that clip.
struct VarlenArgs {
    const long long *so;  // [n_clips + 1] sample offsets
    const long long *fo;  // [n_clips + 1] frame (output row) offsets
    unsigned long long total_frames;  // rows of the output block
    uint32_t n_clips;
    int32_t framing;      // SS_FRAMING_* (literal framing: FRAME_ZERO / FRAME_FIRST from each clip's own T_b)
    int32_t pad_reflect;  // centred frames: clips of <= flen / 2 samples have no frames with np.pad 'reflect'
    int32_t dct_ortho;    // SS_DCT_ORTHO: the scales do not depend on T_b (FrontArgs / Fast512Args carry them)
    float dct2_gain;
    unsigned *err;        // the config's device error word (set to kVarlenError on a bad clip)
};
constexpr unsigned kVarlenError = 2u;

// The offset tables of the packed layouts (fo / ro below: n non-decreasing offsets, the rows of clip or entry i start at off[i]).
// The owner of row g: the last i < n with off[i] <= g (binary search; any i for offsets that are not non-decreasing -- the decoders
// below then find them inconsistent, or g outside the owner's rows.  Entries without rows share their offset with their successor
// and are stepped over; the caller still checks g < off[i + 1]).
__device__ __forceinline__ unsigned offset_find(const long long *off, unsigned n, long long g)
{
    unsigned lo = 0u, hi = n;
    while (hi - lo > 1u) {
        const unsigned mid = (lo + hi) >> 1;
        if (off[mid] <= g) lo = mid;
        else hi = mid;
    }
    return lo;
}
// The same from a lower bound c the caller already knows (the owner of an earlier row): a few steps along the offsets, and the
// binary search where that does not get there.
__device__ __forceinline__ unsigned offset_seek(const long long *off, unsigned n, unsigned c, long long g)
{
    for (int k = 0; k < 4 && c + 1 < n && off[c + 1] <= g; ++k) ++c;
    if (c + 1 < n && off[c + 1] <= g) c = offset_find(off, n, g);
    return c;
}
// The quad kernels' form (ss_kaldi_c256, ss_nemo_c256): the owner (clip of a packed launch, entry of a pool launch) of row
// g = q4 + 0..3 over the row offsets `off`: the owner of the quad's first row from the wave's forward cursor (claims only increase),
// then at most three owners WITH rows further on.
__device__ __forceinline__ unsigned row_owner(const long long *off, unsigned n, unsigned q4, unsigned g, unsigned &cursor)
{
    unsigned c = offset_seek(off, n, cursor, q4);
    cursor = c;
    bool step = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        step = c + 1 < n && off[c + 1] <= static_cast<long long>(g);
        c += step ? 1u : 0u;
    }
    // owners without rows inside the quad (off[b] == off[b + 1]) take steps of their own: a lane that took all three looks once
    // more, and searches where they did not get there
    if (step && c + 1 < n && off[c + 1] <= static_cast<long long>(g)) c = offset_find(off, n, static_cast<long long>(g));
    return c;
}

// Frames of a clip of L samples, as ss::num_frames computes them on the host (processing.rs:101 in f32; padded: ceil; centred:
// 1 + L / step).  0: the clip yields none (the host rejects it) or is longer than 2^31 - 1 samples.
__device__ __forceinline__ unsigned varlen_frames(const VarlenArgs &v, uint32_t flen, uint32_t step, long long L)
{
    if (L < 0 || L > 0x7fffffffll) return 0u;
    const unsigned n = static_cast<unsigned>(L);
    if (v.framing == SS_FRAMING_CENTER) return (n == 0u || (v.pad_reflect && n <= flen / 2)) ? 0u : 1u + n / step;
    if (n < flen) return 0u;
    const float q = __fdiv_rn(__uint2float_rn(n - flen), __uint2float_rn(step));
    return static_cast<unsigned>(v.framing == SS_FRAMING_PADDED ? ceilf(q) : floorf(q));
}

// Clip b of a packed launch: where its samples start, how many there are, its frame count and its first output row.  ok: the
// offsets agree with each other (rows fo[b] .. fo[b+1] are exactly the T_b frames `so` implies, inside the output block).
struct VarClip {
    long long s0, f0;
    unsigned n, T;
    bool ok;
};
__device__ __forceinline__ VarClip varlen_clip(const VarlenArgs &v, uint32_t flen, uint32_t step, unsigned b)
{
    VarClip c;
    c.s0 = v.so[b];
    c.f0 = v.fo[b];
    const long long s1 = v.so[b + 1], f1 = v.fo[b + 1];
    c.T = varlen_frames(v, flen, step, s1 - c.s0);
    c.n = static_cast<unsigned>(s1 - c.s0);
    c.ok = c.T > 0u && c.s0 >= 0 && c.f0 >= 0 && f1 - c.f0 == static_cast<long long>(c.T) &&
           static_cast<unsigned long long>(f1) <= v.total_frames;
    return c;
}
// feature.rs:126-131 for a clip of T frames (n = T * M as f32): the host's g * (1 / sqrtf(2 n)) and g * (1 / sqrtf(4 n)),
// correctly rounded step by step.  (sqrtf and the division are correctly rounded in HIP's default fp32 mode; __fsqrt_rn is not
// here -- it maps to the native square root unless OCML_BASIC_ROUNDED_OPERATIONS is defined.)
__device__ __forceinline__ void varlen_dct_scales(const VarlenArgs &v, unsigned T, unsigned M, float &scale_k, float &scale_00)
{
    const float nn = __ull2float_rn(static_cast<unsigned long long>(T) * M);
    scale_k = __fmul_rn(v.dct2_gain, __fdiv_rn(1.0f, sqrtf(__fmul_rn(2.0f, nn))));
    scale_00 = __fmul_rn(v.dct2_gain, __fdiv_rn(1.0f, sqrtf(__fmul_rn(4.0f, nn))));
}
// One pass over the clips, spread over the grid: a clip whose offsets are inconsistent sets the error word (its frames are
// skipped where they are computed).  A vector store to the pinned word.
__device__ __forceinline__ void varlen_check_clips(const VarlenArgs &v, uint32_t flen, uint32_t step, unsigned tid, unsigned nthreads)
{
    bool bad = false;
    for (unsigned b = tid; b < v.n_clips; b += nthreads) bad |= !varlen_clip(v, flen, step, b).ok;
    if (bad && v.err) __hip_atomic_store(v.err, kVarlenError, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
// every configuration (fft_points, windows, pre-emphasis, framing, DCT norm, exponent, banks): the varlen build of
// ss_front_generic.  a: as for launch_front_generic with x = the packed samples; batch / n_samples / n_frames are unused.
hipError_t launch_front_generic_varlen(const FrontArgs &a, const VarlenArgs &v, uint32_t log2c, hipStream_t stream, int num_cus,
                                       LaunchInfo *info);

// Packed variable-length clips on the STFT path (ss_mel_spectrogram_packed_device / ss_stft_packed_device): clip b is
// x[so[b] : so[b+1]], its R_b = ceil(n_b / hop) rows are rows ro[b] .. ro[b+1] of the packed row space -- mel: clip b's [M x R_b]
// block starts at out + M ro[b]; stft: rows ro[b] .. ro[b+1] of [total_rows x F].  As with VarlenArgs, the kernels recompute every
// R_b from `so` (the host's ss::stft_rows in f32, bit for bit) and skip -- and report through `err` -- a clip whose rows disagree
// with it or end past total_rows.
struct VarRowsArgs {
    const long long *so;  // [n_clips + 1] sample offsets
    const long long *ro;  // [n_clips + 1] row offsets
    unsigned long long total_rows;  // rows of the output block
    uint32_t n_clips;
    uint32_t hop;
    unsigned *err;        // the config's device error word (set to kVarlenError on a bad clip)
};
// Rows of a clip of L samples, as ss::stft_rows computes them on the host (functions.rs:97 in f32).  0: an empty clip (the host
// rejects it) or one longer than 2^31 - 1 samples.
__device__ __forceinline__ unsigned varrows_rows(uint32_t hop, long long L)
{
    if (L <= 0 || L > 0x7fffffffll) return 0u;
    return static_cast<unsigned>(ceilf(__fdiv_rn(__uint2float_rn(static_cast<unsigned>(L)), __uint2float_rn(hop))));
}
// Clip b of a packed STFT-path launch: its first sample, its length, its rows and its first packed row.  ok: the offsets agree
// with each other (rows ro[b] .. ro[b+1] are exactly the R_b rows `so` implies, inside the output block).
struct VarRowClip {
    long long s0, r0;
    unsigned n, R;
    bool ok;
};
__device__ __forceinline__ VarRowClip varrows_clip(const VarRowsArgs &v, unsigned b)
{
    VarRowClip c;
    c.s0 = v.so[b];
    c.r0 = v.ro[b];
    const long long s1 = v.so[b + 1], r1 = v.ro[b + 1];
    c.R = varrows_rows(v.hop, s1 - c.s0);
    c.n = static_cast<unsigned>(s1 - c.s0);
    c.ok = c.R > 0u && c.s0 >= 0 && c.r0 >= 0 && r1 - c.r0 == static_cast<long long>(c.R) &&
           static_cast<unsigned long long>(r1) <= v.total_rows;
    return c;
}
// One pass over the clips, spread over the grid (see varlen_check_clips).  A vector store to the pinned word.
__device__ __forceinline__ void varrows_check_clips(const VarRowsArgs &v, unsigned tid, unsigned nthreads)
{
    bool bad = false;
    for (unsigned b = tid; b < v.n_clips; b += nthreads) bad |= !varrows_clip(v, b).ok;
    if (bad && v.err) __hip_atomic_store(v.err, kVarlenError, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
// mel output at any fft_points (chirp-z included) and every stft output: the packed-rows build of ss_front_generic's STFT / mel path.
// a: as for launch_front_generic's STFT path with x = the packed samples; batch / n_samples / rows / real_rows are unused.
hipError_t launch_front_generic_varrows(const FrontArgs &a, const VarRowsArgs &v, uint32_t log2c, hipStream_t stream, int num_cus,
                                        LaunchInfo *info, const DbArgs *db = nullptr);

// Streaming STFT (ss_stft_stream_device / ss_mel_spectrogram_stream_device): every stream (a row of the batch) carries the last
// S = fft_points - hop samples it was fed (config.rs:162, functions.rs:137-160).  A window that reaches before the chunk reads them:
// sample p < 0 of stream s is state[s * S + S + p] (p >= -S always holds: a row's window ends at least one hop into the chunk).
struct StreamArgs {
    const float *state;  // [batch][state_len]
    uint32_t state_len;  // S
};
// The argument of type T in a kernel's trailing argument pack (empty pack: none) -- the builds with an empty pack keep the argument
// block, and the code, they had before the pack existed.
template <typename T, typename... V>
__device__ __forceinline__ const T *pack_arg(const V &...v)
{
    const T *p = nullptr;
    (
        [&] {
            if constexpr (std::is_same_v<T, V>) p = &v;
        }(),
        ...);
    return p;
}
// The dB epilogue of the mel kernels (ss_log_mel_spectrogram*): a DbArgs LAST in the trailing argument pack -- behind the layout's own
// argument and behind a BatchPcmArgs -- selects it the way a BatchPcmArgs selects the PCM loader.  Every mel value goes through
// power_db() just before it is stored; with max_key non-null the largest dB value of every clip is gathered into max_key[clip]
// (float_key order, integer atomicMax: the result does not depend on the order of arrival) for the top_db floor pass behind the
// launch.  max_key must hold 0x80808080 in every word at launch (below the key of every finite float).
struct DbArgs {
    float amin, ref_db;  // ref_db = 10 log10(max(amin, |ref|)), formed on the host
    int *max_key;        // [clips] or null (no floor: nothing is reduced)
};
// librosa's power_to_db of one element: 10 log10(max(amin, s)) - ref_db, the product and the difference as ONE fma (what the device
// default contraction makes of ss_post.hip's `10.0f * log10f(..) - ref_db`)
__device__ __forceinline__ float power_db(float s, float amin, float ref_db) { return fmaf(10.0f, log10f(fmaxf(amin, s)), -ref_db); }
// floats as ordered integers, so that atomicMax on an int finds the largest float (negative values included)
__device__ __forceinline__ int float_key(float v)
{
    const int b = __float_as_int(v);
    return b >= 0 ? b : b ^ 0x7fffffff;
}
__device__ __forceinline__ float key_float(int k) { return __int_as_float(k >= 0 ? k : k ^ 0x7fffffff); }
// The launches around a log-mel mel launch (ss_post.hip).  In front of it, with a floor: max_key[0 .. clips) := 0x80808080.  Behind it:
// the top_db floor out[i] = max(out[i], max of i's clip - top_db) over
// equal-length clips of `seg` elements each (no table) / over the [M x R_b] blocks of a packed call's clips (cols = M; a clip that
// the mel kernels' table check skips is left alone); and, behind a mel kernel without a dB build, power_db over equal-length
// clips in place with the maxima gathered as the dB builds gather them.
hipError_t launch_db_keys_init(int *max_key, size_t clips, hipStream_t stream);
hipError_t launch_db_floor_equal(float *out, size_t clips, size_t seg, float top_db, const int *max_key, hipStream_t stream);
hipError_t launch_db_floor_varrows(float *out, const VarRowsArgs &v, size_t cols, float top_db, const int *max_key, hipStream_t stream);
hipError_t launch_power_to_db_equal(float *x, size_t clips, size_t seg, const DbArgs &db, hipStream_t stream);

// Packed feature rows (the packed calls of ss_post.hip and ss_deltas.hip): clip b = blockIdx.x owns rows off[b] .. off[b+1] of a
// block of total_rows rows.  A segment that is reversed, starts below 0 or ends past total_rows comes back empty.
struct Segment {
    unsigned long long row0;
    unsigned rows;  // 0: nothing to do (empty or rejected segment)
};
__device__ __forceinline__ Segment packed_segment(const long long *__restrict__ off, unsigned long long total_rows)
{
    const long long lo = off[blockIdx.x], hi = off[blockIdx.x + 1];
    Segment s{0, 0};
    if (lo >= 0 && lo < hi && static_cast<unsigned long long>(hi) <= total_rows) {  // total_rows < 2^31: the row count fits
        s.row0 = static_cast<unsigned long long>(lo);
        s.rows = static_cast<unsigned>(hi - lo);
    }
    return s;
}
// Workgroups per clip (gridDim.y) of a launch over packed clips: about 8192 workgroups in all, so that a block of few long clips still
// fills the device, at most 64 per clip and never more than the longest possible clip has work for (most_useful).  Sized from what
// the host knows; the bits of the results do not depend on it.
inline unsigned packed_split(size_t n_clips, unsigned long long most_useful)
{
    const unsigned long long want = std::max<unsigned long long>(1, 8192 / n_clips);
    return static_cast<unsigned>(std::min<unsigned long long>(64, std::min(want, std::max<unsigned long long>(1, most_useful))));
}

// The pools of raw feature rows (ss_deltas.hip, ss_splice.hip): entry i = blockIdx.x owns rows ro[i] .. ro[i+1] of the blocks and
// pool row slots[i] of state_len = hist * cols + 1 floats -- the stream's last `hist` raw rows (oldest first, right-aligned, zeros
// in front) and, in the last float, how many of them are valid.  An entry with a slot outside the pool, or (not the flush) a pair
// that is empty, reversed, starts below 0 or ends past total_rows, comes back with state == nullptr; a count word that is not an
// integer in [0, hist] is read as 0.  The flush build has no table: entry i owns rows i * flush_rows .. of out.
struct RowPoolEntry {
    unsigned long long row0;  // first row of the entry in vec / out (flush: in out)
    unsigned rows;            // new rows
    unsigned count;           // valid history rows, 0 .. hist
    float *state;             // the entry's pool row; nullptr: a rejected entry
};
template <bool FLUSH>
__device__ __forceinline__ RowPoolEntry row_pool_entry(const long long *__restrict__ ro, const int *__restrict__ slots, unsigned long long total_rows,
                                                      unsigned pool_streams, float *pool, unsigned state_len, unsigned hist, unsigned flush_rows)
{
    RowPoolEntry e{0, 0, 0, nullptr};
    const int slot = slots[blockIdx.x];
    if (slot < 0 || static_cast<unsigned>(slot) >= pool_streams) return e;
    if (FLUSH) {
        e.row0 = static_cast<unsigned long long>(blockIdx.x) * flush_rows;
    } else {
        const long long lo = ro[blockIdx.x], hi = ro[blockIdx.x + 1];
        if (!(lo >= 0 && lo < hi && static_cast<unsigned long long>(hi) <= total_rows)) return e;
        e.row0 = static_cast<unsigned long long>(lo);
        e.rows = static_cast<unsigned>(hi - lo);  // total_rows < 2^31: the row count fits
    }
    e.state = pool + static_cast<size_t>(slot) * state_len;
    const float cw = e.state[state_len - 1];
    if (cw >= 0.0f && cw <= static_cast<float>(hist) && cw == floorf(cw)) e.count = static_cast<unsigned>(cw);
    return e;
}
// the streaming build of ss_front_generic's STFT / mel path (any fft_points, chirp-z included): a as for launch_front_generic's
// STFT path, on the chunk (n_pad 0 and real_rows = rows in continuous mode)
hipError_t launch_front_generic_stream(const FrontArgs &a, const StreamArgs &s, uint32_t log2c, hipStream_t stream, int num_cus,
                                       LaunchInfo *info);
// The state advance, a second stream-ordered launch behind the rows: state row s := the last S samples of (old row ++ the chunk's
// first `advance` samples, zeros past n_samples).  One workgroup per stream, in place (every read of a block of the row is done
// before any lane of the workgroup writes it).
hipError_t launch_stream_advance(float *state, uint32_t state_len, const float *x, unsigned long long ld, uint32_t n_samples,
                                 uint32_t advance, uint32_t batch, hipStream_t stream);

// Streaming MFCC / mfe (ss_mfcc_stream_device / ss_mfe_stream_device): row t of a call (the stream's frame that ends at chunk
// sample (t + 1) * step) starts at chunk sample t * step - lead, lead = flen - step.  Stream s carries the last
// S = max(flen + sh - step, 0) samples it was fed (sh: the pre-emphasis shift, 0 without pre-emphasis): sample p < 0 of stream s is
// state[s * S + S + p], and every frame sample and pre-emphasis tap that a row reads has p >= -S.
struct FrameStreamArgs {
    const float *state;  // [batch][state_len]; null where state_len == 0
    uint32_t state_len;  // S
    int32_t lead;        // flen - step (negative where frames are shorter than the hop)
};
// the streaming build of ss_front_generic's MFCC / mfe path (any configuration the generic kernel serves, contract or padded framing):
// a as for launch_front_generic's MFCC path with n_frames = rows per stream, frame_mode FRAME_NORMAL and dct_scale_00 = dct_scale_0
hipError_t launch_front_generic_frame_stream(const FrontArgs &a, const FrameStreamArgs &s, uint32_t log2c, hipStream_t stream, int num_cus,
                                             LaunchInfo *info);

// Ragged streaming MFCC / mfe over a pool of stream states (ss_mfcc_stream_packed_device / ss_mfe_stream_packed_device): entry i of
// a call is the chunk x[so[i] : so[i+1]] (R_i = n_i / step whole hops, R_i = 0 allowed) of the stream whose state is row slots[i] of
// the pool; its rows are rows ro[i] .. ro[i+1] of the packed output.  Row t of an entry reads as row t of a dense streaming call on
// that stream alone (FrameStreamArgs above): sample p < 0 is pool[slots[i] * S + S + p].  The three tables are device arrays the
// host may never have seen (and may change between graph replays), so both kernels decode every entry with stream_entry() and
// skip -- and report through `err` -- one that is inconsistent.
struct FrameStreamPackedArgs {
    float *pool;             // [pool_streams][state_len]; null where state_len == 0
    uint32_t state_len;      // S
    int32_t lead;            // flen - step (negative where frames are shorter than the hop)
    const long long *so;     // [n_active + 1] sample offsets
    const long long *ro;     // [n_active + 1] row offsets
    const int32_t *slots;    // [n_active] pool row of each entry
    uint32_t n_active;
    uint32_t pool_streams;
    uint32_t total_rows;     // rows of the output block
    uint32_t step;
    unsigned *err;           // the config's device error word (set to kVarlenError on a bad entry)
};
// Entry i of a ragged streaming launch: where its chunk starts, its length, its rows, its first output row and its pool row.
// ok: the chunk is whole hops, rows ro[i] .. ro[i+1] are exactly its R_i rows inside the output block, and the slot names a pool
// row.  The rows kernels and ss_stream_advance_packed both decide by this one function which entries they skip.
struct StreamEntry {
    long long s0, r0;
    unsigned n, R, slot;
    bool ok;
};
__device__ __forceinline__ StreamEntry stream_entry(const FrameStreamPackedArgs &v, unsigned i)
{
    StreamEntry e;
    e.s0 = v.so[i];
    e.r0 = v.ro[i];
    const long long s1 = v.so[i + 1], r1 = v.ro[i + 1];
    const int slot = v.slots[i];
    const bool len_ok = e.s0 >= 0 && s1 >= e.s0 && s1 - e.s0 <= 0x7fffffffll;
    e.n = len_ok ? static_cast<unsigned>(s1 - e.s0) : 0u;
    e.R = e.n / v.step;
    e.slot = static_cast<unsigned>(slot);
    e.ok = len_ok && e.R * v.step == e.n && e.r0 >= 0 && r1 >= e.r0 && r1 - e.r0 == static_cast<long long>(e.R) &&
           r1 <= static_cast<long long>(v.total_rows) && slot >= 0 && e.slot < v.pool_streams;
    return e;
}
// One pass over the entries, spread over the grid (see varlen_check_clips).  A vector store to the pinned word.
__device__ __forceinline__ void stream_check_entries(const FrameStreamPackedArgs &v, unsigned tid, unsigned nthreads)
{
    bool bad = false;
    for (unsigned i = tid; i < v.n_active; i += nthreads) bad |= !stream_entry(v, i).ok;
    if (bad && v.err) __hip_atomic_store(v.err, kVarlenError, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
// the ragged streaming build of ss_front_generic's MFCC / mfe path: a as for launch_front_generic_frame_stream with x = the packed
// chunks; batch / n_samples / n_frames / ld are unused.  The grid comes from s.total_rows (one workgroup where it is 0: the entry pass).
hipError_t launch_front_generic_frame_stream_packed(const FrontArgs &a, const FrameStreamPackedArgs &s, uint32_t log2c, hipStream_t stream,
                                                    int num_cus, LaunchInfo *info);
// The pool's state advance, a second stream-ordered launch behind the rows: for every ok entry with n_i > 0, pool row slots[i] := the
// last S samples of (old row ++ the entry's chunk), in place (ss_stream_advance's discipline).  Grid-stride over the entries.
hipError_t launch_stream_advance_packed(const FrameStreamPackedArgs &s, const float *x, hipStream_t stream);

// The same pool fed signed 16-bit PCM (ss_mfcc_stream_packed_i16_device / ss_mfe_stream_packed_i16_device): chunk sample k of the
// call is (float)x[k] * scale, scale a power of two (the product is exact, so contracting it into what follows changes no bit).
// The entry block is the float pool's, so that stream_entry(), stream_check_entries() and the lookups over its tables serve both;
// the type of its own selects the PCM builds in the kernels' trailing argument packs (FrontArgs::x / Fast512Args::x are unused
// there).  Offsets stay in samples.  x is 4-byte aligned where the headline build runs (a sample pair is one dword: every so[i] is
// a multiple of the even step); the generic build and the advance read single samples.
struct FrameStreamPackedPcmArgs {
    FrameStreamPackedArgs e;
    const int16_t *x;  // the packed chunks
    float scale;
};
// sample k of a PCM buffer
__device__ __forceinline__ float pcm_sample(const int16_t *x, long long k, float scale) { return static_cast<float>(x[k]) * scale; }
// the two samples of a PCM dword: sign-extended, converted, times the power-of-two scale (exact: the bits the float loader finds in
// the converted buffer)
__device__ __forceinline__ float2 pcm_pair(int w, float scale)
{
    return make_float2(static_cast<float>(static_cast<int16_t>(w)) * scale, static_cast<float>(w >> 16) * scale);
}
// The raw dword of a PCM sample pair: two int16, fetched by one 32-bit load at 2-byte alignment (a pair may start at an odd sample:
// odd ld, odd base, odd clip offset).  gfx950 global loads take any alignment in the unaligned access mode the HSA ABI sets -- the
// mode the float builds' 8-byte pair loads at dword alignment already rely on -- so one load serves either parity.
__device__ __forceinline__ float pcm_raw_pair(const void *p)
{
    int w;
    __builtin_memcpy(&w, __builtin_assume_aligned(p, 2), sizeof w);
    return __int_as_float(w);
}
// a as for launch_front_generic_frame_stream_packed (a.x unused)
hipError_t launch_front_generic_frame_stream_packed(const FrontArgs &a, const FrameStreamPackedPcmArgs &s, uint32_t log2c, hipStream_t stream,
                                                    int num_cus, LaunchInfo *info);
// ss_stream_advance_packed with the chunk read as PCM: the pool rows end up holding the floats the float call would have stored
hipError_t launch_stream_advance_packed(const FrameStreamPackedPcmArgs &s, hipStream_t stream);

// The one-shot calls fed signed 16-bit PCM (ss_mfcc_batch_i16_device / ss_mfe_batch_i16_device / ss_mfcc_packed_i16_device /
// ss_mfe_packed_i16_device): sample k is (float)x[k] * scale, scale a power of two (the product is exact).  Trailing argument packs
// of the kernels' PCM builds, as FrameStreamPackedPcmArgs is; FrontArgs::x / Fast512Args::x are unused there.  ld and the offsets
// stay in samples; x needs 2-byte alignment only (the generic builds read single samples, the headline builds read a sample pair as
// one dword at 2-byte alignment).
struct BatchPcmArgs {  // equal-length clips: clip b starts at x + b * ld
    const int16_t *x;
    float scale;
};
struct VarlenPcmArgs {  // packed clips: the float layout's tables (varlen_clip(), varlen_check_clips() serve both)
    VarlenArgs v;
    const int16_t *x;
    float scale;
};
// a as for launch_front_generic / launch_front_generic_varlen (a.x unused); MFCC / mfe / power outputs as the float layouts
hipError_t launch_front_generic(const FrontArgs &a, const BatchPcmArgs &p, uint32_t log2c, hipStream_t stream, int num_cus, LaunchInfo *info,
                                const DbArgs *db = nullptr);
hipError_t launch_front_generic_varlen(const FrontArgs &a, const VarlenPcmArgs &v, uint32_t log2c, hipStream_t stream, int num_cus,
                                       LaunchInfo *info);
// The fallback of the equal-length PCM calls whose kernel has no PCM build (both packed kernels have one): dst[r * ld + k] = (float)src[r * ld + k] * scale for k < n, r < rows
// (the gaps between rows are left alone).  Grid-stride, plain vector loads and stores.
hipError_t launch_pcm_to_float(const int16_t *src, float *dst, size_t rows, size_t n, size_t ld, float scale, hipStream_t stream);

// Ragged streaming STFT / mel spectrogram over a pool of stream states (ss_mel_spectrogram_stream_packed_device /
// ss_stft_stream_packed_device): the same tables on the STFT path, continuous mode.  The entry block is the frame pool's, with
// step = hop, state_len = fft_points - hop and lead unused, so that stream_entry(), stream_check_entries(), the lookups over its tables and
// ss_stream_advance_packed ("last S samples of old row ++ chunk": the dense continuous advance) serve both families; the type of
// its own only selects the STFT-path builds in the kernels' trailing argument packs.  Row t of an entry is row t of a dense
// continuous call on that stream alone (StreamArgs above): its window is the W samples that end at chunk sample (t + 1) * hop, and
// sample p < 0 is pool[slots[i] * S + S + p].
struct StftStreamPackedArgs {
    FrameStreamPackedArgs e;
};
// the ragged streaming build of ss_front_generic's STFT / mel path (any fft_points, chirp-z included; mel and stft output): a as
// for launch_front_generic_stream with x = the packed chunks and n_pad = 0; batch / n_samples / rows / real_rows / ld are unused.
// The grid comes from s.e.total_rows (one workgroup where it is 0: the entry pass).
hipError_t launch_front_generic_stream_packed(const FrontArgs &a, const StftStreamPackedArgs &s, uint32_t log2c, hipStream_t stream,
                                              int num_cus, LaunchInfo *info);

// The STFT path fed signed 16-bit PCM (the ss_mel_spectrogram*_i16* / ss_stft*_i16* entry points): a BatchPcmArgs behind the layout's
// own argument in the kernels' trailing packs selects the PCM loader -- alone (equal-length clips: launch_front_generic above with
// out_kind OUT_MEL / OUT_STFT), behind a VarRowsArgs (packed clips) or behind a StftStreamPackedArgs (the pool: chunk samples are
// PCM, the pool rows stay float; launch_stream_advance_packed(FrameStreamPackedPcmArgs) moves them on).  The tables, the offsets
// (in samples) and every check are the float layouts'; a.x is unused.  Reported as ss_front_generic_varrowsi / _streampi.
hipError_t launch_front_generic_varrows(const FrontArgs &a, const VarRowsArgs &v, const BatchPcmArgs &p, uint32_t log2c, hipStream_t stream,
                                        int num_cus, LaunchInfo *info, const DbArgs *db = nullptr);
hipError_t launch_front_generic_stream_packed(const FrontArgs &a, const StftStreamPackedArgs &s, const BatchPcmArgs &p, uint32_t log2c,
                                              hipStream_t stream, int num_cus, LaunchInfo *info);
#if SS_LAB
// Test aid (lab library): every word of every CU's LDS := 0xFFFFFFFF (ss_debug_poison_lds).
hipError_t launch_poison_lds(hipStream_t stream, int num_cus);
#endif
// Element-wise pre-emphasis (processing.rs:31-53).
hipError_t launch_preemphasis(const float *x, float *y, size_t n, size_t shift, float cof, hipStream_t stream);

// Arguments of the fft_points = 512 MFCC kernel (ss_mfcc512.hip).
struct Fast512Args {
    const float *x;
    unsigned long long ld;
    uint32_t n_samples, batch, flen, step, n_frames;
    float scale;
    int32_t spectrum_exponent;
    // one table block, copied verbatim into LDS (layout: ss::fast512_layout in ss_internal.h):
    //   tw2   [15][16] float2  exp(-2 pi i j r / 256), r = 1..15
    //   twn   [8][16]  float2  exp(-2 pi i (j + 16 r) / 512)
    //   cos   [16][52]         row c: cos(pi c (2 m_q + 1) / 2M) for q = slot*16 + lane < 48 (0 for unused q / c >= n_ceps)
    //   start [3][16]  int32   first P bin of the filter owned by (slot, lane)
    //   filt  [3][16]  int32   its filter index (-1: none)
    //   melw  [16][mel_wpitch] lane row: taps of slot 0, 1, 2, each zero-padded to a multiple of 4
    const float *tab;
    int32_t mel_wpitch;  // floats per lane row = 4 * (mel_q4[0] + mel_q4[1] + mel_q4[2])
    int32_t mel_q4[3];   // taps / 4 per slot (lock-step loop lengths)
    uint32_t n_filters, n_ceps;
    float dct_scale_k, dct_scale_0, dct_scale_00;
    int32_t dc_elimination;
    float *out;          // MFCC [frames x n_ceps], or (out_mfe) mel energies [frames x n_filters]
    float *out_energy;   // out_mfe: frame energies [frames] (feature.rs:216-219)
    int32_t out_mfe;     // 1: stop after the mel stage and write mfe's (features, energy) (feature.rs:200-233);
                         // 2: stop after the spectrum and write power_spectrum's rows [frames x 257] (processing.rs:179-181)
    // optional front end (the switches of ss_params; default off, as in the reference's mfcc):
    int32_t win_floats;     // > 0: frame window [flen] behind the mel rows of the table block
    float preemph;          // != 0: y[n] = x[n] - preemph * x[(n - preemph_shift) mod n_samples] (processing.rs:31-53) on load
    uint32_t preemph_shift;
    // librosa-compatible variants (ss_params.framing = SS_FRAMING_CENTER, banks that cover the whole spectrum)
    int32_t center;         // frame t covers x[t*step - flen/2 : t*step + flen/2); flen % 4 == 0
    int32_t pad_reflect;    // center: np.pad 'reflect' outside the clip (else zeros)
    int32_t fullp;          // the table block was built for P rows of all 257 bins
    int32_t paired;         // 40 filters: filter m in slot 2 and 39 - m in slot 0 of one lane, (16 + i, 23 - i) in lanes 2i, 2i + 1 of slot 1;
                            // 2: and the filters of slots 1 / 2 lie inside the slots' first 6 / 2 taps
    unsigned long long *dbg;  // diagnostic runs only: per-wave realtime stamps, or null
    // filled by launch_mfcc_c256: floor(x / n_frames) = umulhi(x, nf_magic) >> nf_shift for x < 2^31 (nf_magic = 0: divide)
    uint32_t nf_magic, nf_shift;
    // filled by launch_mfcc_c256: workgroup b owns quads [b * q_base + min(b, q_rem), + q_base + (b < q_rem)) -- the balanced
    // contiguous split without a division in the kernel's prologue (everything in front of the first loads is start-up latency)
    uint32_t q_base, q_rem;
};

hipError_t launch_mfcc_c256(const Fast512Args &a, hipStream_t stream, int num_cus, LaunchInfo *info);

// Several independent batches in ONE launch (ss_mfcc_batches_device / ss_mel_spectrogram_batches_device): the second argument of
// the kernel builds that take a batch table (MULTI).  Batch b has its own input block x[b] (clips of a.n_samples at row stride
// a.ld) and output block out[b]; its work units -- frame quads (512-point MFCC), frames (4096-point MFCC), row pairs (2048-point
// mel) -- are [uend[b-1], uend[b]) of the launch's unit range (entries past the last batch: 0xffffffff); total[b] = its clips *
// n_frames (the 512-point kernel's last quad of a batch may be partly filled).  Filled by the launch_*_multi functions.
constexpr int kMaxLaunchBatches = 8;
struct BatchTable {
    const float *x[kMaxLaunchBatches];
    float *out[kMaxLaunchBatches];
    uint32_t uend[kMaxLaunchBatches];
    uint32_t total[kMaxLaunchBatches];
};
using Fast512Multi = BatchTable;
// second kernel argument: the batch table of a MULTI build, nothing otherwise
template <bool MULTI>
struct MultiArg {
};
template <>
struct MultiArg<true> {
    BatchTable m;
};
// a: the argument block of one batch (x / out / batch are ignored); d_x / d_out / clips: n_batches <= kMaxLaunchBatches entries.
// hipErrorInvalidValue before the launch: the configuration has no multi-batch build (the caller launches batch by batch).
hipError_t launch_mfcc_c256_multi(const Fast512Args &a, int n_batches, const float *const *d_x, float *const *d_out, const size_t *clips,
                                  hipStream_t stream, int num_cus, LaunchInfo *info);
// Packed variable-length clips on the headline build (MFCC, default frame shape and bank, contract framing, reference DCT): one launch
// over the packed output rows (VarlenArgs, declared below).  hipErrorInvalidValue before the launch for every other configuration.
struct VarlenArgs;
hipError_t launch_mfcc_c256_varlen(const Fast512Args &a, const VarlenArgs &v, hipStream_t stream, int num_cus, LaunchInfo *info);
// Streaming MFCC / mfe on the headline build (FrameStreamArgs, declared above): a as for launch_mfcc_c256 with batch = streams,
// n_frames = rows per stream, n_samples = the chunk; MFCC of the default frame shape and bank (40 filters, paired tight-tap layout)
// or mfe of the default bank, no window, no pre-emphasis, reference DCT scales with dct_scale_00 = dct_scale_0.
// hipErrorInvalidValue before the launch for every other configuration.
hipError_t launch_mfcc_c256_stream(const Fast512Args &a, const FrameStreamArgs &s, hipStream_t stream, int num_cus, LaunchInfo *info);
// Ragged streaming MFCC / mfe on the headline build (FrameStreamPackedArgs, declared above): the shapes launch_mfcc_c256_stream
// serves, with a.x = the packed chunks (batch / n_samples / n_frames / ld unused) and the quad range over s.total_rows.
// hipErrorInvalidValue before the launch for every other configuration.
hipError_t launch_mfcc_c256_stream_packed(const Fast512Args &a, const FrameStreamPackedArgs &s, hipStream_t stream, int num_cus,
                                          LaunchInfo *info);
// the same shapes fed 16-bit PCM (FrameStreamPackedPcmArgs, declared above; a.x unused), reported as ss_mfcc_c256spi<...>; s.x not
// 4-byte aligned is hipErrorInvalidValue too
hipError_t launch_mfcc_c256_stream_packed(const Fast512Args &a, const FrameStreamPackedPcmArgs &s, hipStream_t stream, int num_cus,
                                          LaunchInfo *info);
// launch_mfcc_c256 / launch_mfcc_c256_varlen fed 16-bit PCM (BatchPcmArgs / VarlenPcmArgs, declared above; a.x unused), reported as
// ss_mfcc_c256i<...> / ss_mfcc_c256vi<...>.  The equal-length PCM builds: what launch_mfcc_c256 serves with contract framing and no
// fused pre-emphasis (MFCC, mfe, the optional window; every frame length, an odd one's half pair included); the varlen PCM build:
// what launch_mfcc_c256_varlen serves.  hipErrorInvalidValue before the launch for every other configuration.
hipError_t launch_mfcc_c256(const Fast512Args &a, const BatchPcmArgs &p, hipStream_t stream, int num_cus, LaunchInfo *info);
hipError_t launch_mfcc_c256_varlen(const Fast512Args &a, const VarlenPcmArgs &v, hipStream_t stream, int num_cus, LaunchInfo *info);
// whether the kernel has an mfe-output / windowed / pre-emphasised build for this shape (the default bank at flen 320)
bool mfcc_c256_has_mfe(const Fast512Args &a);

// Arguments of the fft_points = 2048 mel-spectrogram kernel (ss_mel2048.hip).
struct Mel2048Args {
    const float *x;
    unsigned long long ld;
    uint32_t n_samples, batch;
    uint32_t hop, n_pad, rows, real_rows;
    float scale;  // wnorm (config.rs:178)
    // one table block, copied verbatim into LDS (layout: ss::mel2048_layout in ss_internal.h)
    const float *tab;
    int32_t mel_wpitch;  // floats per lane weight row
    int32_t mel_q4[4];   // taps / 4 per slot
    uint32_t n_filters;
    float *out;       // [batch][n_filters][rows], or (out_stft) [batch][rows][1025][2]
    int32_t out_stft; // 1: write the scaled complex spectrum stft2 returns (functions.rs:86-123) instead of the mel rows
    int32_t fullp;    // the bank reaches past (F+1)/2: P rows hold every bin (not in the 4096-point kernel)
    // whole-line tile build (ss_mel_c1024<tile>): device view of the config's pinned error word, or null -- a wave sets it
    // when a tile hand-off never came (the host turns it into SS_ERR_DEVICE).  Touched on the cold path only; how long a wave
    // polls before it gives up is the word behind the table block.
    unsigned *ctl;
    // twelve-wave builds, diagnostic (ss_mel_spectrogram_timed_region): two words per wave -- shader cycles lived, 100 MHz ticks
    // lived -- or null
    unsigned long long *stamps;
};

hipError_t launch_mel_c1024(const Mel2048Args &a, hipStream_t stream, int num_cus, LaunchInfo *info, const DbArgs *db = nullptr);
// (db, here and on the three launchers of the dense and the packed layout below: the dB build of the twelve-wave mel kernel where the
// call runs that kernel -- info->db_fused says so; the eight-wave builds have no dB build and run as they are)
// the streaming builds (mel output; StreamArgs above), chosen between eight and twelve waves by launch_mel_c1024's rule;
// hipErrorInvalidValue before the launch for stft output or a shape that does not fit
hipError_t launch_mel_c1024_stream(const Mel2048Args &a, const StreamArgs &s, hipStream_t stream, int num_cus, LaunchInfo *info);
// packed variable-length clips (VarRowsArgs above) on the twelve-wave mel build, whatever the unit count (a clip's bits must not
// depend on the clips beside it); a: x / out = the packed blocks, batch / n_samples / rows / real_rows unused.  hipErrorInvalidValue
// before the launch for stft output, a bank that reaches past (F+1)/2 (fullp) or a shape that does not fit
hipError_t launch_mel_c1024_varlen(const Mel2048Args &a, const VarRowsArgs &v, hipStream_t stream, int num_cus, LaunchInfo *info,
                                   const DbArgs *db = nullptr);
// ragged streaming over a pool of stream states (StftStreamPackedArgs above) on the twelve-wave mel build, whatever the unit count
// (an entry's bits must not depend on the entries beside it); a: x / out = the packed blocks, n_pad = 0, batch / n_samples / rows /
// real_rows unused.  hipErrorInvalidValue before the launch for stft output, a bank that reaches past (F+1)/2 (fullp) or a shape
// that does not fit
hipError_t launch_mel_c1024_stream_packed(const Mel2048Args &a, const StftStreamPackedArgs &s, hipStream_t stream, int num_cus,
                                          LaunchInfo *info);
// several blocks of channels in one launch of the twelve-wave mel build (a: one block's arguments; x / out / batch are ignored);
// hipErrorInvalidValue before the launch where the shape has no batch-table build
hipError_t launch_mel_c1024_multi(const Mel2048Args &a, int n_batches, const float *const *d_x, float *const *d_out, const size_t *channels,
                                  hipStream_t stream, int num_cus, LaunchInfo *info);
// The three twelve-wave mel layouts fed 16-bit PCM (BatchPcmArgs above; a.x unused), reported as ss_mel_c1024i<w12,...> /
// ss_mel_c1024vi<...> / ss_mel_c1024spi<...>: a lane's sample pair is one dword of two int16, loaded at 2-byte alignment (ld, base and
// offsets of either parity).  The equal-length form serves exactly the calls launch_mel_c1024 gives the twelve-wave mel build (the
// same rule, so the bits are the float call's); hipErrorInvalidValue before the launch for every other call -- eight waves, stft
// output, fullp -- which the caller runs on the float build behind a conversion.
hipError_t launch_mel_c1024(const Mel2048Args &a, const BatchPcmArgs &p, hipStream_t stream, int num_cus, LaunchInfo *info,
                            const DbArgs *db = nullptr);
hipError_t launch_mel_c1024_varlen(const Mel2048Args &a, const VarRowsArgs &v, const BatchPcmArgs &p, hipStream_t stream, int num_cus,
                                   LaunchInfo *info, const DbArgs *db = nullptr);
hipError_t launch_mel_c1024_stream_packed(const Mel2048Args &a, const StftStreamPackedArgs &s, const BatchPcmArgs &p, hipStream_t stream,
                                          int num_cus, LaunchInfo *info);
#if SS_LAB
// the retired whole-line-tile build (tools/experiments/ss_mel2048_tile.hip, linked into the lab library only);
// hipErrorInvalidValue where the shape has no tile build
hipError_t launch_mel_c1024_tile(const Mel2048Args &a, hipStream_t stream, int num_cus, LaunchInfo *info);
#endif
// fft_points = 1024 mel-spectrogram kernel (ss_mfcc1024.hip): same argument block, table layout ss::mfcc1024_layout
hipError_t launch_mel_c512(const Mel2048Args &a, hipStream_t stream, int num_cus, LaunchInfo *info);
// fft_points = 4096 mel-spectrogram kernel (ss_mfcc4096.hip): same argument block, table layout ss::mfcc4096_layout
// without cosine rows, Vorbis window [4096] behind the mel rows
hipError_t launch_mel_c2048(const Mel2048Args &a, hipStream_t stream, int num_cus, LaunchInfo *info);

// Arguments of the fft_points = 512 mel-spectrogram kernel (ss_mel512.hip).
struct Mel512Args {
    const float *x;
    unsigned long long ld;
    uint32_t n_samples, batch;
    uint32_t hop, n_pad, rows, real_rows;
    float scale;  // wnorm (config.rs:178)
    const float *tab;    // table block (layout: ss::mel512_layout in ss_internal.h), copied verbatim into LDS
    int32_t mel_wpitch;  // floats per lane weight row
    int32_t mel_q4[5];   // taps / 4 per slot
    int32_t fullp;       // the bank reaches past bin 128: P rows hold all 257 bins
    uint32_t n_filters;
    float *out;          // [batch][n_filters][rows], or (out_stft) [batch][rows][257][2]
    int32_t out_stft;    // 1: write the scaled complex spectrum stft2 returns (functions.rs:86-123) instead of the mel rows
};

hipError_t launch_mel_c256(const Mel512Args &a, hipStream_t stream, int num_cus, LaunchInfo *info);

// Arguments of the fft_points = 2048 MFCC / mfe kernel (ss_mfcc2048.hip).
struct Mfcc2048Args {
    const float *x;
    unsigned long long ld;
    uint32_t n_samples, batch, flen, step, n_frames;
    float scale;  // 1/N (processing.rs:180)
    int32_t spectrum_exponent;
    const float *tab;    // table block (layout: ss::mfcc2048_layout in ss_internal.h), copied verbatim into LDS
    int32_t mel_wpitch;  // floats per lane weight row
    int32_t mel_q4[4];   // taps / 4 per slot
    uint32_t n_filters, n_ceps;
    float dct_scale_k, dct_scale_0, dct_scale_00;
    int32_t dc_elimination;
    int32_t windowed;    // the table block carries a frame window (mfcc_window switch)
    int32_t out_mfe;     // 1: write mfe's (features, energy) instead of the cepstra
    int32_t center;      // librosa center=True framing
    int32_t pad_reflect; // np.pad 'reflect' (else zeros) outside the clip for centred frames
    int32_t fullp;       // the bank reaches past the reference's (F+1)/2: P rows hold every bin up to fft_points/2
    float preemph;       // fused pre-emphasis coefficient (0 = off) and shift (processing.rs:31-53)
    uint32_t preemph_shift;
    float *out;
    float *out_energy;
};

hipError_t launch_mfcc_c1024(const Mfcc2048Args &a, hipStream_t stream, int num_cus, LaunchInfo *info);

// fft_points = 1024 MFCC / mfe kernel (ss_mfcc1024.hip): same argument block, table layout ss::mfcc1024_layout
using Mfcc1024Args = Mfcc2048Args;
hipError_t launch_mfcc_c512(const Mfcc1024Args &a, hipStream_t stream, int num_cus, LaunchInfo *info);

// Arguments of the fft_points = 256 MFCC / mfe kernel (ss_mfcc256.hip): two frames per 256-point complex transform.
struct Mfcc256Args {
    const float *x;
    unsigned long long ld;
    uint32_t n_samples, batch, flen, step, n_frames;
    float scale;  // 1/N (processing.rs:180)
    int32_t spectrum_exponent;
    const float *tab;    // table block (layout: ss::mfcc256_layout in ss_internal.h), copied verbatim into LDS
    int32_t mel_wpitch;  // floats per lane weight row
    int32_t mel_q4[5];   // taps / 4 per slot (three slots in the 256-point kernel, five in the wide-bank 512-point one)
    uint32_t n_filters, n_ceps;
    float dct_scale_k, dct_scale_0, dct_scale_00;
    int32_t dc_elimination;
    int32_t windowed;    // the table block carries a frame window (mfcc_window switch)
    int32_t out_mfe;     // 1: write mfe's (features, energy) instead of the cepstra
    int32_t center;      // wide-bank 512-point kernel only: librosa center=True framing (flen % 4 == 0)
    int32_t pad_reflect; // np.pad 'reflect' (else zeros) outside the clip for centred frames
    float preemph;       // fused pre-emphasis coefficient (0 = off) and shift (processing.rs:31-53)
    uint32_t preemph_shift;
    uint32_t nf_magic, nf_shift;  // set by the launcher: frame -> (clip, t) by multiply-high
    float *out;
    float *out_energy;
};

hipError_t launch_mfcc_c256x2(const Mfcc256Args &a, hipStream_t stream, int num_cus, LaunchInfo *info);
// fft_points = 512 MFCC / mfe with up to 80 filters (ss_mfcc512w.hip): same argument block, table layout ss::mfcc512w_layout
hipError_t launch_mfcc_c256w(const Mfcc256Args &a, hipStream_t stream, int num_cus, LaunchInfo *info);

// Arguments of the fft_points = 4096 MFCC kernel (ss_mfcc4096.hip).
struct Mfcc4096Args {
    const float *x;
    unsigned long long ld;
    uint32_t n_samples, batch, flen, step, n_frames;
    float scale;  // 1/N (processing.rs:180)
    int32_t spectrum_exponent;
    const float *tab;    // table block (layout: ss::mfcc4096_layout in ss_internal.h), copied verbatim into LDS
    int32_t mel_wpitch;  // floats per lane weight row
    int32_t mel_q4[4];   // taps / 4 per slot
    int32_t cos_floats;  // floats of the cosine block in front of the mel rows
    int32_t dct_fold2;   // 1: per-lane cosine rows of the twice-folded DCT (n_filters % 4 == 0, n_ceps <= 43)
    uint32_t n_filters, n_ceps;
    float dct_scale_k, dct_scale_0, dct_scale_00;
    int32_t dc_elimination;
    float preemph;       // fused pre-emphasis coefficient (0 = off) and shift (processing.rs:31-53)
    uint32_t preemph_shift;
    float *out;          // MFCC [frames x n_ceps], or (out_mfe) mel energies [frames x n_filters]
    float *out_energy;   // out_mfe: frame energies [frames]
    int32_t out_mfe;     // 1: stop after the mel stage and write mfe's (features, energy) (feature.rs:200-233)
    const float *window; // optional frame window [flen] in device memory (mfcc_window switch), or null
    float *dbg;  // diagnostic (SS_DEBUG_ROWS): frame 0's P row [1028] + ln(mel) row [256], or null
    // twelve-wave default-shape build, diagnostic (ss_mfcc_timed_region): two words per wave -- shader cycles lived, 100 MHz ticks
    // lived -- or null
    unsigned long long *stamps;
};

hipError_t launch_mfcc_c2048(const Mfcc4096Args &a, hipStream_t stream, int num_cus, LaunchInfo *info);
// several batches in one launch of the twelve-wave default-shape build (see launch_mfcc_c256_multi)
hipError_t launch_mfcc_c2048_multi(const Mfcc4096Args &a, int n_batches, const float *const *d_x, float *const *d_out, const size_t *clips,
                                   hipStream_t stream, int num_cus, LaunchInfo *info);

// Arguments of the Kaldi-compatible 512-point fbank / MFCC kernel (ss_kaldi512.hip; the specification is the ss_kaldi_* comment of
// include/speechsauce_amd.h).
struct KaldiArgs {
    const float *x;
    unsigned long long ld;
    uint32_t n_samples, batch, flen, step, n_frames;
    const float *tab;    // table block (ss::KaldiTables: mfcc512w_layout + the frame window [512]), copied verbatim into LDS
    int32_t mel_wpitch;  // floats per lane weight row
    int32_t mel_q4[5];   // taps / 4 per slot
    uint32_t n_filters, n_ceps;
    float input_scale;   // step 1 (1: skipped)
    float preemph;       // step 4 (0: skipped)
    float flen_f;        // the divisor of the frame mean
    float log_floor;     // ln(energy_floor), -inf where energy_floor == 0
    int32_t remove_dc, raw_energy, use_energy;
    int32_t out_mfcc;    // 0: fbank rows [frames x n_filters] (+ out_energy where non-null); 1: cepstra [frames x n_ceps]
    int32_t use_power;
    float *out;
    float *out_energy;   // fbank builds: log energy [frames], or null
    uint32_t nf_magic, nf_shift;  // set by the launcher: frame -> (clip, t) by multiply-high
};
// Packed clips of the Kaldi kernel: VarlenArgs' layout with Kaldi's frame count (1 + (L - flen) / shift in integers).
struct KaldiVarlenArgs {
    const long long *so;  // [n_clips + 1] sample offsets
    const long long *fo;  // [n_clips + 1] frame (output row) offsets
    unsigned long long total_frames;
    uint32_t n_clips;
    unsigned *err;        // the handle's device error word (set to kVarlenError on a bad clip)
};
hipError_t launch_kaldi_c256(const KaldiArgs &a, hipStream_t stream, int num_cus, LaunchInfo *info);
// a: x / out = the packed blocks; batch / n_samples / n_frames / ld are unused
hipError_t launch_kaldi_c256_varlen(const KaldiArgs &a, const KaldiVarlenArgs &v, hipStream_t stream, int num_cus, LaunchInfo *info);
// The same two calls fed signed 16-bit PCM (ss_kpcm_*): sample k is (float)x[k] * scale, scale a power of two (the product is
// exact).  Trailing argument packs of the kernel's PCM builds, as BatchPcmArgs / VarlenPcmArgs are for the generic kernel; a.x is
// unused, and the packed pack carries the float layout's tables (kaldi_clip(), row_owner() and the error pass serve both: the
// kernel's own KaldiVarlenArgs argument stays empty).  ld and the offsets stay in samples; x needs 2-byte alignment only.
struct KaldiPcmArgs {
    const int16_t *x;
    float scale;
};
struct KaldiVarlenPcmArgs {
    KaldiVarlenArgs v;
    const int16_t *x;
    float scale;
};
hipError_t launch_kaldi_c256(const KaldiArgs &a, const KaldiPcmArgs &p, hipStream_t stream, int num_cus, LaunchInfo *info);
hipError_t launch_kaldi_c256_varlen(const KaldiArgs &a, const KaldiVarlenPcmArgs &v, hipStream_t stream, int num_cus, LaunchInfo *info);
// The stream-pool builds (ss_kaldi512_pool.hip; ss_kstream_*_packed*_device): the packed output rows of a ragged streaming launch
// over the frame pool's entry block -- step = the frame shift, state_len = S = D * shift, D = ceil(flen / shift) - 1; lead unused:
// row t of an entry starts at chunk sample t * step - S.  pcm: the chunks are sp.x (2-byte aligned) times sp.scale, else a.x
// (sp.x / sp.scale unused); batch / n_samples / n_frames / ld are unused.  The grid comes from total_rows (one workgroup where it
// is 0: the entry pass).  The advance is launch_stream_advance_packed over the same block.
hipError_t launch_kaldi_c256_stream_packed(const KaldiArgs &a, const FrameStreamPackedPcmArgs &sp, bool pcm, hipStream_t stream, int num_cus,
                                           LaunchInfo *info);

// Arguments of the NeMo / Parakeet log-mel kernels (ss_nemo512.hip; the specification is the ss_nemo_* comment of
// include/speechsauce_amd.h).
struct NemoArgs {
    const float *x;
    unsigned long long ld;
    uint32_t n_samples, batch, n_frames;  // equal-length clips: n_frames = n_samples / 160 rows each
    uint32_t win_len;    // W: live samples per frame (even); frame t starts at clip sample 160 t - W / 2
    const float *tab;    // table block (ss::NemoTables, nemo512_layout), copied verbatim into LDS
    int32_t mel_wpitch;  // floats per lane weight row
    int32_t mel_q4[8];   // taps / 4 per slot
    uint32_t n_mels;
    float preemph;       // step 2 (0: skipped)
    float log_guard;     // step 6
    float norm_eps;      // step 8
    float *out;          // [rows x n_mels]
    uint32_t nf_magic, nf_shift;  // set by the launcher: frame -> (clip, t) by multiply-high
};
// Packed clips: KaldiVarlenArgs' layout with T = len / 160; a clip without rows is consistent.
struct NemoVarlenArgs {
    const long long *so;  // [n_clips + 1] sample offsets
    const long long *fo;  // [n_clips + 1] frame (output row) offsets
    unsigned long long total_frames;
    uint32_t n_clips;
    unsigned *err;        // the handle's device error word (set to kVarlenError on a bad clip)
};
hipError_t launch_nemo_c256(const NemoArgs &a, hipStream_t stream, int num_cus, LaunchInfo *info);
// a: x / out = the packed blocks; batch / n_samples / n_frames / ld are unused
hipError_t launch_nemo_c256_varlen(const NemoArgs &a, const NemoVarlenArgs &v, hipStream_t stream, int num_cus, LaunchInfo *info);
// step 8 in place on a.out: the rows of a.batch clips of a.n_frames rows, or (v non-null) of the packed clips, a bad one skipped.
// The grid depends on the clip count and n_mels only.
hipError_t launch_nemo_norm(const NemoArgs &a, const NemoVarlenArgs *v, hipStream_t stream);
// The stream-pool builds (ss_nemo512_pool.hip; ss_nstream_log_mel_packed*_device): the packed output rows of a ragged streaming launch
// over the frame pool's entry block -- step = 160, state_len = S = 160 L + W / 2 + 1 with L = ceil(W / 320) - 1, lead = S - 1: row t
// of an entry starts at chunk sample 160 t - lead, and its pre-emphasis predecessor is the sample in front of that.  pcm: the chunks
// are sp.x (2-byte aligned) times sp.scale, else a.x (sp.x / sp.scale unused); batch / n_samples / n_frames / ld are unused.  The
// grid comes from total_rows (one workgroup where it is 0: the entry pass).  The advance is launch_stream_advance_packed over the
// same block.
hipError_t launch_nemo_c256_stream_packed(const NemoArgs &a, const FrameStreamPackedPcmArgs &sp, bool pcm, hipStream_t stream, int num_cus,
                                          LaunchInfo *info);
// The flush (ss_nstream_flush_device): row i * delay + u of a.out is row u of the stream whose state is pool row slots[i], the frame
// that starts 160 (u - delay) - W / 2 from the stream's end; an entry whose slot lies outside the pool is skipped.
struct NemoFlushArgs {
    float *pool;           // [pool_streams][state_len]
    uint32_t state_len;    // S
    uint32_t delay;        // L: rows per entry
    const int32_t *slots;  // [n_active]
    uint32_t n_active;
    uint32_t pool_streams;
    unsigned *err;         // the handle's device error word (set to kVarlenError on a bad entry)
};
// Two launches: the n_active * delay rows (none where delay == 0), then the zeroing of the named pool rows, which also reports a bad
// entry.  The grids depend on n_active and delay only.
hipError_t launch_nemo_c256_flush(const NemoArgs &a, const NemoFlushArgs &s, hipStream_t stream, int num_cus, LaunchInfo *info);

// The fused splice + affine transform of packed rows (ss_affine.hip; ss_affine_splice_packed*): out[g] = M * (spliced row g) + bias
// on the f32 matrix instruction.  x / ro and out / oo are the two packed blocks and their tables as ss_splice_packed_device takes
// them (total_rows, total_out_rows, n_clips < 2^31).  table: the handle's device block -- the bias padded with zeros to bias_len =
// 16 * (feature tiles) floats, then the matrix in operand order [feature tile][group][lane][4]: steps = ceil(in_dim / 4) k-steps in
// groups = ceil(steps / 4) groups of four, a lane's four values of a group side by side.
struct AffineArgs {
    const float *x;
    const long long *ro, *oo;
    const float *table;
    float *out;
    unsigned long long total_rows, total_out_rows;
    uint32_t n_clips;
    uint32_t cols, left, stride;
    uint32_t width;             // left + 1 + right
    uint32_t step_c, step_col;  // n / cols, n % cols: how (context row, column) moves on by n elements (vec4: 16, else 4)
    uint32_t steps, groups, bias_len, out_dim;
    int32_t vec4;               // cols % 4 == 0 and x is 16-byte aligned: a lane loads four elements of a spliced row at once
    int32_t store16;            // out_dim % 4 == 0 and out is 16-byte aligned: a lane's four features go out as one store
};
// one launch; the grid depends on total_out_rows, out_dim and in_dim only
hipError_t launch_affine_splice(const AffineArgs &a, hipStream_t stream);

}  // namespace ss
