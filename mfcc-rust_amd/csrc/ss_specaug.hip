// SpecAugment time / frequency masking of packed rows, seeded on the device: ss_specaug_* and ss_mask_spans_* of
// include/speechsauce_amd.h, whose comment is the definition; the reference crate has no such stage, so this file restates nothing of
// it.  The random numbers are Philox4x32-10 (ss_philox.h): a span is a pure function of (seed, epoch, clip id, mask index) and of
// the clip's own length, so the plan needs no generator state, no atomics and no host.
//
// Two launches.  ss_specaug_plan_kernel, one lane per (clip, mask), reads the rng block and the offset table and writes the spans
// table.  ss_specaug_apply_kernel<INPLACE> reads the table and the spans and masks the rows; workgroup (b, y) serves clip b =
// blockIdx.x together with the gridDim.y - 1 others of that clip (packed_split), so containment is per clip and the grid depends on
// n_clips only.  Each workgroup first checks its clip's <= 32 spans against the clip's own extent and keeps them in LDS: a span that
// is out of range is held with width 0, and everything below tests rows and columns against checked spans only.
//
// Out of place: the clip is one contiguous run of T_b * cols elements in vec and in out, walked as a flat stream the way ss_pad.hip's
// pad_flat walks a block: 16-byte stores from the run's first 16-byte boundary in out on, element stores for the up to 3 elements in
// front of it and behind the last whole store, dword-aligned wide loads (vec and out are 4-byte aligned only, and their phases
// differ in general).  A lane finds the (row, column) of its first element with one 64-bit division when it starts and moves on by
// additions: the step of the walk is uniform.  The time test is made once per row a group touches, the frequency test per element;
// both read the spans at uniform LDS addresses (broadcasts).  Every element is moved as bits: no float instruction sees the rows.
//
// In place (out == vec): nothing is loaded.  A time span is a contiguous run of width * cols elements and is filled with 16-byte
// stores like the walk above; a frequency span is `width` elements of every row, written by a power-of-two team of lanes per row.
// Overlapping spans write the same bits twice.  The traffic is the masked bytes.
//
// The epoch bump of the combined call is one 8-byte vector store by lane 0 of workgroup (0, 0) of the apply launch: the plan launch
// ahead of it in stream order is the only reader of the block, so a captured graph draws new masks on every replay.
#include "ss_device.h"
#include "ss_hip_staging.h"
#include "ss_host_checks.h"
#include "ss_internal.h"
#include "ss_philox.h"

#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <string>

namespace ss {

namespace {

constexpr unsigned kMaxMasks = 16;        // time masks, and frequency masks, of one call
constexpr unsigned kFreqBase = 0x10000u;  // mask index of frequency mask 0
constexpr unsigned kFlatChunk = 1024;     // 16-byte groups per workgroup step of the flat walk: four per lane
constexpr unsigned kVE = 4;               // floats of a 16-byte store

// (start, width) of mask index k: width in [0, bound], start in [0, extent - width] (bound <= extent)
__host__ __device__ inline void draw_span(uint64_t seed, uint64_t epoch, uint32_t clip_id, uint32_t k, uint32_t bound, uint32_t extent, int32_t &start,
                                          int32_t &width)
{
    const Philox4 r = philox4x32_10(clip_id, k, static_cast<uint32_t>(epoch), static_cast<uint32_t>(epoch >> 32), static_cast<uint32_t>(seed),
                                    static_cast<uint32_t>(seed >> 32));
    const uint32_t w = static_cast<uint32_t>((static_cast<uint64_t>(r.w[0]) * (static_cast<uint64_t>(bound) + 1)) >> 32);
    const uint32_t s = static_cast<uint32_t>((static_cast<uint64_t>(r.w[1]) * (static_cast<uint64_t>(extent) - w + 1)) >> 32);
    start = static_cast<int32_t>(s);
    width = static_cast<int32_t>(w);
}

struct PlanScalars {
    unsigned long long total_rows;
    unsigned cols, n_time, n_freq, max_time_width, max_freq_width, clip_base;
    float time_ratio;
};

// span m (time masks first) of clip b with the segment lo .. hi: the one definition the plan launch and ss_specaug_spans share
__host__ __device__ inline void plan_span(uint64_t seed, uint64_t epoch, const PlanScalars &p, unsigned b, unsigned m, long long lo, long long hi,
                                          int32_t &start, int32_t &width)
{
    if (!(lo >= 0 && lo <= hi && static_cast<unsigned long long>(hi) <= p.total_rows)) {  // a bad segment
        start = -1;
        width = 0;
        return;
    }
    const uint32_t T = static_cast<uint32_t>(hi - lo);  // total_rows < 2^31
    if (m < p.n_time) {
        const uint32_t cap = static_cast<uint32_t>(static_cast<double>(p.time_ratio) * static_cast<double>(T));  // one f64 product, truncated
        draw_span(seed, epoch, p.clip_base + b, m, cap < p.max_time_width ? cap : p.max_time_width, T, start, width);
    } else {
        draw_span(seed, epoch, p.clip_base + b, kFreqBase + (m - p.n_time), p.max_freq_width < p.cols ? p.max_freq_width : p.cols, p.cols, start, width);
    }
}

__global__ __launch_bounds__(256) void ss_specaug_plan_kernel(const unsigned long long *__restrict__ rng, const long long *__restrict__ ro,
                                                             int *__restrict__ spans, unsigned n_clips, PlanScalars p)
{
    const unsigned n_masks = p.n_time + p.n_freq;
    const unsigned long long i = static_cast<unsigned long long>(blockIdx.x) * 256u + threadIdx.x;
    if (i >= static_cast<unsigned long long>(n_clips) * n_masks) return;
    const unsigned b = static_cast<unsigned>(i / n_masks), m = static_cast<unsigned>(i - static_cast<unsigned long long>(b) * n_masks);
    int32_t start, width;
    plan_span(rng[0], rng[1], p, b, m, ro[b], ro[b + 1], start, width);
    spans[2 * i] = start;  // the table is 4-byte aligned only
    spans[2 * i + 1] = width;
}

// elements from p up to its first 16-byte boundary (p is 4-byte aligned)
__device__ __forceinline__ unsigned to_boundary(const unsigned *p)
{
    return ((16u - static_cast<unsigned>(reinterpret_cast<uintptr_t>(p) & 15u)) & 15u) / 4u;
}

// The clip's checked spans: [0, n_time) time spans, [n_time, n_time + n_freq) frequency spans; a skipped span has width 0.  The
// tests give a word -- all ones for a hit, 0 otherwise -- that the walk blends with: select() has no branch and no bool, and the span
// loops stay scalar loops over LDS broadcasts.  (The first form of this walk kept bools and `hit ? mask : v`; at -O3 the compiler
// vectorised the span loops, and the build wrote the mask over every element of a 16-byte group: tests/test_specaug.py's clip of
// 63 rows is the one that shows it.)
struct ClipSpans {
    const int *start, *width;
    unsigned n_time, n_freq;
    __device__ __forceinline__ unsigned hit(unsigned x, unsigned k0, unsigned k1) const
    {
        unsigned any = 0;
#pragma clang loop vectorize(disable) interleave(disable)
        for (unsigned k = k0; k < k1; ++k) any |= static_cast<unsigned>(x - static_cast<unsigned>(start[k]) < static_cast<unsigned>(width[k]));
        return 0u - any;
    }
    __device__ __forceinline__ unsigned time_hit(unsigned r) const { return hit(r, 0, n_time); }
    __device__ __forceinline__ unsigned freq_hit(unsigned c) const { return hit(c, n_time, n_time + n_freq); }
};

// m is all ones or 0
__device__ __forceinline__ unsigned select(unsigned m, unsigned mask, unsigned v) { return (mask & m) | (v & ~m); }

// (row, column) of a flat element index, moved on by additions
struct RowCol {
    unsigned r, c;
    __device__ __forceinline__ void advance(unsigned dr, unsigned dc, unsigned cols)  // dc < cols
    {
        c += dc;
        if (c >= cols) {
            c -= cols;
            ++r;
        }
        r += dr;
    }
};

// dst[e] = masked(e / cols, e % cols) ? mask : src[e] for e < n = T * cols: the flat walk of one clip
__device__ __forceinline__ void mask_flat(const unsigned *__restrict__ src, unsigned *__restrict__ dst, size_t n, unsigned cols, const ClipSpans &sp,
                                          unsigned mask)
{
    const unsigned tb = to_boundary(dst);
    const unsigned head = n < tb ? static_cast<unsigned>(n) : tb;
    const size_t groups = (n - head) / kVE;
    const unsigned tail = static_cast<unsigned>(n - head - groups * kVE);
    if (blockIdx.y == 0 && threadIdx.x < head + tail) {  // at most 6 single elements
        const size_t e = threadIdx.x < head ? threadIdx.x : groups * kVE + threadIdx.x;
        const unsigned r = static_cast<unsigned>(e / cols), c = static_cast<unsigned>(e - static_cast<size_t>(r) * cols);
        dst[e] = select(sp.time_hit(r) | sp.freq_hit(c), mask, src[e]);
    }
    constexpr unsigned U = kFlatChunk / 256;
    size_t g0 = static_cast<size_t>(blockIdx.y) * kFlatChunk;
    if (g0 >= groups) return;  // uniform per workgroup
    // one division per lane; its U groups lie 256 groups apart, and the next step gridDim.y * kFlatChunk groups further on
    RowCol at[U];
    {
        const size_t e = head + (g0 + threadIdx.x) * kVE;
        at[0].r = static_cast<unsigned>(e / cols);
        at[0].c = static_cast<unsigned>(e - static_cast<size_t>(at[0].r) * cols);
    }
    const unsigned lane_dr = 256u * kVE / cols, lane_dc = 256u * kVE % cols;
#pragma unroll
    for (unsigned u = 1; u < U; ++u) {
        at[u] = at[u - 1];
        at[u].advance(lane_dr, lane_dc, cols);
    }
    const unsigned step = gridDim.y * kFlatChunk * kVE;  // <= 64 * 4096 elements
    const unsigned step_dr = step / cols, step_dc = step % cols;
    for (; g0 < groups; g0 += static_cast<size_t>(gridDim.y) * kFlatChunk) {
        unsigned v[U][kVE];
        size_t q[U];
        bool live[U];
        // the loads issued back to back: a group past the end loads group 0 instead (in bounds: groups > 0), so that no load sits behind a branch
#pragma unroll
        for (unsigned u = 0; u < U; ++u) {
            const size_t g = g0 + u * 256 + threadIdx.x;
            live[u] = g < groups;
            q[u] = head + g * kVE;
            __builtin_memcpy(v[u], __builtin_assume_aligned(src + (live[u] ? q[u] : head), 4), sizeof v[u]);  // dword-aligned wide loads
        }
#pragma unroll
        for (unsigned u = 0; u < U; ++u) {
            unsigned r = at[u].r, c = at[u].c;
            unsigned tm = sp.time_hit(r);
#pragma unroll
            for (unsigned j = 0; j < kVE; ++j) {
                v[u][j] = select(tm | sp.freq_hit(c), mask, v[u][j]);
                if (++c == cols) {
                    c = 0;
                    tm = sp.time_hit(++r);
                }
            }
            if (live[u]) *reinterpret_cast<uint4 *>(dst + q[u]) = make_uint4(v[u][0], v[u][1], v[u][2], v[u][3]);
            at[u].advance(step_dr, step_dc, cols);
        }
    }
}

// dst[e] = mask for e < n; the workgroups of the clip take the chunks in turn, the first of them is `first` (rotated per span so that
// short spans do not all fall to workgroup 0)
__device__ __forceinline__ void fill_flat(unsigned *__restrict__ dst, size_t n, unsigned mask, unsigned first)
{
    const unsigned tb = to_boundary(dst);
    const unsigned head = n < tb ? static_cast<unsigned>(n) : tb;
    const size_t groups = (n - head) / kVE;
    const unsigned tail = static_cast<unsigned>(n - head - groups * kVE);
    const unsigned turn = (blockIdx.y + gridDim.y - first % gridDim.y) % gridDim.y;
    if (turn == 0 && threadIdx.x < head + tail) dst[threadIdx.x < head ? threadIdx.x : groups * kVE + threadIdx.x] = mask;
    for (size_t g = static_cast<size_t>(turn) * 256 + threadIdx.x; g < groups; g += static_cast<size_t>(gridDim.y) * 256)
        *reinterpret_cast<uint4 *>(dst + head + g * kVE) = make_uint4(mask, mask, mask, mask);
}

template <bool INPLACE>
__global__ __launch_bounds__(256) void ss_specaug_apply_kernel(const unsigned *vec, const long long *__restrict__ ro,
                                                              const int *__restrict__ spans, unsigned *out, unsigned long long *rng,
                                                              unsigned long long total_rows, unsigned cols, unsigned n_time, unsigned n_freq,
                                                              unsigned mask)
{
    __shared__ int s_start[2 * kMaxMasks], s_width[2 * kMaxMasks];
    const unsigned b = blockIdx.x, n_masks = n_time + n_freq;
    if (rng && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) {  // the combined call: epoch + 1, both dwords in one vector store
        const unsigned long long e = rng[1] + 1;
        *reinterpret_cast<uint2 *>(rng + 1) = make_uint2(static_cast<unsigned>(e), static_cast<unsigned>(e >> 32));
    }
    const long long lo = ro[b], hi = ro[b + 1];
    if (!(lo >= 0 && lo <= hi && static_cast<unsigned long long>(hi) <= total_rows)) return;  // a bad segment: uniform per workgroup
    const unsigned T = static_cast<unsigned>(hi - lo);  // total_rows < 2^31
    if (threadIdx.x < n_masks) {
        const size_t i = (static_cast<size_t>(b) * n_masks + threadIdx.x) * 2;
        const int start = spans[i], width = spans[i + 1];
        const unsigned extent = threadIdx.x < n_time ? T : cols;
        // start, width < 2^31: the sum cannot wrap
        const bool ok = start >= 0 && width >= 0 && static_cast<unsigned>(start) + static_cast<unsigned>(width) <= extent;
        s_start[threadIdx.x] = ok ? start : 0;
        s_width[threadIdx.x] = ok ? width : 0;
    }
    __syncthreads();
    const ClipSpans sp{s_start, s_width, n_time, n_freq};
    const size_t base = static_cast<size_t>(lo) * cols;
    if constexpr (!INPLACE) {
        mask_flat(vec + base, out + base, static_cast<size_t>(T) * cols, cols, sp, mask);
    } else {
        unsigned *dst = out + base;
        for (unsigned k = 0; k < n_time; ++k)  // uniform
            if (s_width[k] > 0) fill_flat(dst + static_cast<size_t>(s_start[k]) * cols, static_cast<size_t>(s_width[k]) * cols, mask, k);
        for (unsigned k = n_time; k < n_masks; ++k) {
            const unsigned width = static_cast<unsigned>(s_width[k]), start = static_cast<unsigned>(s_start[k]);
            if (width == 0) continue;
            unsigned lg = 0;  // a team of 2^lg lanes per row: the smallest that covers the span, at most the workgroup
            while (lg < 8 && (1u << lg) < width) ++lg;
            const unsigned team = 1u << lg, rows_per_pass = 256u >> lg;
            for (unsigned r = blockIdx.y * rows_per_pass + (threadIdx.x >> lg); r < T; r += gridDim.y * rows_per_pass)
                for (unsigned c = threadIdx.x & (team - 1); c < width; c += team) dst[static_cast<size_t>(r) * cols + start + c] = mask;
        }
    }
}

// ---- host side ----

constexpr unsigned long long kCountLimit = 1ull << 31;

int check_sizes(size_t n_clips, size_t total_rows, size_t cols, size_t n_time, size_t n_freq)
{
    if (cols == 0) return fail(SS_ERR_ARG, "empty feature matrix (cols == 0)");
    if (n_time > kMaxMasks || n_freq > kMaxMasks) return fail(SS_ERR_ARG, "n_time and n_freq must be at most 16");
    if (n_clips >= kCountLimit || total_rows >= kCountLimit || cols >= kCountLimit) return fail(SS_ERR_ARG, "n_clips, total_rows and cols must be below 2^31");
    return SS_OK;
}

int check_plan(size_t clip_base, size_t n_clips, size_t total_rows, size_t cols, size_t n_time, size_t max_time_width, float time_ratio, size_t n_freq,
               size_t max_freq_width)
{
    const int rc = check_sizes(n_clips, total_rows, cols, n_time, n_freq);
    if (rc) return rc;
    if (max_time_width >= kCountLimit || max_freq_width >= kCountLimit) return fail(SS_ERR_ARG, "max_time_width and max_freq_width must be below 2^31");
    if (!(time_ratio >= 0.0f && time_ratio <= 1.0f)) return fail(SS_ERR_ARG, "time_ratio must lie in [0, 1]");
    if (clip_base > (1ull << 32) || n_clips > (1ull << 32) - clip_base) return fail(SS_ERR_ARG, "clip_base + n_clips must not exceed 2^32");
    return SS_OK;
}

PlanScalars plan_scalars(size_t clip_base, size_t total_rows, size_t cols, size_t n_time, size_t max_time_width, float time_ratio, size_t n_freq,
                         size_t max_freq_width)
{
    return PlanScalars{static_cast<unsigned long long>(total_rows), static_cast<unsigned>(cols),           static_cast<unsigned>(n_time),
                       static_cast<unsigned>(n_freq),               static_cast<unsigned>(max_time_width), static_cast<unsigned>(max_freq_width),
                       static_cast<unsigned>(clip_base),            time_ratio};
}

// the overlap rules of the apply launch: out == vec is in place, a partial overlap is an error; spans and rng lie outside both
int check_buffers(const float *vec, const float *out, size_t total_rows, size_t cols, const int32_t *spans, size_t n_clips, size_t n_masks, const uint64_t *rng)
{
    const size_t vbytes = total_rows * cols * sizeof(float), sbytes = n_clips * n_masks * 2 * sizeof(int32_t);
    if (reinterpret_cast<uintptr_t>(vec) % 4 || reinterpret_cast<uintptr_t>(out) % 4 || reinterpret_cast<uintptr_t>(spans) % 4)
        return fail(SS_ERR_ARG, "vec, out and spans must be 4-byte aligned");
    if (out != vec && ranges_overlap(vec, vbytes, out, vbytes)) return fail(SS_ERR_ARG, "out partly overlaps vec (out == vec is the in-place call)");
    if (sbytes && (ranges_overlap(vec, vbytes, spans, sbytes) || ranges_overlap(out, vbytes, spans, sbytes))) return fail(SS_ERR_ARG, "spans overlaps vec or out");
    if (rng) {
        if (reinterpret_cast<uintptr_t>(rng) % 8) return fail(SS_ERR_ARG, "rng must be 8-byte aligned");
        if (ranges_overlap(vec, vbytes, rng, 16) || ranges_overlap(out, vbytes, rng, 16)) return fail(SS_ERR_ARG, "rng overlaps vec or out");
        if (sbytes && ranges_overlap(spans, sbytes, rng, 16)) return fail(SS_ERR_ARG, "rng overlaps spans");
    }
    return SS_OK;
}

int launch_plan(const uint64_t *d_rng, size_t n_clips, const int64_t *d_ro, const PlanScalars &p, int32_t *d_spans, hipStream_t stream)
{
    const unsigned long long lanes = static_cast<unsigned long long>(n_clips) * (p.n_time + p.n_freq);
    if (lanes == 0) return SS_OK;  // a table without entries
    hipLaunchKernelGGL(ss_specaug_plan_kernel, dim3(static_cast<unsigned>((lanes + 255) / 256)), dim3(256), 0, stream,
                       reinterpret_cast<const unsigned long long *>(d_rng), reinterpret_cast<const long long *>(d_ro), reinterpret_cast<int *>(d_spans),
                       static_cast<unsigned>(n_clips), p);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "ss_specaug_plan_kernel");
    note_kernel("ss_specaug_plan_kernel");
    return SS_OK;
}

// d_rng != nullptr: the combined call, whose apply launch stores epoch + 1
int launch_apply(const float *d_vec, size_t n_clips, const int64_t *d_ro, size_t total_rows, size_t cols, const int32_t *d_spans, size_t n_time, size_t n_freq,
                 float mask_value, float *d_out, uint64_t *d_rng, hipStream_t stream)
{
    unsigned mask = 0;
    std::memcpy(&mask, &mask_value, sizeof mask);  // written as its bit pattern
    const dim3 grid(static_cast<unsigned>(n_clips), packed_split(n_clips, 64));  // no size of the table's making
    const bool inplace = d_out == d_vec;
#define SS_SPECAUG_LAUNCH(IP)                                                                                                                    \
    hipLaunchKernelGGL(ss_specaug_apply_kernel<IP>, grid, dim3(256), 0, stream, reinterpret_cast<const unsigned *>(d_vec),                     \
                       reinterpret_cast<const long long *>(d_ro), reinterpret_cast<const int *>(d_spans), reinterpret_cast<unsigned *>(d_out), \
                       reinterpret_cast<unsigned long long *>(d_rng), static_cast<unsigned long long>(total_rows), static_cast<unsigned>(cols), \
                       static_cast<unsigned>(n_time), static_cast<unsigned>(n_freq), mask)
    if (inplace) SS_SPECAUG_LAUNCH(true);
    else SS_SPECAUG_LAUNCH(false);
#undef SS_SPECAUG_LAUNCH
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "ss_specaug_apply_kernel");
    note_kernel(inplace ? "ss_specaug_apply_kernel<inplace>" : "ss_specaug_apply_kernel<copy>");
    return SS_OK;
}

}  // namespace

}  // namespace ss

extern "C" {

// host only, no device: what the plan launch writes, from the same plan_span
int ss_specaug_spans(const uint64_t *rng, size_t clip_base, size_t n_clips, const int64_t *row_offsets, size_t total_rows, size_t cols, size_t n_time,
                     size_t max_time_width, float time_ratio, size_t n_freq, size_t max_freq_width, int32_t *spans)
{
    if (n_clips == 0) return SS_OK;
    if (!rng || !row_offsets || (!spans && n_time + n_freq)) return ss::fail(SS_ERR_ARG, "null buffer");
    const int rc = ss::check_plan(clip_base, n_clips, total_rows, cols, n_time, max_time_width, time_ratio, n_freq, max_freq_width);
    if (rc) return rc;
    const ss::PlanScalars p = ss::plan_scalars(clip_base, total_rows, cols, n_time, max_time_width, time_ratio, n_freq, max_freq_width);
    const unsigned n_masks = p.n_time + p.n_freq;
    for (size_t b = 0; b < n_clips; ++b)
        for (unsigned m = 0; m < n_masks; ++m)
            ss::plan_span(rng[0], rng[1], p, static_cast<unsigned>(b), m, row_offsets[b], row_offsets[b + 1], spans[(b * n_masks + m) * 2],
                          spans[(b * n_masks + m) * 2 + 1]);
    return SS_OK;
}

int ss_specaug_plan_packed_device(const uint64_t *d_rng, size_t clip_base, size_t n_clips, const int64_t *d_row_offsets, size_t total_rows, size_t cols,
                                  size_t n_time, size_t max_time_width, float time_ratio, size_t n_freq, size_t max_freq_width, int32_t *d_spans, void *stream)
{
    if (n_clips == 0) return SS_OK;
    if (!d_rng || !d_row_offsets || (!d_spans && n_time + n_freq)) return ss::fail(SS_ERR_ARG, "null buffer");
    const int rc = ss::check_plan(clip_base, n_clips, total_rows, cols, n_time, max_time_width, time_ratio, n_freq, max_freq_width);
    if (rc) return rc;
    if (reinterpret_cast<uintptr_t>(d_rng) % 8 || reinterpret_cast<uintptr_t>(d_spans) % 4) return ss::fail(SS_ERR_ARG, "rng must be 8-byte and spans 4-byte aligned");
    const size_t sbytes = n_clips * (n_time + n_freq) * 2 * sizeof(int32_t);
    if (sbytes && ss::ranges_overlap(d_rng, 16, d_spans, sbytes)) return ss::fail(SS_ERR_ARG, "rng overlaps spans");
    return ss::launch_plan(d_rng, n_clips, d_row_offsets, ss::plan_scalars(clip_base, total_rows, cols, n_time, max_time_width, time_ratio, n_freq, max_freq_width),
                           d_spans, static_cast<hipStream_t>(stream));
}

int ss_mask_spans_packed_device(const float *d_vec, size_t n_clips, const int64_t *d_row_offsets, size_t total_rows, size_t cols, const int32_t *d_spans,
                                size_t n_time, size_t n_freq, float mask_value, float *d_out, void *stream)
{
    if (n_clips == 0) return SS_OK;
    if (!d_vec || !d_row_offsets || !d_out || (!d_spans && n_time + n_freq)) return ss::fail(SS_ERR_ARG, "null buffer");
    int rc = ss::check_sizes(n_clips, total_rows, cols, n_time, n_freq);
    if (rc || (rc = ss::check_buffers(d_vec, d_out, total_rows, cols, d_spans, n_clips, n_time + n_freq, nullptr))) return rc;
    return ss::launch_apply(d_vec, n_clips, d_row_offsets, total_rows, cols, d_spans, n_time, n_freq, mask_value, d_out, nullptr, static_cast<hipStream_t>(stream));
}

int ss_specaug_packed_device(const float *d_vec, size_t n_clips, const int64_t *d_row_offsets, size_t total_rows, size_t cols, uint64_t *d_rng, size_t clip_base,
                             size_t n_time, size_t max_time_width, float time_ratio, size_t n_freq, size_t max_freq_width, float mask_value, float *d_out,
                             int32_t *d_spans, void *stream)
{
    if (n_clips == 0) return SS_OK;
    if (!d_vec || !d_row_offsets || !d_out || !d_rng || (!d_spans && n_time + n_freq)) return ss::fail(SS_ERR_ARG, "null buffer");
    int rc = ss::check_plan(clip_base, n_clips, total_rows, cols, n_time, max_time_width, time_ratio, n_freq, max_freq_width);
    if (rc || (rc = ss::check_buffers(d_vec, d_out, total_rows, cols, d_spans, n_clips, n_time + n_freq, d_rng))) return rc;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    rc = ss::launch_plan(d_rng, n_clips, d_row_offsets, ss::plan_scalars(clip_base, total_rows, cols, n_time, max_time_width, time_ratio, n_freq, max_freq_width),
                         d_spans, st);
    if (rc) return rc;
    return ss::launch_apply(d_vec, n_clips, d_row_offsets, total_rows, cols, d_spans, n_time, n_freq, mask_value, d_out, d_rng, st);
}

// host-pointer forms (synchronous): the table is checked on the host before the device is touched
int ss_mask_spans_packed(const float *vec, size_t n_clips, const int64_t *row_offsets, size_t total_rows, size_t cols, const int32_t *spans, size_t n_time,
                         size_t n_freq, float mask_value, float *out)
{
    if (n_clips == 0) return SS_OK;
    if (!vec || !row_offsets || !out || (!spans && n_time + n_freq)) return ss::fail(SS_ERR_ARG, "null buffer");
    int rc = ss::check_sizes(n_clips, total_rows, cols, n_time, n_freq);
    if (rc || (rc = ss::check_buffers(vec, out, total_rows, cols, spans, n_clips, n_time + n_freq, nullptr)) ||
        (rc = ss::check_clip_table(row_offsets, n_clips, total_rows)))
        return rc;
    if (!ss::have_device()) return ss::no_device();
    // A checked host table covers rows 0 .. ro[n_clips) without a gap, so exactly those rows come down; the rows behind them are in
    // no clip and stay as the caller's out holds them.  In place (out == vec) the call runs on one device block.
    const size_t vbytes = total_rows * cols * sizeof(float), covered = static_cast<size_t>(row_offsets[n_clips]) * cols * sizeof(float);
    ss::HostStage st("ss_mask_spans_packed");
    float *d_vec = st.up(vec, vbytes);
    float *d_out = out == vec ? d_vec : st.room<float>(vbytes);
    const int64_t *d_ro = st.up(row_offsets, (n_clips + 1) * sizeof(int64_t));
    const int32_t *d_spans = st.up(spans, n_clips * (n_time + n_freq) * 2 * sizeof(int32_t));
    if (st.ok()) st.ran(ss_mask_spans_packed_device(d_vec, n_clips, d_ro, total_rows, cols, d_spans, n_time, n_freq, mask_value, d_out, nullptr));
    st.sync();
    st.down(out, d_out, covered);
    return st.status();
}

int ss_specaug_packed(const float *vec, size_t n_clips, const int64_t *row_offsets, size_t total_rows, size_t cols, uint64_t *rng, size_t clip_base, size_t n_time,
                      size_t max_time_width, float time_ratio, size_t n_freq, size_t max_freq_width, float mask_value, float *out, int32_t *spans)
{
    if (n_clips == 0) return SS_OK;
    if (!vec || !row_offsets || !out || !rng || (!spans && n_time + n_freq)) return ss::fail(SS_ERR_ARG, "null buffer");
    int rc = ss::check_plan(clip_base, n_clips, total_rows, cols, n_time, max_time_width, time_ratio, n_freq, max_freq_width);
    if (rc || (rc = ss::check_buffers(vec, out, total_rows, cols, spans, n_clips, n_time + n_freq, rng)) ||
        (rc = ss::check_clip_table(row_offsets, n_clips, total_rows)))
        return rc;
    if (!ss::have_device()) return ss::no_device();
    // as ss_mask_spans_packed; the spans come down here, and of the generator's two words the advanced counter alone
    const size_t vbytes = total_rows * cols * sizeof(float), covered = static_cast<size_t>(row_offsets[n_clips]) * cols * sizeof(float);
    const size_t sbytes = n_clips * (n_time + n_freq) * 2 * sizeof(int32_t);
    ss::HostStage st("ss_specaug_packed");
    float *d_vec = st.up(vec, vbytes);
    float *d_out = out == vec ? d_vec : st.room<float>(vbytes);
    const int64_t *d_ro = st.up(row_offsets, (n_clips + 1) * sizeof(int64_t));
    int32_t *d_spans = st.room<int32_t>(sbytes);
    uint64_t *d_rng = st.up(rng, 16);
    if (st.ok())
        st.ran(ss_specaug_packed_device(d_vec, n_clips, d_ro, total_rows, cols, d_rng, clip_base, n_time, max_time_width, time_ratio, n_freq, max_freq_width,
                                        mask_value, d_out, d_spans, nullptr));
    st.sync();
    st.down(out, d_out, covered);
    st.down(spans, d_spans, sbytes);
    st.down(rng + 1, d_rng + 1, 8);
    return st.status();
}

}  // extern "C"
