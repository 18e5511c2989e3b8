// Post-processing on the feature matrix: cmvn, cmvnw, derivative_extraction, extract_derivative_feature.
// Reference: speechsauce/src/processing.rs:222-254 (derivative_extraction), :265-300 (cmvn), :315-371 (cmvnw),
// feature.rs:253-269 (extract_derivative_feature); the pads are np.pad 'edge' / 'symmetric' as util.rs:108-124 quotes.
//
// The data is the [clips x rows x cols] feature block the hot path just wrote (5 MB for 1024 one-second clips), so these
// are small HBM/L2-bound kernels with neighbouring threads on neighbouring addresses (columns fastest) and f64 accumulators
// for the statistics (full rate on gfx950; it keeps the result within an ulp of the f64 oracle for 6 000-row matrices too):
// cmvn sums chunks of rows per thread and normalises per element (two launches, no atomics: bit-reproducible); cmvnw slides
// its window sums over a chunk of rows per thread (O(rows + win) loads per column chunk instead of O(rows * win)).
// cmvn, its packed form and the stream pool take the squares about a value of the column itself (var_about): the mean is formed
// from the plain sum as before (ss_vad.hip and the mean-only outputs rest on its bits), the variance keeps its digits on a column
// that barely moves around a large offset.
#include "ss_device.h"
#include "ss_hip_staging.h"
#include "ss_host_checks.h"
#include "ss_internal.h"
#include "speechsauce_amd.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>

namespace ss {

namespace {

constexpr double kEps30 = 9.313225746154785e-10;  // 2f32.powf(-30.), processing.rs:266, :324

// Walker over np.pad(..., 'symmetric') of an axis of length n (reflection that repeats the edge sample, period 2n):
// position p of the padded axis maps to idx; step() moves to p + 1 without a division.
struct SymWalk {
    unsigned idx;
    int dir;
    unsigned n;
    __device__ SymWalk(long long p, unsigned n_) : n(n_)
    {
        const long long period = 2ll * n_;
        long long m = p % period;
        if (m < 0) m += period;
        dir = m < n_ ? 1 : -1;
        idx = static_cast<unsigned>(m < n_ ? m : period - 1 - m);
    }
    __device__ void step()
    {
        if (dir > 0) {
            if (idx + 1 == n) dir = -1;  // the edge sample repeats
            else ++idx;
        } else {
            if (idx == 0) dir = 1;
            else --idx;
        }
    }
};

// Population variance of n values from their mean and s2k = sum (v - K)^2, K one of the values: s2k / n - (mean - K)^2.  Both
// terms are of the order of the column's spread squared (about the origin they are of the order of mean^2, and a column that
// moves by a few ulps around 1000 is lost in their difference).  Clamped at 0; a NaN passes (fmax would turn it into 0).
__device__ __forceinline__ double var_about(double s2k, double n, double mean, double K)
{
    const double d = mean - K;
    const double var = fma(-d, d, s2k / n);
    return var < 0.0 ? 0.0 : var;
}

__device__ __forceinline__ bool finite_sum(double s) { return fabs(s) < INFINITY; }  // false for NaN

// ---- element-wise logarithms: lmfe's ln (feature.rs:242-245 -> util.rs:372-381) and librosa's power_to_db ----
__global__ __launch_bounds__(256) void ss_ln_kernel(float *__restrict__ x, unsigned long long n)
{
    const unsigned long long g = static_cast<unsigned long long>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (g < n) x[g] = logf(x[g]);
}

// (float_key / key_float, the ordered-integer keys of the maxima: ss_device.h)
// 10 log10(max(amin, S)) - 10 log10(max(amin, ref)); the block maxima go to one word for the top_db clamp
__global__ __launch_bounds__(256) void ss_power_to_db_kernel(const float *__restrict__ s, float *__restrict__ out, unsigned long long n, float amin,
                                                            float ref_db, int *__restrict__ max_key)
{
    const unsigned long long g = static_cast<unsigned long long>(blockIdx.x) * blockDim.x + threadIdx.x;
    float db = -INFINITY;
    if (g < n) {
        db = 10.0f * log10f(fmaxf(amin, s[g])) - ref_db;
        out[g] = db;
    }
    if (max_key) {
        for (int m = 1; m < 64; m <<= 1) db = fmaxf(db, __shfl_xor(db, m, 64));
        if ((threadIdx.x & 63) == 0 && db > -INFINITY) atomicMax(max_key, float_key(db));
    }
}

__global__ __launch_bounds__(256) void ss_db_floor_kernel(float *__restrict__ out, unsigned long long n, float top_db, const int *__restrict__ max_key)
{
    const unsigned long long g = static_cast<unsigned long long>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (g < n) out[g] = fmaxf(out[g], key_float(*max_key) - top_db);
}

// ---- cmvn: column statistics in two kernels, no atomics (bit-reproducible) ----
// partial sums of x and (x - K)^2 over a chunk of rows, K the clip's first row of the column; thread = (clip, chunk, column),
// columns fastest
__global__ __launch_bounds__(256) void ss_cmvn_partial_kernel(const float *__restrict__ x, double *__restrict__ part, unsigned long long total,
                                                             unsigned rows, unsigned cols, unsigned chunks, unsigned rpc)
{
    const unsigned long long g = static_cast<unsigned long long>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (g >= total) return;
    const unsigned c = static_cast<unsigned>(g % cols);
    const unsigned long long cc = g / cols;
    const unsigned chunk = static_cast<unsigned>(cc % chunks);
    const unsigned long long clip = cc / chunks;
    const unsigned r0 = chunk * rpc, r1 = min(rows, r0 + rpc);
    const float *src = x + clip * rows * cols + c;
    const double K = static_cast<double>(src[0]);
    double s1 = 0.0, s2 = 0.0;
    for (unsigned r = r0; r < r1; ++r) {
        const double v = static_cast<double>(src[static_cast<size_t>(r) * cols]);
        const double d = v - K;
        s1 += v;
        s2 += d * d;
    }
    part[2 * g] = s1;
    part[2 * g + 1] = s2;
}

// thread = output element: mean (and population std, about the clip's first row) of its column from the chunk partials, then
// (x - mean) / (std + 2^-30)
__global__ __launch_bounds__(256) void ss_cmvn_apply_kernel(const float *__restrict__ x, const double *__restrict__ part, float *__restrict__ out,
                                                           unsigned long long total, unsigned rows, unsigned cols, unsigned chunks, int variance)
{
    const unsigned long long g = static_cast<unsigned long long>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (g >= total) return;
    const unsigned long long per_clip = static_cast<unsigned long long>(rows) * cols;
    const unsigned long long clip = g / per_clip;
    const unsigned c = static_cast<unsigned>((g - clip * per_clip) % cols);
    const double *pp = part + 2 * (clip * chunks * cols + c);
    double s1 = 0.0, s2 = 0.0;
    for (unsigned k = 0; k < chunks; ++k) {
        s1 += pp[2 * static_cast<size_t>(k) * cols];
        s2 += pp[2 * static_cast<size_t>(k) * cols + 1];
    }
    const double mean = s1 / rows;
    double inv = 1.0;
    if (variance) {
        // std_axis(Axis(0), 0.) of the mean-subtracted column (processing.rs:283)
        const double var = var_about(s2, rows, mean, static_cast<double>(x[clip * per_clip + c]));
        inv = 1.0 / (sqrt(var) + kEps30);
    }
    out[g] = static_cast<float>((static_cast<double>(x[g]) - mean) * inv);
}

// ---- cmvnw: sliding window sums over the symmetric-padded rows; thread = (clip, chunk of rows, column) ----
// The chunk bodies: rows i0 .. i1 of a column of ONE clip (src / dst point at that clip's column; rows is the clip's own row count,
// so the symmetric reflection wraps inside the clip).  The sums slide: the row that enters is added, the row that leaves is
// subtracted.  A NaN or an infinity cannot be subtracted out again (inf - inf), so sums that are not finite after a step are
// formed afresh from the window (cmvnw_window_sums): a finite window behind a bad row is normalised as if the row had never been
// there, and finite input never takes that branch.
template <bool SQUARES>
__device__ __forceinline__ void cmvnw_window_sums(const float *__restrict__ src, unsigned cols, unsigned win, SymWalk w, double &s1, double &s2)
{
    s1 = 0.0;
    s2 = 0.0;
    for (unsigned k = 0; k < win; ++k) {
        const double v = static_cast<double>(src[static_cast<size_t>(w.idx) * cols]);
        s1 += v;
        if (SQUARES) s2 += v * v;
        w.step();
    }
}

// pass 1: ms[i] = x[i] - mean of the win rows centred on i
__device__ __forceinline__ void cmvnw_mean_chunk(const float *__restrict__ src, float *__restrict__ dst, unsigned rows, unsigned cols, unsigned win,
                                                 unsigned i0, unsigned i1)
{
    const long long pad = (win - 1) / 2;
    SymWalk head(static_cast<long long>(i0) - pad, rows), tail = head;  // tail: oldest row of the window, head: next row to enter
    double s = 0.0;
#pragma unroll 4
    for (unsigned w = 0; w < win; ++w) {
        s += static_cast<double>(src[static_cast<size_t>(head.idx) * cols]);
        head.step();
    }
    for (unsigned i = i0; i < i1; ++i) {
        dst[static_cast<size_t>(i) * cols] = static_cast<float>(static_cast<double>(src[static_cast<size_t>(i) * cols]) - s / win);
        s += static_cast<double>(src[static_cast<size_t>(head.idx) * cols]) - static_cast<double>(src[static_cast<size_t>(tail.idx) * cols]);
        head.step();
        tail.step();
        if (!finite_sum(s)) {
            double unused;
            cmvnw_window_sums<false>(src, cols, win, tail, s, unused);
        }
    }
}

// pass 2 (variance_normalization): ms / (population std of ms over the same symmetric window + 2^-30).  The window's mean of ms is
// small against its spread (ms is mean-subtracted), so the squares are summed about the origin.
__device__ __forceinline__ void cmvnw_var_chunk(const float *__restrict__ src, float *__restrict__ dst, unsigned rows, unsigned cols, unsigned win,
                                                unsigned i0, unsigned i1)
{
    const long long pad = (win - 1) / 2;
    SymWalk head(static_cast<long long>(i0) - pad, rows), tail = head;
    double s1 = 0.0, s2 = 0.0;
#pragma unroll 4
    for (unsigned w = 0; w < win; ++w) {
        const double v = static_cast<double>(src[static_cast<size_t>(head.idx) * cols]);
        s1 += v;
        s2 += v * v;
        head.step();
    }
    for (unsigned i = i0; i < i1; ++i) {
        const double m = s1 / win;
        const double d = s2 / win - m * m;
        const double var = d < 0.0 ? 0.0 : d;  // a NaN passes: a window that holds one gives NaN, as the reference does
        dst[static_cast<size_t>(i) * cols] = static_cast<float>(static_cast<double>(src[static_cast<size_t>(i) * cols]) / (sqrt(var) + kEps30));
        const double vin = static_cast<double>(src[static_cast<size_t>(head.idx) * cols]);
        const double vout = static_cast<double>(src[static_cast<size_t>(tail.idx) * cols]);
        s1 += vin - vout;
        s2 += vin * vin - vout * vout;
        head.step();
        tail.step();
        if (!finite_sum(s1) || !finite_sum(s2)) cmvnw_window_sums<true>(src, cols, win, tail, s1, s2);
    }
}

__global__ __launch_bounds__(256) void ss_cmvnw_mean_kernel(const float *__restrict__ x, float *__restrict__ ms, unsigned long long total,
                                                            unsigned rows, unsigned cols, unsigned win, unsigned chunks, unsigned rpc)
{
    const unsigned long long g = static_cast<unsigned long long>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (g >= total) return;
    const unsigned c = static_cast<unsigned>(g % cols);
    const unsigned long long cc = g / cols;
    const unsigned chunk = static_cast<unsigned>(cc % chunks);
    const unsigned long long clip = cc / chunks;
    const unsigned i0 = chunk * rpc, i1 = min(rows, i0 + rpc);
    cmvnw_mean_chunk(x + clip * rows * cols + c, ms + clip * rows * cols + c, rows, cols, win, i0, i1);
}

__global__ __launch_bounds__(256) void ss_cmvnw_var_kernel(const float *__restrict__ ms, float *__restrict__ out, unsigned long long total,
                                                           unsigned rows, unsigned cols, unsigned win, unsigned chunks, unsigned rpc)
{
    const unsigned long long g = static_cast<unsigned long long>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (g >= total) return;
    const unsigned c = static_cast<unsigned>(g % cols);
    const unsigned long long cc = g / cols;
    const unsigned chunk = static_cast<unsigned>(cc % chunks);
    const unsigned long long clip = cc / chunks;
    const unsigned i0 = chunk * rpc, i1 = min(rows, i0 + rpc);
    cmvnw_var_chunk(ms + clip * rows * cols + c, out + clip * rows * cols + c, rows, cols, win, i0, i1);
}

// derivative along the FEATURE axis with edge clamping, literal reference arithmetic: sum_R (R f[c+R] - f[c-R]) / sum_R 2R^2
__device__ __forceinline__ float deriv_at(const float *row, unsigned cols, unsigned c, unsigned dw, float inv_scale)
{
    float acc = 0.f;
    for (unsigned R = 1; R <= dw; ++R) {
        const unsigned hi = c + R < cols ? c + R : cols - 1;
        const unsigned lo = c >= R ? c - R : 0;
        acc += row[hi] * static_cast<float>(R) - row[lo];
    }
    return acc * inv_scale;
}

__global__ __launch_bounds__(256) void ss_derivative_kernel(const float *__restrict__ x, float *__restrict__ out, unsigned long long total,
                                                            unsigned cols, unsigned dw, float inv_scale)
{
    const unsigned long long g = static_cast<unsigned long long>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (g >= total) return;
    const unsigned long long r = g / cols;
    const unsigned c = static_cast<unsigned>(g - r * cols);
    out[g] = deriv_at(x + r * cols, cols, c, dw, inv_scale);
}

// cube[r][c][0..2] = (f, d1, d2), d1 = derivative(f, 2), d2 = derivative(d1, 2); d1 is recomputed for the 5 clamped neighbours
__global__ __launch_bounds__(256) void ss_derivative_cube_kernel(const float *__restrict__ x, float *__restrict__ cube, unsigned long long total,
                                                                 unsigned cols)
{
    const unsigned long long g = static_cast<unsigned long long>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (g >= total) return;
    const unsigned long long r = g / cols;
    const unsigned c = static_cast<unsigned>(g - r * cols);
    const float *row = x + r * cols;
    constexpr float inv10 = 1.0f / 10.0f;  // sum_{R=1,2} 2 R^2
    float acc = 0.f;
    for (unsigned R = 1; R <= 2; ++R) {
        const unsigned hi = c + R < cols ? c + R : cols - 1;
        const unsigned lo = c >= R ? c - R : 0;
        acc += deriv_at(row, cols, hi, 2, inv10) * static_cast<float>(R) - deriv_at(row, cols, lo, 2, inv10);
    }
    cube[3 * g] = row[c];
    cube[3 * g + 1] = deriv_at(row, cols, c, 2, inv10);
    cube[3 * g + 2] = acc * inv10;
}

// ---- packed variable-length clips (ss_cmvn_packed* / ss_cmvnw_packed* / ss_power_to_db_packed*) ----
// Clip b owns rows off[b] .. off[b+1] of the [total_rows x cols] block; the table is a device array that only the kernels read.
// Workgroup (b, z) = blockIdx (x, y) serves clip b: every chunk boundary and summation order is counted from the clip's own first
// row and depends on its row count and the scalar arguments only, so a clip's bits do not depend on where it sits in the block.
// gridDim.y workgroups share a long clip (strided over its tasks); for a short clip the ones past its work return at once.
// Containment: a segment that is reversed, starts below 0 or ends past total_rows is skipped, and every address a workgroup forms
// lies inside its own validated segment (packed_segment, ss_device.h).
constexpr unsigned kCmvnChunks = 64;   // chunks = min(64, ceil(rows / 32)), as ss_cmvn_batch_device
constexpr unsigned kCmvnTile = 32;     // columns whose chunk partials sit in LDS at a time: 64 x 32 x 2 doubles = 32 KiB
constexpr unsigned kCmvnSplitRows = 2048;  // a clip gets one workgroup per 2048 rows (up to gridDim.y)

// cmvn of one clip per workgroup, one launch, no scratch: the chunk partials of ss_cmvn_partial_kernel go to LDS instead of HBM,
// the column statistics are summed from them in the same order, then the workgroup normalises the clip's elements.  The
// workgroups that share a long clip each compute the (identical) statistics and normalise a strided share of the elements.
__global__ __launch_bounds__(256) void ss_cmvn_packed_kernel(const float *__restrict__ x, const long long *__restrict__ off, float *__restrict__ out,
                                                            unsigned long long total_rows, unsigned cols, int variance)
{
    __shared__ double part[kCmvnChunks * kCmvnTile * 2];
    __shared__ double stat[kCmvnTile * 2];  // mean, 1 / (std + 2^-30)
    const Segment seg = packed_segment(off, total_rows);
    if (seg.rows == 0) return;
    const unsigned rows = seg.rows;
    const unsigned share = min(gridDim.y, (rows + kCmvnSplitRows - 1) / kCmvnSplitRows);
    if (blockIdx.y >= share) return;
    const unsigned chunks = min(kCmvnChunks, (rows + 31) / 32);
    const unsigned rpc = (rows + chunks - 1) / chunks;
    const float *src = x + seg.row0 * cols;
    float *dst = out + seg.row0 * cols;
    for (unsigned c0 = 0; c0 < cols; c0 += kCmvnTile) {
        const unsigned ct = min(kCmvnTile, cols - c0);
        for (unsigned k = threadIdx.x; k < chunks * ct; k += 256) {  // task = (chunk, column), columns fastest
            const unsigned chunk = k / ct, c = k - chunk * ct;
            const unsigned r0 = chunk * rpc, r1 = min(rows, r0 + rpc);
            const float *p = src + c0 + c;
            const double K = static_cast<double>(p[0]);  // the clip's first row of the column
            double s1 = 0.0, s2 = 0.0;
            for (unsigned r = r0; r < r1; ++r) {
                const double v = static_cast<double>(p[static_cast<size_t>(r) * cols]);
                const double d = v - K;
                s1 += v;
                s2 += d * d;
            }
            part[2 * k] = s1;
            part[2 * k + 1] = s2;
        }
        __syncthreads();
        if (threadIdx.x < ct) {
            double s1 = 0.0, s2 = 0.0;
            for (unsigned k = 0; k < chunks; ++k) {
                s1 += part[2 * (k * ct + threadIdx.x)];
                s2 += part[2 * (k * ct + threadIdx.x) + 1];
            }
            const double mean = s1 / rows;
            double inv = 1.0;
            if (variance) {
                const double var = var_about(s2, rows, mean, static_cast<double>(src[c0 + threadIdx.x]));  // as ss_cmvn_apply_kernel
                inv = 1.0 / (sqrt(var) + kEps30);
            }
            stat[2 * threadIdx.x] = mean;
            stat[2 * threadIdx.x + 1] = inv;
        }
        __syncthreads();
        const unsigned long long n = static_cast<unsigned long long>(rows) * ct;
        for (unsigned long long e = static_cast<unsigned long long>(blockIdx.y) * 256 + threadIdx.x; e < n; e += static_cast<unsigned long long>(share) * 256) {
            const unsigned long long r = e / ct;
            const unsigned c = static_cast<unsigned>(e - r * ct);
            const size_t at = static_cast<size_t>(r) * cols + c0 + c;
            dst[at] = static_cast<float>((static_cast<double>(src[at]) - stat[2 * c]) * stat[2 * c + 1]);
        }
        __syncthreads();  // the next column tile overwrites part / stat
    }
}

// pass 1 (VAR = false) or pass 2 (VAR = true) of cmvnw over packed clips (cmvnw_mean_chunk / cmvnw_var_chunk above): task = (chunk
// of rpc rows counted from the clip's first row, column), columns fastest; the gridDim.y workgroups of a clip stride over its tasks
template <bool VAR>
__global__ __launch_bounds__(256) void ss_cmvnw_packed_kernel(const float *__restrict__ in, const long long *__restrict__ off, float *__restrict__ out,
                                                             unsigned long long total_rows, unsigned cols, unsigned win, unsigned rpc)
{
    const Segment seg = packed_segment(off, total_rows);
    if (seg.rows == 0) return;
    const unsigned rows = seg.rows;
    const unsigned chunks = (rows + rpc - 1) / rpc;
    const unsigned long long tasks = static_cast<unsigned long long>(chunks) * cols;
    const float *src = in + seg.row0 * cols;
    float *dst = out + seg.row0 * cols;
    for (unsigned long long k = static_cast<unsigned long long>(blockIdx.y) * 256 + threadIdx.x; k < tasks; k += static_cast<unsigned long long>(gridDim.y) * 256) {
        const unsigned chunk = static_cast<unsigned>(k / cols);
        const unsigned c = static_cast<unsigned>(k - static_cast<unsigned long long>(chunk) * cols);
        const unsigned i0 = chunk * rpc, i1 = min(rows, i0 + rpc);
        if (VAR) cmvnw_var_chunk(src + c, dst + c, rows, cols, win, i0, i1);
        else cmvnw_mean_chunk(src + c, dst + c, rows, cols, win, i0, i1);
    }
}

// ---- causal sliding-window CMVN over a pool of stream states (ss_cmvn_stream_packed*) ----
// Entry i owns rows ro[i] .. ro[i+1] of the [total_rows x cols] blocks and pool row slots[i]: L = (win - 1) * cols + 1 floats, the
// last win - 1 raw rows of its stream (oldest first, right-aligned, zeros in front) and, in the last float, how many of them are
// valid.  Row t of the stream is normalised over its own trailing window, rows max(t - win + 1, 0) .. t: the valid history rows,
// then the entry's rows up to the row itself.  Both sums (the squares about the row itself) are formed afresh for every element,
// oldest row first, so an element's bits depend on the window's values only -- not on how the stream was cut into calls, the
// entry's place in the call or its slot.
// One workgroup per entry, one launch: the workgroup owns its pool row, normalises the entry's rows and then moves the row on.
// Containment: an entry is skipped unless 0 <= ro[i] <= ro[i+1] <= total_rows and 0 <= slots[i] < pool_streams; a count word that
// is not an integer in [0, win - 1] (NaN included) is read as 0, so the window never reaches in front of the pool row.
struct StreamEntry {
    unsigned long long row0;
    unsigned rows;   // 0: nothing to do (no rows or a rejected entry)
    unsigned count;  // valid history rows, 0 .. win - 1
    float *state;    // the entry's pool row
};

__device__ __forceinline__ StreamEntry cmvn_stream_entry(const long long *__restrict__ ro, const int *__restrict__ slots, unsigned long long total_rows,
                                                         unsigned pool_streams, float *pool, unsigned state_len, unsigned hist)
{
    const long long lo = ro[blockIdx.x], hi = ro[blockIdx.x + 1];
    const int slot = slots[blockIdx.x];
    StreamEntry e{0, 0, 0, nullptr};
    if (lo >= 0 && lo < hi && static_cast<unsigned long long>(hi) <= total_rows && slot >= 0 && static_cast<unsigned>(slot) < pool_streams) {
        e.row0 = static_cast<unsigned long long>(lo);
        e.rows = static_cast<unsigned>(hi - lo);  // total_rows < 2^31: the row count fits
        e.state = pool + static_cast<size_t>(slot) * state_len;
        const float cw = e.state[state_len - 1];
        if (cw >= 0.0f && cw <= static_cast<float>(hist) && cw == floorf(cw)) e.count = static_cast<unsigned>(cw);  // hist < 2^24: exact
    }
    return e;
}

constexpr unsigned kStreamMove = 4;      // pool-row floats a thread moves per step of the advance in global memory
constexpr unsigned kStreamTile = 32;     // columns staged in LDS at a time, as kCmvnTile
constexpr unsigned kStreamLds = 10240;   // floats of LDS (40 KiB: four workgroups per CU): win = 301 with up to 20 new rows per tile

// the two sums of one element over n values `stride` floats apart, oldest first: s1 of the values, s2 of their squared distances
// from K, the row being normalised (fma written out: the same bits from every caller).  Without variance normalisation nobody reads
// s2: SQUARES = false leaves it alone (s1 is formed in the same order either way).
template <bool SQUARES>
__device__ __forceinline__ void stream_window_sums(const float *p, unsigned n, size_t stride, double K, double &s1, double &s2)
{
#pragma unroll 8
    for (unsigned j = 0; j < n; ++j, p += stride) {
        const double v = static_cast<double>(*p);
        s1 += v;
        if (SQUARES) {
            const double d = v - K;
            s2 = fma(d, d, s2);
        }
    }
}

// the tail of ss_cmvn_packed_kernel on the sums of a window of n rows
__device__ __forceinline__ float stream_normalise(float x, double s1, double s2, unsigned n, int variance)
{
    const double mean = s1 / n;
    double inv = 1.0;
    if (variance) {
        const double var = var_about(s2, n, mean, static_cast<double>(x));
        inv = 1.0 / (sqrt(var) + kEps30);
    }
    return static_cast<float>((static_cast<double>(x) - mean) * inv);
}

__global__ __launch_bounds__(256) void ss_cmvn_stream_packed_kernel(const float *__restrict__ x, const long long *__restrict__ ro,
                                                                   const int *__restrict__ slots, float *__restrict__ out, float *pool,
                                                                   unsigned long long total_rows, unsigned pool_streams, unsigned cols,
                                                                   unsigned win, int variance)
{
    __shared__ float tile[kStreamLds];
    const unsigned hist = win - 1, state_len = hist * cols + 1;
    const StreamEntry e = cmvn_stream_entry(ro, slots, total_rows, pool_streams, pool, state_len, hist);
    if (e.rows == 0) return;  // the whole workgroup: the pool row stays as it is
    const unsigned rows = e.rows, count = e.count;
    const float *src = x + e.row0 * cols;
    float *dst = out + e.row0 * cols;
    const float *old = e.state + static_cast<size_t>(hist - count) * cols;  // the oldest valid history row
    // The stream's rows are counted from the oldest valid history row: 0 .. count - 1 the history, count .. count + rows - 1 the
    // entry's.  After the call the pool row holds rows count + rows - hist .. count + rows - 1 (zeros where that is below 0).
    const long long lead = static_cast<long long>(hist) - count - rows;  // rows of zeros in front of the new pool row (<= 0: none)
    const unsigned long long span = static_cast<unsigned long long>(count) + rows;
    if (span * min(cols, kStreamTile) <= kStreamLds) {
        // the usual tick: per column tile the history and the new rows go to LDS once, every element walks its window there, and
        // the tile's share of the new pool row is written from LDS (nothing of the pool row is read after it was written)
        for (unsigned c0 = 0; c0 < cols; c0 += kStreamTile) {
            const unsigned ct = min(kStreamTile, cols - c0);
            const unsigned staged = static_cast<unsigned>(span) * ct;
            for (unsigned i = threadIdx.x; i < staged; i += 256) {
                const unsigned j = i / ct, c = i - j * ct;
                tile[i] = j < count ? old[static_cast<size_t>(j) * cols + c0 + c] : src[static_cast<size_t>(j - count) * cols + c0 + c];
            }
            __syncthreads();
            for (unsigned k = threadIdx.x; k < rows * ct; k += 256) {  // task = (row, column), columns fastest
                const unsigned t = k / ct, c = k - t * ct;
                const unsigned n = min(count + t + 1, win);  // rows in the window, the row itself the newest
                const float xt = tile[(count + t) * ct + c];
                double s1 = 0.0, s2 = 0.0;
                const float *oldest = tile + (count + t + 1 - n) * ct + c;
                if (variance) stream_window_sums<true>(oldest, n, ct, static_cast<double>(xt), s1, s2);
                else stream_window_sums<false>(oldest, n, ct, 0.0, s1, s2);
                dst[static_cast<size_t>(t) * cols + c0 + c] = stream_normalise(xt, s1, s2, n, variance);
            }
            for (unsigned i = threadIdx.x; i < hist * ct; i += 256) {
                const unsigned r = i / ct, c = i - r * ct;
                const long long j = static_cast<long long>(r) - lead;
                e.state[static_cast<size_t>(r) * cols + c0 + c] = j >= 0 ? tile[static_cast<unsigned>(j) * ct + c] : 0.0f;
            }
            __syncthreads();  // the next column tile overwrites the staged rows
        }
    } else {
        // a long catch-up entry or a window too large for LDS: the same walk, in the same order, in global memory
        const unsigned long long tasks = static_cast<unsigned long long>(rows) * cols;
        for (unsigned long long k = threadIdx.x; k < tasks; k += 256) {
            const unsigned t = static_cast<unsigned>(k / cols);
            const unsigned c = static_cast<unsigned>(k - static_cast<unsigned long long>(t) * cols);
            const unsigned n = min(count + t + 1, win);
            const unsigned first = count + t + 1 - n;   // the window's oldest row
            const unsigned h0 = min(first, count);      // history rows h0 .. count - 1, then the entry's rows first - h0 .. t
            const float xt = src[k];
            double s1 = 0.0, s2 = 0.0;
            const float *hist_rows = old + static_cast<size_t>(h0) * cols + c, *new_rows = src + static_cast<size_t>(first - h0) * cols + c;
            if (variance) {
                stream_window_sums<true>(hist_rows, count - h0, cols, static_cast<double>(xt), s1, s2);
                stream_window_sums<true>(new_rows, n - (count - h0), cols, static_cast<double>(xt), s1, s2);
            } else {
                stream_window_sums<false>(hist_rows, count - h0, cols, 0.0, s1, s2);
                stream_window_sums<false>(new_rows, n - (count - h0), cols, 0.0, s1, s2);
            }
            dst[k] = stream_normalise(xt, s1, s2, n, variance);
        }
        // A history row moves towards the front of the pool row it is read from, so the row is rewritten in ascending steps of
        // 256 * kStreamMove floats, every step read in full before it is written: a later step reads only what lies behind
        // everything written so far.
        const unsigned long long hn = static_cast<unsigned long long>(hist) * cols;
        for (unsigned long long base = 0; base < hn; base += 256 * kStreamMove) {
            float v[kStreamMove];
#pragma unroll
            for (unsigned u = 0; u < kStreamMove; ++u) {
                const unsigned long long at = base + u * 256 + threadIdx.x;
                v[u] = 0.0f;
                if (at < hn) {
                    const long long j = static_cast<long long>(at / cols) - lead;
                    const unsigned c = static_cast<unsigned>(at % cols);
                    if (j >= static_cast<long long>(count)) v[u] = src[static_cast<size_t>(j - count) * cols + c];
                    else if (j >= 0) v[u] = old[static_cast<size_t>(j) * cols + c];
                }
            }
            __syncthreads();
#pragma unroll
            for (unsigned u = 0; u < kStreamMove; ++u) {
                const unsigned long long at = base + u * 256 + threadIdx.x;
                if (at < hn) e.state[at] = v[u];
            }
        }
        __syncthreads();  // (win_size == 1: no step above; the count word is read by every thread before it is written)
    }
    if (threadIdx.x == 0) e.state[state_len - 1] = static_cast<float>(min(count + rows, hist));
}

// power_to_db over packed clips: clip b's segment is elements cols * off[b] .. cols * off[b+1]; its maximum goes to max_key[b]
// (ordered-integer atomicMax: a maximum does not depend on the order of arrival), the floor pass reads it back
__global__ __launch_bounds__(256) void ss_power_to_db_packed_kernel(const float *__restrict__ s, const long long *__restrict__ off, float *__restrict__ out,
                                                                   unsigned long long total_rows, unsigned cols, float amin, float ref_db,
                                                                   int *__restrict__ max_key)
{
    const Segment seg = packed_segment(off, total_rows);
    if (seg.rows == 0) return;
    const unsigned long long n = static_cast<unsigned long long>(seg.rows) * cols;
    const float *src = s + seg.row0 * cols;
    float *dst = out + seg.row0 * cols;
    float mx = -INFINITY;
    for (unsigned long long g = static_cast<unsigned long long>(blockIdx.y) * 256 + threadIdx.x; g < n; g += static_cast<unsigned long long>(gridDim.y) * 256) {
        const float db = 10.0f * log10f(fmaxf(amin, src[g])) - ref_db;
        dst[g] = db;
        mx = fmaxf(mx, db);
    }
    if (max_key) {
        for (int m = 1; m < 64; m <<= 1) mx = fmaxf(mx, __shfl_xor(mx, m, 64));
        if ((threadIdx.x & 63) == 0 && mx > -INFINITY) atomicMax(max_key + blockIdx.x, float_key(mx));
    }
}

__global__ __launch_bounds__(256) void ss_db_floor_packed_kernel(float *__restrict__ out, const long long *__restrict__ off, unsigned long long total_rows,
                                                                unsigned cols, float top_db, const int *__restrict__ max_key)
{
    const Segment seg = packed_segment(off, total_rows);
    if (seg.rows == 0) return;
    const unsigned long long n = static_cast<unsigned long long>(seg.rows) * cols;
    float *dst = out + seg.row0 * cols;
    const float floor_db = key_float(max_key[blockIdx.x]) - top_db;
    for (unsigned long long g = static_cast<unsigned long long>(blockIdx.y) * 256 + threadIdx.x; g < n; g += static_cast<unsigned long long>(gridDim.y) * 256)
        dst[g] = fmaxf(dst[g], floor_db);
}

// ---- the dB step of the log-mel calls (ss_log_mel_spectrogram*): per-clip maxima in max_key (DbArgs, ss_device.h) ----
// A clip's block: `seg` elements from element blockIdx.x * seg (equal-length clips, no table), or the [M x R_b] block of clip
// blockIdx.x of a packed call -- only where the clip passes the mel kernels' own table check (varrows_clip): what they skipped
// stays as it is.
struct ClipBlock {
    unsigned long long first, n;  // n = 0: nothing to do
};
__device__ __forceinline__ ClipBlock equal_block(unsigned long long seg) { return {blockIdx.x * seg, seg}; }
__device__ __forceinline__ ClipBlock varrows_block(const VarRowsArgs &v, unsigned cols)
{
    const VarRowClip c = varrows_clip(v, blockIdx.x);
    if (!c.ok) return {0, 0};
    return {static_cast<unsigned long long>(c.r0) * cols, static_cast<unsigned long long>(c.R) * cols};
}
// the floor of ss_db_floor_packed_kernel over such a block
__device__ __forceinline__ void db_floor_block(float *__restrict__ out, const ClipBlock b, float top_db, const int *__restrict__ max_key)
{
    float *dst = out + b.first;
    const float floor_db = key_float(max_key[blockIdx.x]) - top_db;
    for (unsigned long long g = static_cast<unsigned long long>(blockIdx.y) * 256 + threadIdx.x; g < b.n; g += static_cast<unsigned long long>(gridDim.y) * 256)
        dst[g] = fmaxf(dst[g], floor_db);
}
__global__ __launch_bounds__(256) void ss_db_floor_equal_kernel(float *__restrict__ out, unsigned long long seg, float top_db,
                                                               const int *__restrict__ max_key)
{
    db_floor_block(out, equal_block(seg), top_db, max_key);
}
__global__ __launch_bounds__(256) void ss_db_floor_varrows_kernel(float *__restrict__ out, const VarRowsArgs v, unsigned cols, float top_db,
                                                                 const int *__restrict__ max_key)
{
    db_floor_block(out, varrows_block(v, cols), top_db, max_key);
}
// the maxima's start value in every word: 0x80808080, below the key of every finite float (what ss_power_to_db_packed_device's memset
// writes) -- as a kernel, so that a captured call is a chain of kernel nodes only
__global__ __launch_bounds__(256) void ss_db_keys_init_kernel(int *__restrict__ max_key, unsigned n)
{
    const unsigned g = blockIdx.x * 256u + threadIdx.x;
    if (g < n) max_key[g] = static_cast<int>(0x80808080u);
}
// ss_power_to_db_packed_kernel's pass over equal-length clips, in place (behind a mel kernel that has no dB build)
__global__ __launch_bounds__(256) void ss_power_to_db_equal_kernel(float *x, unsigned long long seg, float amin, float ref_db, int *__restrict__ max_key)
{
    float *dst = x + blockIdx.x * seg;
    float mx = -INFINITY;
    for (unsigned long long g = static_cast<unsigned long long>(blockIdx.y) * 256 + threadIdx.x; g < seg; g += static_cast<unsigned long long>(gridDim.y) * 256) {
        const float db = power_db(dst[g], amin, ref_db);
        dst[g] = db;
        mx = fmaxf(mx, db);
    }
    if (max_key) {
        for (int m = 1; m < 64; m <<= 1) mx = fmaxf(mx, __shfl_xor(mx, m, 64));
        if ((threadIdx.x & 63) == 0 && mx > -INFINITY) atomicMax(max_key + blockIdx.x, float_key(mx));
    }
}

unsigned blocks_for(unsigned long long n) { return static_cast<unsigned>((n + 255) / 256); }

int check_shape(const void *a, const void *b, size_t batch, size_t rows, size_t cols)
{
    if (!a || !b) return fail(SS_ERR_ARG, "null buffer");
    if (rows == 0 || cols == 0) return fail(SS_ERR_ARG, "empty feature matrix");
    if (rows >= (1ull << 31) || cols >= (1ull << 31) || batch * rows * cols / 256 >= (1ull << 31)) return fail(SS_ERR_ARG, "feature block too large");
    return SS_OK;
}

// ---- packed clips: argument checks, grid shape ----

int check_packed(const void *a, const void *off, const void *b, size_t n_clips, size_t total_rows, size_t cols)
{
    if (!a || !off || !b) return fail(SS_ERR_ARG, "null buffer");
    if (cols == 0) return fail(SS_ERR_ARG, "empty feature matrix (cols == 0)");
    if (total_rows >= (1ull << 31) || cols >= (1ull << 31) || n_clips >= (1ull << 31)) return fail(SS_ERR_ARG, "feature block too large");
    return SS_OK;
}

// ---- causal CMVN over a pool of stream states: argument checks ----

// L = (win_size - 1) * cols + 1 floats per pool row; the count word is a float, so the window stays below 2^24 rows
int cmvn_stream_len(size_t cols, size_t win_size, size_t &len)
{
    if (cols == 0) return fail(SS_ERR_ARG, "empty feature matrix (cols == 0)");
    if (win_size == 0) return fail(SS_ERR_ARG, "win_size must be >= 1");
    if (cols >= (1ull << 31) || win_size > (1ull << 24) || (win_size - 1) * cols + 1 >= (1ull << 31))
        return fail(SS_ERR_ARG, "stream state too large: (win_size - 1) * cols + 1 must be below 2^31 and win_size at most 2^24");
    len = (win_size - 1) * cols + 1;
    return SS_OK;
}

// what both forms of ss_cmvn_stream_packed* reject before the device is touched (the tables apart)
int check_cmvn_stream(const float *vec, const void *ro, const void *slots, size_t n_active, size_t total_rows, size_t pool_streams, size_t cols,
                      size_t win_size, const float *pool, const float *out, size_t &len)
{
    if (!vec || !ro || !slots || !pool || !out) return fail(SS_ERR_ARG, "null buffer");
    const int rc = cmvn_stream_len(cols, win_size, len);
    if (rc) return rc;
    if (n_active >= (1ull << 31) || pool_streams >= (1ull << 31) || total_rows >= (1ull << 31))
        return fail(SS_ERR_ARG, "n_active, pool_streams and total_rows must be below 2^31");
    if (pool_streams == 0) return fail(SS_ERR_ARG, "the pool has no rows");
    const size_t bytes = total_rows * cols * sizeof(float), pbytes = pool_streams * len * sizeof(float);
    if (ranges_overlap(vec, bytes, out, bytes)) return fail(SS_ERR_ARG, "out overlaps vec: the call is not in place (later rows need the raw earlier rows)");
    if (ranges_overlap(pool, pbytes, vec, bytes) || ranges_overlap(pool, pbytes, out, bytes)) return fail(SS_ERR_ARG, "the pool overlaps vec or out");
    return SS_OK;
}

}  // namespace

// the dB step's launches (ss_device.h)
hipError_t launch_db_keys_init(int *max_key, size_t clips, hipStream_t stream)
{
    if (clips == 0) return hipSuccess;
    hipLaunchKernelGGL(ss_db_keys_init_kernel, dim3(blocks_for(clips)), dim3(256), 0, stream, max_key, static_cast<unsigned>(clips));
    return hipGetLastError();
}
hipError_t launch_db_floor_equal(float *out, size_t clips, size_t seg, float top_db, const int *max_key, hipStream_t stream)
{
    if (clips == 0 || seg == 0) return hipSuccess;
    const dim3 grid(static_cast<unsigned>(clips), packed_split(clips, (seg + 1023) / 1024));
    hipLaunchKernelGGL(ss_db_floor_equal_kernel, grid, dim3(256), 0, stream, out, static_cast<unsigned long long>(seg), top_db, max_key);
    return hipGetLastError();
}
hipError_t launch_db_floor_varrows(float *out, const VarRowsArgs &v, size_t cols, float top_db, const int *max_key, hipStream_t stream)
{
    if (v.n_clips == 0 || v.total_rows == 0) return hipSuccess;
    const dim3 grid(v.n_clips, packed_split(v.n_clips, (v.total_rows * cols + 1023) / 1024));
    hipLaunchKernelGGL(ss_db_floor_varrows_kernel, grid, dim3(256), 0, stream, out, v, static_cast<unsigned>(cols), top_db, max_key);
    return hipGetLastError();
}
hipError_t launch_power_to_db_equal(float *x, size_t clips, size_t seg, const DbArgs &db, hipStream_t stream)
{
    if (clips == 0 || seg == 0) return hipSuccess;
    const dim3 grid(static_cast<unsigned>(clips), packed_split(clips, (seg + 1023) / 1024));
    hipLaunchKernelGGL(ss_power_to_db_equal_kernel, grid, dim3(256), 0, stream, x, static_cast<unsigned long long>(seg), db.amin, db.ref_db, db.max_key);
    return hipGetLastError();
}

}  // namespace ss

extern "C" {

int ss_cmvn_batch_device(const float *d_vec, size_t batch, size_t rows, size_t cols, int variance_normalization, float *d_out,
                         void *stream)
{
    int rc = ss::check_shape(d_vec, d_out, batch, rows, cols);
    if (rc) return rc;
    if (batch == 0) return SS_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    // rows are summed in chunks (one thread per clip, chunk and column), then every element is normalised
    const unsigned chunks = static_cast<unsigned>(std::min<size_t>(64, (rows + 31) / 32));
    const unsigned rpc = static_cast<unsigned>((rows + chunks - 1) / chunks);
    const unsigned long long np = static_cast<unsigned long long>(batch) * chunks * cols;
    const unsigned long long n = static_cast<unsigned long long>(batch) * rows * cols;
    double *d_part = nullptr;
    hipError_t e = hipMallocAsync(reinterpret_cast<void **>(&d_part), np * 2 * sizeof(double), s);
    if (e != hipSuccess) return ss::hip_fail(e, "hipMallocAsync");
    hipLaunchKernelGGL(ss::ss_cmvn_partial_kernel, dim3(ss::blocks_for(np)), dim3(256), 0, s, d_vec, d_part, np, static_cast<unsigned>(rows),
                       static_cast<unsigned>(cols), chunks, rpc);
    hipLaunchKernelGGL(ss::ss_cmvn_apply_kernel, dim3(ss::blocks_for(n)), dim3(256), 0, s, d_vec, d_part, d_out, n, static_cast<unsigned>(rows),
                       static_cast<unsigned>(cols), chunks, variance_normalization);
    e = hipFreeAsync(d_part, s);
    if (e != hipSuccess) return ss::hip_fail(e, "hipFreeAsync");
    e = hipGetLastError();
    return e == hipSuccess ? SS_OK : ss::hip_fail(e, "ss_cmvn kernels");
}

int ss_cmvnw_batch_device(const float *d_vec, size_t batch, size_t rows, size_t cols, size_t win_size, int variance_normalization,
                          float *d_out, void *stream)
{
    int rc = ss::check_shape(d_vec, d_out, batch, rows, cols);
    if (rc) return rc;
    if (win_size % 2 != 1) return ss::fail(SS_ERR_BAD_CONFIG, "Windows size must be odd!");  // assert, processing.rs:327
    if (win_size >= (1ull << 31)) return ss::fail(SS_ERR_ARG, "window too large");
    if (batch == 0) return SS_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const unsigned r = static_cast<unsigned>(rows), c = static_cast<unsigned>(cols), w = static_cast<unsigned>(win_size);
    // a thread slides the window over a chunk of rows: chunks long enough to amortise the first window sum
    const unsigned rpc = static_cast<unsigned>(std::min<size_t>(256, std::max<size_t>(8, (win_size + 15) / 16)));
    const unsigned chunks = (r + rpc - 1) / rpc;
    const unsigned long long nt = static_cast<unsigned long long>(batch) * chunks * cols;
    const unsigned long long n = static_cast<unsigned long long>(batch) * rows * cols;
    if (!variance_normalization) {
        hipLaunchKernelGGL(ss::ss_cmvnw_mean_kernel, dim3(ss::blocks_for(nt)), dim3(256), 0, s, d_vec, d_out, nt, r, c, w, chunks, rpc);
    } else {
        // the second pass reads its neighbours' mean-subtracted values: they go through a stream-ordered scratch block
        float *d_ms = nullptr;
        hipError_t e = hipMallocAsync(reinterpret_cast<void **>(&d_ms), n * sizeof(float), s);
        if (e != hipSuccess) return ss::hip_fail(e, "hipMallocAsync");
        hipLaunchKernelGGL(ss::ss_cmvnw_mean_kernel, dim3(ss::blocks_for(nt)), dim3(256), 0, s, d_vec, d_ms, nt, r, c, w, chunks, rpc);
        hipLaunchKernelGGL(ss::ss_cmvnw_var_kernel, dim3(ss::blocks_for(nt)), dim3(256), 0, s, d_ms, d_out, nt, r, c, w, chunks, rpc);
        e = hipFreeAsync(d_ms, s);
        if (e != hipSuccess) return ss::hip_fail(e, "hipFreeAsync");
    }
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? SS_OK : ss::hip_fail(e, "ss_cmvnw kernels");
}

int ss_derivative_extraction_device(const float *d_feat, size_t rows, size_t cols, size_t delta_windows, float *d_out, void *stream)
{
    int rc = ss::check_shape(d_feat, d_out, 1, rows, cols);
    if (rc) return rc;
    if (delta_windows == 0 || delta_windows >= (1u << 20)) return ss::fail(SS_ERR_ARG, "delta_windows must be >= 1");  // scale = 0 in the reference
    double scale = 0.0;
    for (size_t R = 1; R <= delta_windows; ++R) scale += 2.0 * static_cast<double>(R) * static_cast<double>(R);
    const unsigned long long n = static_cast<unsigned long long>(rows) * cols;
    hipLaunchKernelGGL(ss::ss_derivative_kernel, dim3(ss::blocks_for(n)), dim3(256), 0, static_cast<hipStream_t>(stream), d_feat, d_out, n,
                       static_cast<unsigned>(cols), static_cast<unsigned>(delta_windows), static_cast<float>(1.0 / scale));
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? SS_OK : ss::hip_fail(e, "ss_derivative_kernel");
}

int ss_extract_derivative_feature_device(const float *d_feat, size_t rows, size_t cols, float *d_cube, void *stream)
{
    int rc = ss::check_shape(d_feat, d_cube, 1, rows, cols);
    if (rc) return rc;
    const unsigned long long n = static_cast<unsigned long long>(rows) * cols;
    hipLaunchKernelGGL(ss::ss_derivative_cube_kernel, dim3(ss::blocks_for(n)), dim3(256), 0, static_cast<hipStream_t>(stream), d_feat, d_cube,
                       n, static_cast<unsigned>(cols));
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? SS_OK : ss::hip_fail(e, "ss_derivative_cube_kernel");
}

// ---- host-pointer variants (synchronous) ----

int ss_cmvn(const float *vec, size_t rows, size_t cols, int variance_normalization, float *out)
{
    int rc = ss::check_shape(vec, out, 1, rows, cols);
    if (rc) return rc;
    if (!ss::have_device()) return ss::no_device();
    ss::HostStage st("ss_cmvn");
    const float *d_in = st.up(vec, rows * cols * sizeof(float));
    float *d_out = st.room<float>(rows * cols * sizeof(float));
    if (st.ok()) st.ran(ss_cmvn_batch_device(d_in, 1, rows, cols, variance_normalization, d_out, nullptr));
    st.sync();
    st.down(out, d_out, rows * cols * sizeof(float));
    return st.status();
}

int ss_cmvnw(const float *vec, size_t rows, size_t cols, size_t win_size, int variance_normalization, float *out)
{
    int rc = ss::check_shape(vec, out, 1, rows, cols);
    if (rc) return rc;
    if (win_size % 2 != 1) return ss::fail(SS_ERR_BAD_CONFIG, "Windows size must be odd!");
    if (!ss::have_device()) return ss::no_device();
    ss::HostStage st("ss_cmvnw");
    const float *d_in = st.up(vec, rows * cols * sizeof(float));
    float *d_out = st.room<float>(rows * cols * sizeof(float));
    if (st.ok()) st.ran(ss_cmvnw_batch_device(d_in, 1, rows, cols, win_size, variance_normalization, d_out, nullptr));
    st.sync();
    st.down(out, d_out, rows * cols * sizeof(float));
    return st.status();
}

int ss_derivative_extraction(const float *feat, size_t rows, size_t cols, size_t delta_windows, float *out)
{
    int rc = ss::check_shape(feat, out, 1, rows, cols);
    if (rc) return rc;
    if (delta_windows == 0) return ss::fail(SS_ERR_ARG, "delta_windows must be >= 1");
    if (!ss::have_device()) return ss::no_device();
    ss::HostStage st("ss_derivative_extraction");
    const float *d_in = st.up(feat, rows * cols * sizeof(float));
    float *d_out = st.room<float>(rows * cols * sizeof(float));
    if (st.ok()) st.ran(ss_derivative_extraction_device(d_in, rows, cols, delta_windows, d_out, nullptr));
    st.sync();
    st.down(out, d_out, rows * cols * sizeof(float));
    return st.status();
}

int ss_extract_derivative_feature(const float *feat, size_t rows, size_t cols, float *cube)
{
    int rc = ss::check_shape(feat, cube, 1, rows, cols);
    if (rc) return rc;
    if (!ss::have_device()) return ss::no_device();
    ss::HostStage st("ss_extract_derivative_feature");
    const float *d_in = st.up(feat, rows * cols * sizeof(float));
    float *d_out = st.room<float>(3 * rows * cols * sizeof(float));
    if (st.ok()) st.ran(ss_extract_derivative_feature_device(d_in, rows, cols, d_out, nullptr));
    st.sync();
    st.down(cube, d_out, 3 * rows * cols * sizeof(float));
    return st.status();
}

int ss_ln_device(float *d_x, size_t n, void *stream)
{
    if (n == 0) return SS_OK;
    if (!d_x) return ss::fail(SS_ERR_ARG, "null buffer");
    hipLaunchKernelGGL(ss::ss_ln_kernel, dim3(ss::blocks_for(n)), dim3(256), 0, static_cast<hipStream_t>(stream), d_x, static_cast<unsigned long long>(n));
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? SS_OK : ss::hip_fail(e, "ss_ln_kernel");
}

int ss_power_to_db_device(const float *d_s, size_t n, float ref, float amin, float top_db, float *d_out, void *stream)
{
    if (n == 0) return SS_OK;
    if (!d_s || !d_out) return ss::fail(SS_ERR_ARG, "null buffer");
    if (!(amin > 0.0f)) return ss::fail(SS_ERR_ARG, "amin must be strictly positive");  // librosa.power_to_db raises the same
    if (ref != ref) return ss::fail(SS_ERR_ARG, "ref must not be NaN");  // |ref| is used, as in librosa (np.abs(ref))
    hipStream_t st = static_cast<hipStream_t>(stream);
    const float ref_db = 10.0f * std::log10(std::max(amin, std::fabs(ref)));
    int *d_max = nullptr;
    if (top_db >= 0.0f) {
        hipError_t e = hipMallocAsync(reinterpret_cast<void **>(&d_max), sizeof(int), st);
        if (e != hipSuccess) return ss::hip_fail(e, "hipMallocAsync");
        e = hipMemsetAsync(d_max, 0x80, sizeof(int), st);  // 0x80808080: below the key of every finite float
        if (e != hipSuccess) return ss::hip_fail(e, "hipMemsetAsync");
    }
    hipLaunchKernelGGL(ss::ss_power_to_db_kernel, dim3(ss::blocks_for(n)), dim3(256), 0, st, d_s, d_out, static_cast<unsigned long long>(n), amin,
                       ref_db, d_max);
    if (d_max) {
        hipLaunchKernelGGL(ss::ss_db_floor_kernel, dim3(ss::blocks_for(n)), dim3(256), 0, st, d_out, static_cast<unsigned long long>(n), top_db, d_max);
        const hipError_t e = hipFreeAsync(d_max, st);
        if (e != hipSuccess) return ss::hip_fail(e, "hipFreeAsync");
    }
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? SS_OK : ss::hip_fail(e, "ss_power_to_db kernels");
}

int ss_power_to_db(const float *s, size_t n, float ref, float amin, float top_db, float *out)
{
    if (n == 0) return SS_OK;
    if (!s || !out) return ss::fail(SS_ERR_ARG, "null buffer");
    if (!ss::have_device()) return ss::no_device();
    ss::HostStage st("ss_power_to_db");
    const float *d_in = st.up(s, n * sizeof(float));
    float *d_out = st.room<float>(n * sizeof(float));
    if (st.ok()) st.ran(ss_power_to_db_device(d_in, n, ref, amin, top_db, d_out, nullptr));
    st.sync();
    st.down(out, d_out, n * sizeof(float));
    return st.status();
}

// ---- packed variable-length clips: clip b owns rows offsets[b] .. offsets[b+1] of the [total_rows x cols] block ----

int ss_cmvn_packed_device(const float *d_vec, size_t n_clips, const int64_t *d_offsets, size_t total_rows, size_t cols,
                          int variance_normalization, float *d_out, void *stream)
{
    if (n_clips == 0) return SS_OK;
    int rc = ss::check_packed(d_vec, d_offsets, d_out, n_clips, total_rows, cols);
    if (rc) return rc;
    if (total_rows == 0) return SS_OK;
    const unsigned split = ss::packed_split(n_clips, (total_rows + ss::kCmvnSplitRows - 1) / ss::kCmvnSplitRows);
    hipLaunchKernelGGL(ss::ss_cmvn_packed_kernel, dim3(static_cast<unsigned>(n_clips), split), dim3(256), 0, static_cast<hipStream_t>(stream), d_vec,
                       reinterpret_cast<const long long *>(d_offsets), d_out, static_cast<unsigned long long>(total_rows), static_cast<unsigned>(cols),
                       variance_normalization);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? SS_OK : ss::hip_fail(e, "ss_cmvn_packed_kernel");
}

int ss_cmvnw_packed_device(const float *d_vec, size_t n_clips, const int64_t *d_offsets, size_t total_rows, size_t cols, size_t win_size,
                           int variance_normalization, float *d_out, void *stream)
{
    if (n_clips == 0) return SS_OK;
    int rc = ss::check_packed(d_vec, d_offsets, d_out, n_clips, total_rows, cols);
    if (rc) return rc;
    if (win_size % 2 != 1) return ss::fail(SS_ERR_BAD_CONFIG, "Windows size must be odd!");  // assert, processing.rs:327
    if (win_size >= (1ull << 31)) return ss::fail(SS_ERR_ARG, "window too large");
    if (total_rows == 0) return SS_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const unsigned c = static_cast<unsigned>(cols), w = static_cast<unsigned>(win_size);
    const unsigned long long tr = total_rows;
    const long long *off = reinterpret_cast<const long long *>(d_offsets);
    const unsigned rpc = static_cast<unsigned>(std::min<size_t>(256, std::max<size_t>(8, (win_size + 15) / 16)));  // as ss_cmvnw_batch_device
    const unsigned split = ss::packed_split(n_clips, ((tr + rpc - 1) / rpc * cols + 255) / 256);
    const dim3 grid(static_cast<unsigned>(n_clips), split);
    if (!variance_normalization) {
        hipLaunchKernelGGL(ss::ss_cmvnw_packed_kernel<false>, grid, dim3(256), 0, s, d_vec, off, d_out, tr, c, w, rpc);
    } else {
        // the second pass reads its neighbours' mean-subtracted values: they go through a stream-ordered scratch block
        float *d_ms = nullptr;
        hipError_t e = hipMallocAsync(reinterpret_cast<void **>(&d_ms), total_rows * cols * sizeof(float), s);
        if (e != hipSuccess) return ss::hip_fail(e, "hipMallocAsync");
        hipLaunchKernelGGL(ss::ss_cmvnw_packed_kernel<false>, grid, dim3(256), 0, s, d_vec, off, d_ms, tr, c, w, rpc);
        hipLaunchKernelGGL(ss::ss_cmvnw_packed_kernel<true>, grid, dim3(256), 0, s, d_ms, off, d_out, tr, c, w, rpc);
        e = hipFreeAsync(d_ms, s);
        if (e != hipSuccess) return ss::hip_fail(e, "hipFreeAsync");
    }
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? SS_OK : ss::hip_fail(e, "ss_cmvnw_packed kernels");
}

int ss_power_to_db_packed_device(const float *d_s, size_t n_clips, const int64_t *d_offsets, size_t total_rows, size_t cols, float ref,
                                 float amin, float top_db, float *d_out, void *stream)
{
    if (n_clips == 0) return SS_OK;
    int rc = ss::check_packed(d_s, d_offsets, d_out, n_clips, total_rows, cols);
    if (rc) return rc;
    if (!(amin > 0.0f)) return ss::fail(SS_ERR_ARG, "amin must be strictly positive");
    if (ref != ref) return ss::fail(SS_ERR_ARG, "ref must not be NaN");
    if (total_rows == 0) return SS_OK;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const float ref_db = 10.0f * std::log10(std::max(amin, std::fabs(ref)));
    const unsigned long long tr = total_rows;
    const long long *off = reinterpret_cast<const long long *>(d_offsets);
    const dim3 grid(static_cast<unsigned>(n_clips), ss::packed_split(n_clips, (tr * cols + 1023) / 1024));
    int *d_max = nullptr;  // one ordered-integer maximum per clip
    if (top_db >= 0.0f) {
        hipError_t e = hipMallocAsync(reinterpret_cast<void **>(&d_max), n_clips * sizeof(int), st);
        if (e != hipSuccess) return ss::hip_fail(e, "hipMallocAsync");
        e = hipMemsetAsync(d_max, 0x80, n_clips * sizeof(int), st);  // 0x80808080: below the key of every finite float
        if (e != hipSuccess) return ss::hip_fail(e, "hipMemsetAsync");
    }
    hipLaunchKernelGGL(ss::ss_power_to_db_packed_kernel, grid, dim3(256), 0, st, d_s, off, d_out, tr, static_cast<unsigned>(cols), amin, ref_db, d_max);
    if (d_max) {
        hipLaunchKernelGGL(ss::ss_db_floor_packed_kernel, grid, dim3(256), 0, st, d_out, off, tr, static_cast<unsigned>(cols), top_db, d_max);
        const hipError_t e = hipFreeAsync(d_max, st);
        if (e != hipSuccess) return ss::hip_fail(e, "hipFreeAsync");
    }
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? SS_OK : ss::hip_fail(e, "ss_power_to_db_packed kernels");
}

// host-pointer forms (synchronous): the table is checked on the host before the device is touched

int ss_cmvn_packed(const float *vec, size_t n_clips, const int64_t *offsets, size_t total_rows, size_t cols, int variance_normalization,
                   float *out)
{
    if (n_clips == 0) return SS_OK;
    int rc = ss::check_packed(vec, offsets, out, n_clips, total_rows, cols);
    if (rc || (rc = ss::check_clip_table(offsets, n_clips, total_rows))) return rc;
    if (offsets[n_clips] == 0) return SS_OK;
    if (!ss::have_device()) return ss::no_device();
    const size_t bytes = total_rows * cols * sizeof(float);
    ss::HostStage st("packed post-processing");
    const float *d_in = st.up(vec, bytes);
    const int64_t *d_off = st.up(offsets, (n_clips + 1) * sizeof(int64_t));
    float *d_out = st.room<float>(bytes);
    if (st.ok()) st.ran(ss_cmvn_packed_device(d_in, n_clips, d_off, total_rows, cols, variance_normalization, d_out, nullptr));
    st.sync();
    st.down(out, d_out, static_cast<size_t>(offsets[n_clips]) * cols * sizeof(float));  // the rows the table covers
    return st.status();
}

int ss_cmvnw_packed(const float *vec, size_t n_clips, const int64_t *offsets, size_t total_rows, size_t cols, size_t win_size,
                    int variance_normalization, float *out)
{
    if (n_clips == 0) return SS_OK;
    int rc = ss::check_packed(vec, offsets, out, n_clips, total_rows, cols);
    if (rc) return rc;
    if (win_size % 2 != 1) return ss::fail(SS_ERR_BAD_CONFIG, "Windows size must be odd!");
    if (win_size >= (1ull << 31)) return ss::fail(SS_ERR_ARG, "window too large");
    if ((rc = ss::check_clip_table(offsets, n_clips, total_rows))) return rc;
    if (offsets[n_clips] == 0) return SS_OK;
    if (!ss::have_device()) return ss::no_device();
    const size_t bytes = total_rows * cols * sizeof(float);
    ss::HostStage st("packed post-processing");
    const float *d_in = st.up(vec, bytes);
    const int64_t *d_off = st.up(offsets, (n_clips + 1) * sizeof(int64_t));
    float *d_out = st.room<float>(bytes);
    if (st.ok()) st.ran(ss_cmvnw_packed_device(d_in, n_clips, d_off, total_rows, cols, win_size, variance_normalization, d_out, nullptr));
    st.sync();
    st.down(out, d_out, static_cast<size_t>(offsets[n_clips]) * cols * sizeof(float));  // the rows the table covers
    return st.status();
}

int ss_power_to_db_packed(const float *s, size_t n_clips, const int64_t *offsets, size_t total_rows, size_t cols, float ref, float amin,
                          float top_db, float *out)
{
    if (n_clips == 0) return SS_OK;
    int rc = ss::check_packed(s, offsets, out, n_clips, total_rows, cols);
    if (rc) return rc;
    if (!(amin > 0.0f)) return ss::fail(SS_ERR_ARG, "amin must be strictly positive");
    if (ref != ref) return ss::fail(SS_ERR_ARG, "ref must not be NaN");
    if ((rc = ss::check_clip_table(offsets, n_clips, total_rows))) return rc;
    if (offsets[n_clips] == 0) return SS_OK;
    if (!ss::have_device()) return ss::no_device();
    const size_t bytes = total_rows * cols * sizeof(float);
    ss::HostStage st("packed post-processing");
    const float *d_in = st.up(s, bytes);
    const int64_t *d_off = st.up(offsets, (n_clips + 1) * sizeof(int64_t));
    float *d_out = st.room<float>(bytes);
    if (st.ok()) st.ran(ss_power_to_db_packed_device(d_in, n_clips, d_off, total_rows, cols, ref, amin, top_db, d_out, nullptr));
    st.sync();
    st.down(out, d_out, static_cast<size_t>(offsets[n_clips]) * cols * sizeof(float));  // the rows the table covers
    return st.status();
}

// ---- causal sliding-window CMVN over a pool of stream states: entry i owns rows ro[i] .. ro[i+1] and pool row slots[i] ----

int ss_cmvn_stream_state_len(size_t cols, size_t win_size, size_t *state_len)
{
    if (!state_len) return ss::fail(SS_ERR_ARG, "null output");
    size_t len = 0;
    const int rc = ss::cmvn_stream_len(cols, win_size, len);
    if (rc) return rc;
    *state_len = len;
    return SS_OK;
}

int ss_cmvn_stream_packed_device(const float *d_vec, size_t n_active, const int64_t *d_row_offsets, size_t total_rows, const int32_t *d_slots,
                                 size_t pool_streams, size_t cols, size_t win_size, int variance_normalization, float *d_pool, float *d_out,
                                 void *stream)
{
    if (n_active == 0) return SS_OK;
    size_t len = 0;
    const int rc = ss::check_cmvn_stream(d_vec, d_row_offsets, d_slots, n_active, total_rows, pool_streams, cols, win_size, d_pool, d_out, len);
    if (rc) return rc;
    if (total_rows == 0) return SS_OK;  // no entry can own a row
    // one launch, one workgroup per entry: the grid depends on n_active only
    hipLaunchKernelGGL(ss::ss_cmvn_stream_packed_kernel, dim3(static_cast<unsigned>(n_active)), dim3(256), 0, static_cast<hipStream_t>(stream), d_vec,
                       reinterpret_cast<const long long *>(d_row_offsets), reinterpret_cast<const int *>(d_slots), d_out, d_pool,
                       static_cast<unsigned long long>(total_rows), static_cast<unsigned>(pool_streams), static_cast<unsigned>(cols),
                       static_cast<unsigned>(win_size), variance_normalization);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? SS_OK : ss::hip_fail(e, "ss_cmvn_stream_packed_kernel");
}

// Host-pointer form: the tables are checked here, before anything touches the device; then vec, the row offsets and the n_active
// named pool rows (gathered into a compact block whose row i is entry i's: the device call runs on slots 0 .. n_active - 1) go
// up, out and the named rows come down.  The caller's pool is written only once everything before it succeeded.
int ss_cmvn_stream_packed(const float *vec, size_t n_active, const int64_t *row_offsets, const int32_t *slots, size_t pool_streams, size_t cols,
                          size_t win_size, int variance_normalization, float *pool, float *out)
{
    if (n_active == 0) return SS_OK;
    if (!row_offsets) return ss::fail(SS_ERR_ARG, "null buffer");
    if (n_active >= (1ull << 31)) return ss::fail(SS_ERR_ARG, "n_active, pool_streams and total_rows must be below 2^31");
    int rc = ss::check_row_offsets(row_offsets, n_active);
    if (rc) return rc;
    const size_t rows = static_cast<size_t>(row_offsets[n_active]);
    size_t len = 0;
    if ((rc = ss::check_cmvn_stream(vec, row_offsets, slots, n_active, rows, pool_streams, cols, win_size, pool, out, len)) ||
        (rc = ss::check_slots(slots, n_active, pool_streams)))
        return rc;
    if (rows == 0) return SS_OK;  // entries without rows only: nothing moves
    if (!ss::have_device()) return ss::no_device();
    ss::PoolRows named;
    named.gather(pool, slots, n_active, len);
    const size_t bytes = rows * cols * sizeof(float);
    ss::HostStage st("ss_cmvn_stream_packed");
    const float *d_vec = st.up(vec, bytes);
    float *d_out = st.room<float>(bytes);
    const int64_t *d_ro = st.up(row_offsets, (n_active + 1) * sizeof(int64_t));
    const auto d_named = st.up_pool(named);
    if (st.ok())
        st.ran(ss_cmvn_stream_packed_device(d_vec, n_active, d_ro, rows, d_named.slots, n_active, cols, win_size, variance_normalization, d_named.rows,
                                            d_out, nullptr));
    st.sync();
    st.down_pool(named, d_named);
    st.down(out, d_out, bytes);
    st.scatter(named, pool, slots);
    return st.status();
}

}  // extern "C"
