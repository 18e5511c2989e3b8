// Time-axis delta features (Kaldi's add-deltas): ss_add_deltas_packed* on packed variable-length clips, and
// ss_add_deltas_stream_packed* / ss_add_deltas_stream_flush* over a pool of stream states with a fixed latency of L = order * window
// rows.  The definition (include/speechsauce_amd.h) is a fixed-order f64 sum of integer taps times f32 values: every product is
// exact, so an output's bits depend on the values under its taps and on nothing else -- not on the tile it was computed in, the
// clip's place in the block, the entry's place in the call or how a stream was cut into calls.
// The reference crate differences along the feature axis (processing.rs:222-254, ss_derivative_extraction* in ss_post.hip); it has
// no time-axis counterpart, so this file restates nothing of it.
#include "ss_device.h"
#include "ss_hip_staging.h"
#include "ss_host_checks.h"
#include "ss_internal.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

namespace ss {

namespace {

constexpr unsigned kMaxLag = 32;               // L = order * window
constexpr unsigned kMaxTaps = 2 * kMaxLag + 1;

// what the host knows about one call: the non-zero taps of every order in ascending j -- their row offsets and their values as
// doubles (small integers, exact) -- and 1 / D_o.  Zero taps are not in the list at all, so the walk has no branch (the loads of
// several taps are in flight together) and a NaN under a zero tap is never read.
struct DeltaTaps {
    double k[2][kMaxTaps];  // k[o - 1][i]: the i-th non-zero tap of order o
    int off[2][kMaxTaps];   // its row offset j, -o * window .. +o * window, ascending
    double inv[2];          // 1.0 / D_o
    unsigned n[2];          // non-zero taps of order o
    unsigned order;         // 1 or 2
    unsigned lag;           // L = order * window
};

// d_o of one element: `p` points at the centre row's value, rows are `stride` floats apart and every row under a tap is readable
// (the caller has resolved the clamping).  One f64 accumulator, ascending j.
__device__ __forceinline__ float delta_at(const float *p, int stride, const DeltaTaps &tp, unsigned o)
{
    const unsigned n = tp.n[o];
    double acc = 0.0;
#pragma unroll 4
    for (unsigned i = 0; i < n; ++i) acc = acc + tp.k[o][i] * static_cast<double>(p[tp.off[o][i] * stride]);
    return static_cast<float>(acc * tp.inv[o]);
}

// ---- packed clips ----
// Clip b owns rows off[b] .. off[b+1].  Workgroup (b, y) takes the row tiles y, y + gridDim.y, ... of clip b: a tile of kRowTile
// rows plus L halo rows on either side (indices clamped to the clip's own first and last row while staging: edge replication of
// the raw rows) goes to LDS once per 32-column tile, columns fastest; every element then walks its taps there.  (packed_segment:
// ss_device.h)
constexpr unsigned kRowTile = 64;                          // output rows per tile
constexpr unsigned kColTile = 32;                          // columns staged at a time
constexpr unsigned kTileRows = kRowTile + 2 * kMaxLag;     // staged rows at the largest lag: 128 x 32 floats = 16 KiB

__global__ __launch_bounds__(256) void ss_add_deltas_packed_kernel(const float *__restrict__ x, const long long *__restrict__ off, float *__restrict__ out,
                                                                  unsigned long long total_rows, unsigned cols, const DeltaTaps tp)
{
    __shared__ float tile[kTileRows * kColTile];
    const Segment seg = packed_segment(off, total_rows);
    if (seg.rows == 0) return;
    const unsigned rows = seg.rows, L = tp.lag;
    const size_t ocols = static_cast<size_t>(tp.order + 1) * cols;  // cols < 2^31, order 2: three times that does not fit 32 bits
    const unsigned n_tiles = (rows + kRowTile - 1) / kRowTile;
    const float *src = x + seg.row0 * cols;
    float *dst = out + seg.row0 * ocols;
    for (unsigned rt = blockIdx.y; rt < n_tiles; rt += gridDim.y) {  // uniform per workgroup
        const unsigned r0 = rt * kRowTile, tr = min(kRowTile, rows - r0);
        const unsigned staged_rows = tr + 2 * L;
        for (unsigned c0 = 0; c0 < cols; c0 += kColTile) {
            const unsigned ct = min(kColTile, cols - c0);
            for (unsigned i = threadIdx.x; i < staged_rows * ct; i += 256) {
                const unsigned s = i / ct, c = i - s * ct;
                const long long r = static_cast<long long>(r0) + s - L;  // the clip's row under staged row s, clamped to the clip
                const unsigned rc = r < 0 ? 0u : static_cast<unsigned>(min(r, static_cast<long long>(rows) - 1));
                tile[i] = src[static_cast<size_t>(rc) * cols + c0 + c];
            }
            __syncthreads();
            for (unsigned k = threadIdx.x; k < tr * ct; k += 256) {  // task = (row, column), columns fastest
                const unsigned t = k / ct, c = k - t * ct;
                const float *p = tile + (t + L) * ct + c;
                float *o = dst + static_cast<size_t>(r0 + t) * ocols + c0 + c;
                o[0] = *p;
                for (unsigned d = 0; d < tp.order; ++d) o[static_cast<size_t>(d + 1) * cols] = delta_at(p, ct, tp, d);
            }
            __syncthreads();  // the next tile overwrites the staged rows
        }
    }
}

// ---- pool of stream states ----
// Entry i owns rows ro[i] .. ro[i+1] of the blocks and pool row slots[i]: len = 2L * cols + 1 floats, the last 2L raw rows of its
// stream (oldest first, right-aligned, zeros in front) and, in the last float, how many of them are valid.  The stream's rows are
// counted from the oldest valid history row: 0 .. count - 1 the history, count .. count + rows - 1 the entry's.  Where count < 2L
// the history is the whole stream, so row 0 is stream row 0 and clamping there is the definition's; where count == 2L no tap
// reaches below row 0.  Output row k is centred on row v = count + k - L (v < 0: a warm-up row of zeros); its last tap is row
// count + k, which has just arrived.  The flush build has no new rows: it writes the L rows centred on count - L .. count - 1,
// clamped at the stream's last row, and zeroes the pool row.  (RowPoolEntry, row_pool_entry: ss_device.h)
constexpr unsigned kStreamRows = 128;  // rows (history + new) an entry may stage per column tile: 128 x 32 floats = 16 KiB
constexpr unsigned kStreamMove = 4;    // pool-row floats a thread moves per step of the advance in global memory

__device__ __forceinline__ void zero_row(float *o, unsigned cols, unsigned order)
{
    for (unsigned d = 0; d <= order; ++d) o[static_cast<size_t>(d) * cols] = 0.0f;
}

// d_o of the element of column c centred on row v (>= 0) where the rows live in two global blocks: rows below `count` in the history
// (`old`), the others in the entry's rows (`src`); the index is clamped to 0 .. last
__device__ __forceinline__ float delta_split(const float *old, const float *src, unsigned count, unsigned cols, unsigned c, long long v, long long last,
                                             const DeltaTaps &tp, unsigned o)
{
    const unsigned n = tp.n[o];
    double acc = 0.0;
#pragma unroll 4
    for (unsigned i = 0; i < n; ++i) {
        const long long r = min(max(v + tp.off[o][i], 0ll), last);
        const float xv = r < static_cast<long long>(count) ? old[static_cast<size_t>(r) * cols + c] : src[static_cast<size_t>(r - count) * cols + c];
        acc = acc + tp.k[o][i] * static_cast<double>(xv);
    }
    return static_cast<float>(acc * tp.inv[o]);
}

template <bool FLUSH>
__global__ __launch_bounds__(256) void ss_add_deltas_stream_kernel(const float *__restrict__ x, const long long *__restrict__ ro,
                                                                  const int *__restrict__ slots, float *__restrict__ out, float *pool,
                                                                  unsigned long long total_rows, unsigned pool_streams, unsigned cols, const DeltaTaps tp)
{
    __shared__ float tile[kStreamRows * kColTile];
    // 32 bits hold both: the host refuses a state length 2 L * cols + 1 >= 2^31 (stream_len), so cols < 2^30 / L and, with L >= order,
    // ocols = (order + 1) * cols < 2^31 -- unlike the packed kernel, whose cols is bounded by 2^31 alone
    const unsigned L = tp.lag, hist = 2 * L, state_len = hist * cols + 1, ocols = (tp.order + 1) * cols;
    const RowPoolEntry e = row_pool_entry<FLUSH>(ro, slots, total_rows, pool_streams, pool, state_len, hist, L);
    if (!e.state || (!FLUSH && e.rows == 0)) return;  // the whole workgroup: the pool row stays as it is
    const unsigned rows = e.rows, count = e.count;
    const unsigned n_out = FLUSH ? L : rows;
    const float *src = x + (FLUSH ? 0 : e.row0 * cols);  // the flush build never reads it: every row it sees is history
    float *dst = out + e.row0 * ocols;
    const float *old = e.state + static_cast<size_t>(hist - count) * cols;  // the oldest valid history row
    const unsigned long long span = static_cast<unsigned long long>(count) + rows;  // rows the entry can see
    const long long last = static_cast<long long>(span) - 1;                     // the clamp on the right (reached by the flush only)
    const long long lead = static_cast<long long>(hist) - static_cast<long long>(span);  // rows of zeros in front of the new pool row (<= 0: none)
    if (FLUSH || span <= kStreamRows) {  // (the flush's span is at most 2L <= 64 rows)
        // the usual tick: per column tile the history and the new rows go to LDS once, every element walks its taps there, and the
        // tile's share of the new pool row is written from LDS (nothing of the pool row is read after it was written)
        const unsigned sp = static_cast<unsigned>(span);
        for (unsigned c0 = 0; c0 < cols; c0 += kColTile) {
            const unsigned ct = min(kColTile, cols - c0);
            for (unsigned i = threadIdx.x; i < sp * ct; i += 256) {
                const unsigned j = i / ct, c = i - j * ct;
                if (FLUSH || j < count) tile[i] = old[static_cast<size_t>(j) * cols + c0 + c];
                else tile[i] = src[static_cast<size_t>(j - count) * cols + c0 + c];
            }
            __syncthreads();
            for (unsigned k = threadIdx.x; k < n_out * ct; k += 256) {  // task = (row, column), columns fastest
                const unsigned t = k / ct, c = k - t * ct;
                const long long v = static_cast<long long>(count) + t - L;
                float *o = dst + static_cast<size_t>(t) * ocols + c0 + c;
                if (v < 0) {
                    zero_row(o, cols, tp.order);
                } else if (v >= static_cast<long long>(L) && v + L <= last) {  // no clamp: walk the staged rows as they are
                    const float *p = tile + static_cast<unsigned>(v) * ct + c;
                    o[0] = *p;
                    for (unsigned d = 0; d < tp.order; ++d) o[static_cast<size_t>(d + 1) * cols] = delta_at(p, ct, tp, d);
                } else {  // a stream's first L rows, and the flush: the same walk with the index clamped
                    o[0] = tile[static_cast<unsigned>(v) * ct + c];
                    for (unsigned d = 0; d < tp.order; ++d) o[static_cast<size_t>(d + 1) * cols] = delta_split(tile + c, tile + c, 0, ct, 0, v, last, tp, d);
                }
            }
            if (!FLUSH) {
                for (unsigned i = threadIdx.x; i < hist * ct; i += 256) {
                    const unsigned r = i / ct, c = i - r * ct;
                    const long long j = static_cast<long long>(r) - lead;
                    e.state[static_cast<size_t>(r) * cols + c0 + c] = j >= 0 ? tile[static_cast<unsigned>(j) * ct + c] : 0.0f;
                }
            }
            __syncthreads();  // the next column tile overwrites the staged rows
        }
    } else if constexpr (!FLUSH) {
        // a long catch-up entry: the same walk, in the same order, in global memory
        const unsigned long long tasks = static_cast<unsigned long long>(n_out) * cols;
        for (unsigned long long k = threadIdx.x; k < tasks; k += 256) {
            const unsigned t = static_cast<unsigned>(k / cols);
            const unsigned c = static_cast<unsigned>(k - static_cast<unsigned long long>(t) * cols);
            const long long v = static_cast<long long>(count) + t - L;
            float *o = dst + static_cast<size_t>(t) * ocols + c;
            if (v < 0) {
                zero_row(o, cols, tp.order);
            } else {
                o[0] = v < static_cast<long long>(count) ? old[static_cast<size_t>(v) * cols + c] : src[static_cast<size_t>(v - count) * cols + c];
                for (unsigned d = 0; d < tp.order; ++d) o[static_cast<size_t>(d + 1) * cols] = delta_split(old, src, count, cols, c, v, last, tp, d);
            }
        }
        // A history row moves towards the front of the pool row it is read from, so the row is rewritten in ascending steps of
        // 256 * kStreamMove floats, every step read in full before it is written: a later step reads only what lies behind
        // everything written so far.  (The first step's barrier also ends every thread's walk above.)
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
    }
    if (FLUSH) {
        // every read of the pool row lies before the last barrier above: the stream is fresh from here on
        for (unsigned i = threadIdx.x; i < state_len; i += 256) e.state[i] = 0.0f;
    } else {
        if (threadIdx.x == 0) e.state[state_len - 1] = static_cast<float>(min(span, static_cast<unsigned long long>(hist)));
    }
}

// ---- host side ----

// order / window -> the integer taps of every order by repeated convolution with [-window .. window] (the non-zero ones kept), and 1 / D_o
int make_taps(size_t order, size_t window, DeltaTaps &tp)
{
    if (order != 1 && order != 2) return fail(SS_ERR_ARG, "order must be 1 or 2");
    if (window == 0) return fail(SS_ERR_ARG, "window must be >= 1");
    if (window > kMaxLag || order * window > kMaxLag) return fail(SS_ERR_ARG, "order * window must be at most 32");
    std::memset(&tp, 0, sizeof(tp));
    const long long w = static_cast<long long>(window);
    long long norm = 0;
    for (long long n = 1; n <= w; ++n) norm += 2 * n * n;
    std::vector<long long> k{1};
    long long d = 1;
    for (size_t o = 0; o < order; ++o) {
        std::vector<long long> next(k.size() + 2 * window, 0);
        for (size_t i = 0; i < k.size(); ++i)
            for (long long n = -w; n <= w; ++n) next[i + static_cast<size_t>(n + w)] += k[i] * n;
        k.swap(next);
        d *= norm;
        const int half = static_cast<int>((o + 1) * window);
        for (size_t i = 0; i < k.size(); ++i)
            if (k[i] != 0) {
                tp.k[o][tp.n[o]] = static_cast<double>(k[i]);
                tp.off[o][tp.n[o]++] = static_cast<int>(i) - half;
            }
        tp.inv[o] = 1.0 / static_cast<double>(d);
    }
    tp.order = static_cast<unsigned>(order);
    tp.lag = static_cast<unsigned>(order * window);
    return SS_OK;
}

int check_packed(const float *vec, const void *off, const float *out, size_t n_clips, size_t total_rows, size_t cols, size_t order, size_t window,
                 DeltaTaps &tp)
{
    if (!vec || !off || !out) return fail(SS_ERR_ARG, "null buffer");
    if (cols == 0) return fail(SS_ERR_ARG, "empty feature matrix (cols == 0)");
    if (total_rows >= (1ull << 31) || cols >= (1ull << 31) || n_clips >= (1ull << 31)) return fail(SS_ERR_ARG, "feature block too large");
    const int rc = make_taps(order, window, tp);
    if (rc) return rc;
    const size_t bytes = total_rows * cols * sizeof(float);
    if (ranges_overlap(vec, bytes, out, bytes * (order + 1))) return fail(SS_ERR_ARG, "out overlaps vec: the call is not in place");
    return SS_OK;
}

int stream_len(size_t cols, size_t order, size_t window, DeltaTaps &tp, size_t &len)
{
    if (cols == 0) return fail(SS_ERR_ARG, "empty feature matrix (cols == 0)");
    const int rc = make_taps(order, window, tp);
    if (rc) return rc;
    if (cols >= (1ull << 31) || 2 * order * window * cols + 1 >= (1ull << 31))
        return fail(SS_ERR_ARG, "stream state too large: 2 * order * window * cols + 1 must be below 2^31");
    len = 2 * order * window * cols + 1;
    return SS_OK;
}

// what the pool calls reject before the device is touched (the tables apart).  The flush has no vec and no row offsets, and its
// total_rows is formed here: n_active * L rows of out.
int check_stream(bool flush, const float *vec, const void *ro, const void *slots, size_t n_active, size_t &total_rows, size_t pool_streams, size_t cols,
                 size_t order, size_t window, const float *pool, const float *out, DeltaTaps &tp, size_t &len)
{
    if ((!flush && (!vec || !ro)) || !slots || !pool || !out) return fail(SS_ERR_ARG, "null buffer");
    const int rc = stream_len(cols, order, window, tp, len);
    if (rc) return rc;
    if (flush && n_active < (1ull << 31)) total_rows = n_active * tp.lag;
    if (n_active >= (1ull << 31) || pool_streams >= (1ull << 31) || total_rows >= (1ull << 31))
        return fail(SS_ERR_ARG, "n_active, pool_streams and total_rows must be below 2^31");
    if (pool_streams == 0) return fail(SS_ERR_ARG, "the pool has no rows");
    const size_t bytes = total_rows * cols * sizeof(float), obytes = bytes * (order + 1), pbytes = pool_streams * len * sizeof(float);
    if (!flush && ranges_overlap(vec, bytes, out, obytes)) return fail(SS_ERR_ARG, "out overlaps vec: the call is not in place");
    if ((!flush && ranges_overlap(pool, pbytes, vec, bytes)) || ranges_overlap(pool, pbytes, out, obytes))
        return fail(SS_ERR_ARG, "the pool overlaps vec or out");
    return SS_OK;
}

// Host staging of both pool calls: vec (in_rows rows, none for the flush) and the row offsets go up with the n_active named pool
// rows, gathered into a compact block whose row i is entry i's (the device call runs on slots 0 .. n_active - 1); out_rows rows of
// out and the pool rows come down.  The caller's pool is written only once everything before it succeeded.
int stream_via_device(bool flush, const float *vec, size_t n_active, const int64_t *row_offsets, const int32_t *slots, size_t in_rows, size_t out_rows,
                      size_t cols, size_t order, size_t window, size_t len, float *pool, float *out)
{
    if (!have_device()) return no_device();
    PoolRows named;
    named.gather(pool, slots, n_active, len);
    const size_t bytes = in_rows * cols * sizeof(float), obytes = out_rows * cols * (order + 1) * sizeof(float);
    HostStage st("ss_add_deltas_stream");
    float *d_out = st.room<float>(obytes);
    const auto d_named = st.up_pool(named);
    const float *d_vec = flush ? nullptr : st.up(vec, bytes);
    const int64_t *d_ro = flush ? nullptr : st.up(row_offsets, (n_active + 1) * sizeof(int64_t));
    if (st.ok())
        st.ran(flush ? ss_add_deltas_stream_flush_device(n_active, d_named.slots, n_active, cols, order, window, d_named.rows, d_out, nullptr)
                     : ss_add_deltas_stream_packed_device(d_vec, n_active, d_ro, in_rows, d_named.slots, n_active, cols, order, window, d_named.rows, d_out,
                                                          nullptr));
    st.sync();
    st.down_pool(named, d_named);
    st.down(out, d_out, obytes);
    st.scatter(named, pool, slots);
    return st.status();
}

}  // namespace

}  // namespace ss

extern "C" {

int ss_add_deltas_packed_device(const float *d_vec, size_t n_clips, const int64_t *d_offsets, size_t total_rows, size_t cols, size_t order,
                                size_t window, float *d_out, void *stream)
{
    if (n_clips == 0) return SS_OK;
    ss::DeltaTaps tp;
    const int rc = ss::check_packed(d_vec, d_offsets, d_out, n_clips, total_rows, cols, order, window, tp);
    if (rc) return rc;
    if (total_rows == 0) return SS_OK;
    // one launch: gridDim.y workgroups share a long clip's row tiles
    const unsigned split = ss::packed_split(n_clips, (total_rows + ss::kRowTile - 1) / ss::kRowTile);
    hipLaunchKernelGGL(ss::ss_add_deltas_packed_kernel, dim3(static_cast<unsigned>(n_clips), split), dim3(256), 0, static_cast<hipStream_t>(stream), d_vec,
                       reinterpret_cast<const long long *>(d_offsets), d_out, static_cast<unsigned long long>(total_rows), static_cast<unsigned>(cols), tp);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? SS_OK : ss::hip_fail(e, "ss_add_deltas_packed_kernel");
}

// host-pointer form (synchronous): the table is checked on the host before the device is touched; the block and the table go up, the
// rows the table covers come down (a host table is gap-free; rows past offsets[n_clips] stay as the caller left them)
int ss_add_deltas_packed(const float *vec, size_t n_clips, const int64_t *offsets, size_t total_rows, size_t cols, size_t order, size_t window,
                         float *out)
{
    if (n_clips == 0) return SS_OK;
    ss::DeltaTaps tp;
    int rc = ss::check_packed(vec, offsets, out, n_clips, total_rows, cols, order, window, tp);
    if (rc || (rc = ss::check_clip_table(offsets, n_clips, total_rows))) return rc;
    if (offsets[n_clips] == 0) return SS_OK;
    if (!ss::have_device()) return ss::no_device();
    const size_t bytes = total_rows * cols * sizeof(float);
    ss::HostStage st("ss_add_deltas_packed");
    const float *d_in = st.up(vec, bytes);
    float *d_out = st.room<float>(bytes * (order + 1));
    const int64_t *d_off = st.up(offsets, (n_clips + 1) * sizeof(int64_t));
    if (st.ok()) st.ran(ss_add_deltas_packed_device(d_in, n_clips, d_off, total_rows, cols, order, window, d_out, nullptr));
    st.sync();
    st.down(out, d_out, static_cast<size_t>(offsets[n_clips]) * cols * (order + 1) * sizeof(float));
    return st.status();
}

int ss_add_deltas_stream_state_len(size_t cols, size_t order, size_t window, size_t *state_len)
{
    if (!state_len) return ss::fail(SS_ERR_ARG, "null output");
    ss::DeltaTaps tp;
    size_t len = 0;
    const int rc = ss::stream_len(cols, order, window, tp, len);
    if (rc) return rc;
    *state_len = len;
    return SS_OK;
}

int ss_add_deltas_stream_packed_device(const float *d_vec, size_t n_active, const int64_t *d_row_offsets, size_t total_rows, const int32_t *d_slots,
                                       size_t pool_streams, size_t cols, size_t order, size_t window, float *d_pool, float *d_out, void *stream)
{
    if (n_active == 0) return SS_OK;
    ss::DeltaTaps tp;
    size_t len = 0;
    const int rc = ss::check_stream(false, d_vec, d_row_offsets, d_slots, n_active, total_rows, pool_streams, cols, order, window, d_pool, d_out, tp, len);
    if (rc) return rc;
    if (total_rows == 0) return SS_OK;  // no entry can own a row
    // one launch, one workgroup per entry: the grid depends on n_active only
    hipLaunchKernelGGL(ss::ss_add_deltas_stream_kernel<false>, dim3(static_cast<unsigned>(n_active)), dim3(256), 0, static_cast<hipStream_t>(stream), d_vec,
                       reinterpret_cast<const long long *>(d_row_offsets), reinterpret_cast<const int *>(d_slots), d_out, d_pool,
                       static_cast<unsigned long long>(total_rows), static_cast<unsigned>(pool_streams), static_cast<unsigned>(cols), tp);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? SS_OK : ss::hip_fail(e, "ss_add_deltas_stream_kernel");
}

int ss_add_deltas_stream_packed(const float *vec, size_t n_active, const int64_t *row_offsets, const int32_t *slots, size_t pool_streams, size_t cols,
                                size_t order, size_t window, float *pool, float *out)
{
    if (n_active == 0) return SS_OK;
    if (!row_offsets) return ss::fail(SS_ERR_ARG, "null buffer");
    if (n_active >= (1ull << 31)) return ss::fail(SS_ERR_ARG, "n_active, pool_streams and total_rows must be below 2^31");
    int rc = ss::check_row_offsets(row_offsets, n_active);
    if (rc) return rc;
    size_t rows = static_cast<size_t>(row_offsets[n_active]);
    ss::DeltaTaps tp;
    size_t len = 0;
    rc = ss::check_stream(false, vec, row_offsets, slots, n_active, rows, pool_streams, cols, order, window, pool, out, tp, len);
    if (rc || (rc = ss::check_slots(slots, n_active, pool_streams))) return rc;
    if (rows == 0) return SS_OK;  // entries without rows only: nothing moves
    return ss::stream_via_device(false, vec, n_active, row_offsets, slots, rows, rows, cols, order, window, len, pool, out);
}

int ss_add_deltas_stream_flush_device(size_t n_active, const int32_t *d_slots, size_t pool_streams, size_t cols, size_t order, size_t window,
                                      float *d_pool, float *d_out, void *stream)
{
    if (n_active == 0) return SS_OK;
    ss::DeltaTaps tp;
    size_t len = 0;
    size_t rows = 0;  // n_active * L, formed by the check
    const int rc = ss::check_stream(true, nullptr, nullptr, d_slots, n_active, rows, pool_streams, cols, order, window, d_pool, d_out, tp, len);
    if (rc) return rc;
    hipLaunchKernelGGL(ss::ss_add_deltas_stream_kernel<true>, dim3(static_cast<unsigned>(n_active)), dim3(256), 0, static_cast<hipStream_t>(stream), nullptr,
                       nullptr, reinterpret_cast<const int *>(d_slots), d_out, d_pool, static_cast<unsigned long long>(rows),
                       static_cast<unsigned>(pool_streams), static_cast<unsigned>(cols), tp);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? SS_OK : ss::hip_fail(e, "ss_add_deltas_stream_kernel");
}

int ss_add_deltas_stream_flush(size_t n_active, const int32_t *slots, size_t pool_streams, size_t cols, size_t order, size_t window, float *pool,
                               float *out)
{
    if (n_active == 0) return SS_OK;
    ss::DeltaTaps tp;
    size_t len = 0, rows = 0;  // rows: n_active * L, formed by the check
    int rc = ss::check_stream(true, nullptr, nullptr, slots, n_active, rows, pool_streams, cols, order, window, pool, out, tp, len);
    if (rc || (rc = ss::check_slots(slots, n_active, pool_streams))) return rc;
    return ss::stream_via_device(true, nullptr, n_active, nullptr, slots, 0, rows, cols, order, window, len, pool, out);
}

}  // extern "C"
