// Frame splicing and subsampling (Kaldi's splice-feats / subsample-feats, FunASR's low frame rate): ss_splice_packed* on packed
// variable-length clips, and ss_splice_stream_packed* / ss_splice_stream_flush* over a pool of stream states that is fed whole
// periods of `stride` rows and answers D = right / stride periods late.  The definition (include/speechsauce_amd.h) is a gather:
// every output float is a bit copy of an input float, so a clip's bits depend on its own rows and nothing else -- not on the tile,
// the clip's place in the block, the entry's place in the call or how a stream was cut into calls.  The values are loaded,
// selected and stored; no arithmetic instruction ever sees one (a NaN keeps its payload, a denormal its bits).
// The reference crate has no such stage, so this file restates nothing of it.
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

constexpr unsigned kMaxContext = 32;  // left, right and stride: the bound of ss_add_deltas*' lag

// what the host knows about one call
struct SpliceShape {
    unsigned cols, left, right, stride;
    unsigned width;  // W = left + 1 + right: the rows under one output row
    unsigned ocols;  // W * cols: floats of an output row
    unsigned delay;  // D = right / stride: the periods a pooled stream's rows come late
    unsigned hist;   // H = D * stride + left: the raw rows a pooled stream carries
};

// Float q of a run of whole output rows: output row k of the run, context row c (0 .. W - 1, i.e. offset c - left) and column.
// I is the width the run's float count needs.
struct SpliceAt {
    unsigned k, c, col;
};
template <typename I>
__device__ __forceinline__ SpliceAt splice_at(I q, const SpliceShape &sh)
{
    const I k = q / sh.ocols;
    const unsigned j = static_cast<unsigned>(q - k * sh.ocols), c = j / sh.cols;
    return SpliceAt{static_cast<unsigned>(k), c, j - c * sh.cols};
}
__device__ __forceinline__ void splice_next(SpliceAt &a, const SpliceShape &sh)  // the place of float q + 1
{
    if (++a.col == sh.cols) {
        a.col = 0;
        if (++a.c == sh.width) {
            a.c = 0;
            ++a.k;
        }
    }
}

// ---- packed clips ----
// Clip b owns rows ro[b] .. ro[b+1] of x and rows oo[b] .. oo[b+1] of out.  Its output is ONE contiguous run of floats whatever
// W * cols is, so workgroup (b, y) forms the tiles y, y + gridDim.y, ... of kSpliceTile output rows each as a flat stream: 16-byte
// stores from the first 16-byte boundary of the tile on, up to three single floats in front of it and behind the last whole store
// (cols = 13, W = 11: 572-byte rows, every phase occurs).  The loads are plain: an input row is asked for W / stride times by
// neighbouring lanes of one tile, which L2 (and the vector L1) serve; HBM sees it once per tile.  No LDS, no barrier.
constexpr unsigned kSpliceTile = 64;  // output rows per tile

template <typename I>
__device__ __forceinline__ void splice_tile(const float *__restrict__ src, unsigned rows, float *__restrict__ dst, unsigned k0, unsigned tile_rows,
                                            const SpliceShape &sh)
{
    const long long last = static_cast<long long>(rows) - 1;
    auto value = [&](const SpliceAt &a) {  // the clip's row under (k0 + k, c), clamped to the clip: edge replication
        const long long r = static_cast<long long>(k0 + a.k) * sh.stride + a.c - static_cast<long long>(sh.left);
        return src[static_cast<size_t>(min(max(r, 0ll), last)) * sh.cols + a.col];
    };
    const I n = static_cast<I>(tile_rows) * sh.ocols;
    const unsigned to_boundary = (4u - static_cast<unsigned>(reinterpret_cast<uintptr_t>(dst) >> 2)) & 3u;
    const unsigned head = n < to_boundary ? static_cast<unsigned>(n) : to_boundary;
    const I quads = (n - head) / 4;
    const unsigned tail = static_cast<unsigned>(n - head - 4 * quads);
    if (threadIdx.x < head + tail) {  // at most six single floats
        const I q = threadIdx.x < head ? static_cast<I>(threadIdx.x) : 4 * quads + threadIdx.x;
        dst[q] = value(splice_at<I>(q, sh));
    }
    for (I i = threadIdx.x; i < quads; i += 256) {
        const I q = head + 4 * i;
        SpliceAt a = splice_at<I>(q, sh);
        float4 v;
        v.x = value(a);
        splice_next(a, sh);
        v.y = value(a);
        splice_next(a, sh);
        v.z = value(a);
        splice_next(a, sh);
        v.w = value(a);
        *reinterpret_cast<float4 *>(dst + q) = v;
    }
}

__global__ __launch_bounds__(256) void ss_splice_packed_kernel(const float *__restrict__ x, const long long *ro, const long long *oo, float *__restrict__ out,
                                                              unsigned long long total_rows, unsigned long long total_out_rows, const SpliceShape sh)
{
    const Segment seg = packed_segment(ro, total_rows);
    if (seg.rows == 0) return;
    const unsigned rows = seg.rows, out_rows = (rows + sh.stride - 1) / sh.stride;
    const long long olo = oo[blockIdx.x], ohi = oo[blockIdx.x + 1];
    // total_out_rows < 2^31: the difference is formed only once both ends are inside the block
    if (!(olo >= 0 && olo <= ohi && static_cast<unsigned long long>(ohi) <= total_out_rows && ohi - olo == static_cast<long long>(out_rows))) return;
    const float *src = x + seg.row0 * sh.cols;
    float *dst = out + static_cast<size_t>(olo) * sh.ocols;
    const unsigned n_tiles = (out_rows + kSpliceTile - 1) / kSpliceTile;
    for (unsigned rt = blockIdx.y; rt < n_tiles; rt += gridDim.y) {  // uniform per workgroup
        const unsigned k0 = rt * kSpliceTile, tr = min(kSpliceTile, out_rows - k0);
        float *d = dst + static_cast<size_t>(k0) * sh.ocols;
        if (sh.ocols < (1u << 25)) splice_tile<unsigned>(src, rows, d, k0, tr, sh);  // a tile has fewer than 2^31 floats
        else splice_tile<unsigned long long>(src, rows, d, k0, tr, sh);
    }
}

// ---- pool of stream states ----
// Entry i owns rows ro[i] .. ro[i+1] of x (whole periods, starting at a period), rows ro[i] / stride .. ro[i+1] / stride of out and
// pool row slots[i]: len = H * cols + 1 floats, the layout and the entry decoding of the add-deltas pool (row_pool_entry,
// ss_device.h).  The stream's rows are counted from the oldest valid history row: 0 .. count - 1 the history, count .. count + rows
// - 1 the entry's.  Output row k is centred on row v = count + (k - D) * stride.  v < 0 happens only while count < H, where count
// is every row the stream has seen: a warm-up row of zeros.  Otherwise the row's first context row v - left is >= 0 where the
// history is full (H = D * stride + left) and is clamped to row 0, the stream's first row, where it is not; its last one, v +
// right <= count + (k + 1) * stride - 1, has arrived.  The flush build has no new rows: it writes the D rows centred on count -
// D * stride .. count - stride, clamped at the stream's last row, and zeroes the pool row.
// column `col` of row r of an entry's stream, where the rows live in two global blocks: rows below `count` in the history (`old`: its
// oldest valid row), the others in the entry's rows (`src`)
__device__ __forceinline__ float row_of_two(const float *old, const float *src, unsigned count, unsigned cols, unsigned col, long long r)
{
    return r < static_cast<long long>(count) ? old[static_cast<size_t>(r) * cols + col] : src[static_cast<size_t>(r - count) * cols + col];
}

template <typename I, bool FLUSH>
__device__ __forceinline__ void splice_stream_rows(const float *old, const float *src, float *dst, unsigned count, long long last, I n, const SpliceShape &sh)
{
    for (I q = threadIdx.x; q < n; q += 256) {
        const SpliceAt a = splice_at<I>(q, sh);
        const long long v = static_cast<long long>(count) + (static_cast<long long>(a.k) - sh.delay) * sh.stride;
        float val = 0.0f;
        if (v >= 0) {
            const long long r = min(max(v + a.c - static_cast<long long>(sh.left), 0ll), last);
            val = FLUSH ? old[static_cast<size_t>(r) * sh.cols + a.col] : row_of_two(old, src, count, sh.cols, a.col, r);
        }
        dst[q] = val;
    }
}

template <bool FLUSH>
__global__ __launch_bounds__(256) void ss_splice_stream_kernel(const float *__restrict__ x, const long long *__restrict__ ro, const int *__restrict__ slots,
                                                              float *__restrict__ out, float *pool, unsigned long long total_rows, unsigned pool_streams,
                                                              const SpliceShape sh)
{
    const unsigned H = sh.hist, D = sh.delay, cols = sh.cols, state_len = H * cols + 1;
    const RowPoolEntry e = row_pool_entry<FLUSH>(ro, slots, total_rows, pool_streams, pool, state_len, H, D);
    if (!e.state) return;                                                // the whole workgroup: the pool row stays as it is
    if (!FLUSH && (e.row0 % sh.stride != 0 || e.rows % sh.stride != 0)) return;  // not whole periods: skipped like a bad pair
    const unsigned rows = e.rows, count = e.count;
    const unsigned n_out = FLUSH ? D : rows / sh.stride;
    const float *src = x + (FLUSH ? 0 : e.row0 * cols);  // the flush build never reads it: every row it sees is history
    float *dst = out + (FLUSH ? e.row0 : e.row0 / sh.stride) * sh.ocols;
    const float *old = e.state + static_cast<size_t>(H - count) * cols;  // the oldest valid history row
    const unsigned long long span = static_cast<unsigned long long>(count) + rows;  // rows the entry can see
    const long long last = static_cast<long long>(span) - 1;                     // the clamp on the right (reached by the flush only)
    const unsigned long long n = static_cast<unsigned long long>(n_out) * sh.ocols;
    if (n < (1ull << 31)) splice_stream_rows<unsigned, FLUSH>(old, src, dst, count, last, static_cast<unsigned>(n), sh);
    else splice_stream_rows<unsigned long long, FLUSH>(old, src, dst, count, last, n, sh);
    __syncthreads();  // every read of the pool row for the output rows lies before this barrier
    if (FLUSH) {
        for (unsigned i = threadIdx.x; i < state_len; i += 256) e.state[i] = 0.0f;  // the stream is fresh from here on
    } else {
        // The new pool row is the last H rows of (history ++ entry), zeros in front where there are fewer.  A history row moves
        // towards the front of the pool row it is read from (rows > 0), so the row is rewritten in ascending steps of 256 floats, each
        // read in full before it is written: a later step reads only what lies behind everything written so far.
        const long long lead = static_cast<long long>(H) - static_cast<long long>(span);  // rows of zeros in front (<= 0: none)
        const unsigned hn = H * cols;                                                     // below state_len < 2^31
        for (unsigned base = 0; base < hn; base += 256) {
            const unsigned at = base + threadIdx.x;
            float v = 0.0f;
            if (at < hn) {
                const long long j = static_cast<long long>(at / cols) - lead;
                if (j >= 0) v = row_of_two(old, src, count, cols, at % cols, j);
            }
            __syncthreads();
            if (at < hn) e.state[at] = v;
        }
        if (threadIdx.x == 0) e.state[state_len - 1] = static_cast<float>(min(span, static_cast<unsigned long long>(H)));
    }
}

// ---- host side ----

constexpr unsigned long long kCountLimit = 1ull << 31;

int make_shape(size_t cols, size_t left, size_t right, size_t stride, SpliceShape &sh)
{
    if (cols == 0) return fail(SS_ERR_ARG, "empty feature matrix (cols == 0)");
    if (left > kMaxContext || right > kMaxContext) return fail(SS_ERR_ARG, "left and right must be at most 32");
    if (stride < 1 || stride > kMaxContext) return fail(SS_ERR_ARG, "stride must be 1 .. 32");
    const size_t width = left + 1 + right;
    if (cols >= kCountLimit || width * cols >= kCountLimit) return fail(SS_ERR_ARG, "row too wide: (left + 1 + right) * cols must be below 2^31");
    sh.cols = static_cast<unsigned>(cols);
    sh.left = static_cast<unsigned>(left);
    sh.right = static_cast<unsigned>(right);
    sh.stride = static_cast<unsigned>(stride);
    sh.width = static_cast<unsigned>(width);
    sh.ocols = static_cast<unsigned>(width * cols);
    sh.delay = sh.right / sh.stride;
    sh.hist = sh.delay * sh.stride + sh.left;
    return SS_OK;
}

int check_packed_scalars(size_t n_clips, size_t total_rows, size_t total_out_rows, size_t cols, size_t left, size_t right, size_t stride, SpliceShape &sh)
{
    const int rc = make_shape(cols, left, right, stride, sh);
    if (rc) return rc;
    if (n_clips >= kCountLimit || total_rows >= kCountLimit || total_out_rows >= kCountLimit) return fail(SS_ERR_ARG, "feature block too large");
    return SS_OK;
}

int check_not_in_place(const float *vec, size_t total_rows, const float *out, size_t total_out_rows, const SpliceShape &sh)
{
    if (ranges_overlap(vec, total_rows * sh.cols * sizeof(float), out, total_out_rows * sh.ocols * sizeof(float)))
        return fail(SS_ERR_ARG, "out overlaps vec: the call is not in place");
    return SS_OK;
}

// (H <= left + right, so the state's H * cols + 1 floats are at most an output row's W * cols: below 2^31 with it)
int stream_len(size_t cols, size_t left, size_t right, size_t stride, SpliceShape &sh, size_t &len)
{
    const int rc = make_shape(cols, left, right, stride, sh);
    if (rc) return rc;
    len = static_cast<size_t>(sh.hist) * cols + 1;
    return SS_OK;
}

// what the pool calls reject before the device is touched (the tables apart).  The flush has no vec and no row offsets; its rows
// of out are n_active * D, and out may be null where that is none.
int check_stream(bool flush, const float *vec, const void *ro, const void *slots, size_t n_active, size_t total_rows, size_t pool_streams, size_t cols,
                 size_t left, size_t right, size_t stride, const float *pool, const float *out, SpliceShape &sh, size_t &len)
{
    const int rc = stream_len(cols, left, right, stride, sh, len);
    if (rc) return rc;
    if ((!flush && (!vec || !ro)) || !slots || !pool || (!out && !(flush && sh.delay == 0))) return fail(SS_ERR_ARG, "null buffer");
    if (n_active >= kCountLimit || pool_streams >= kCountLimit || total_rows >= kCountLimit)
        return fail(SS_ERR_ARG, "n_active, pool_streams and total_rows must be below 2^31");
    if (pool_streams == 0) return fail(SS_ERR_ARG, "the pool has no rows");
    const size_t out_rows = flush ? n_active * sh.delay : total_rows / stride;
    const size_t bytes = total_rows * cols * sizeof(float), obytes = out_rows * sh.ocols * sizeof(float), pbytes = pool_streams * len * sizeof(float);
    if (!flush && ranges_overlap(vec, bytes, out, obytes)) return fail(SS_ERR_ARG, "out overlaps vec: the call is not in place");
    if ((!flush && ranges_overlap(pool, pbytes, vec, bytes)) || (out && ranges_overlap(pool, pbytes, out, obytes)))
        return fail(SS_ERR_ARG, "the pool overlaps vec or out");
    return SS_OK;
}

template <bool FLUSH>
int launch_stream(const float *d_vec, size_t n_active, const int64_t *d_ro, size_t total_rows, const int32_t *d_slots, size_t pool_streams,
                  const SpliceShape &sh, float *d_pool, float *d_out, void *stream)
{
    // one launch, one workgroup per entry: the grid depends on n_active only
    hipLaunchKernelGGL(ss_splice_stream_kernel<FLUSH>, dim3(static_cast<unsigned>(n_active)), dim3(256), 0, static_cast<hipStream_t>(stream), d_vec,
                       reinterpret_cast<const long long *>(d_ro), reinterpret_cast<const int *>(d_slots), d_out, d_pool,
                       static_cast<unsigned long long>(total_rows), static_cast<unsigned>(pool_streams), sh);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "ss_splice_stream_kernel");
    note_kernel(FLUSH ? "ss_splice_stream_kernel<flush>" : "ss_splice_stream_kernel");
    return SS_OK;
}

// Host staging of both pool calls: vec (in_rows rows, none for the flush) and the row offsets go up with the n_active named pool
// rows, gathered into a compact block whose row i is entry i's (the device call runs on slots 0 .. n_active - 1); out_rows rows of
// out and the pool rows come down.  The caller's pool is written only once everything before it succeeded.
int stream_via_device(bool flush, const float *vec, size_t n_active, const int64_t *row_offsets, const int32_t *slots, size_t in_rows, size_t out_rows,
                      const SpliceShape &sh, size_t len, float *pool, float *out)
{
    if (!have_device()) return no_device();
    PoolRows named;
    named.gather(pool, slots, n_active, len);
    const size_t bytes = in_rows * sh.cols * sizeof(float), obytes = out_rows * sh.ocols * sizeof(float);
    HostStage st("ss_splice_stream");
    float *d_out = st.room<float>(obytes);
    const auto d_named = st.up_pool(named);
    const float *d_vec = flush ? nullptr : st.up(vec, bytes);
    const int64_t *d_ro = flush ? nullptr : st.up(row_offsets, (n_active + 1) * sizeof(int64_t));
    if (st.ok())
        st.ran(flush ? launch_stream<true>(nullptr, n_active, nullptr, out_rows, d_named.slots, n_active, sh, d_named.rows, d_out, nullptr)
                     : launch_stream<false>(d_vec, n_active, d_ro, in_rows, d_named.slots, n_active, sh, d_named.rows, d_out, nullptr));
    st.sync();
    st.down_pool(named, d_named);
    st.down(out, d_out, obytes);
    st.scatter(named, pool, slots);
    return st.status();
}

}  // namespace

}  // namespace ss

extern "C" {

int ss_splice_packed_offsets(size_t n_clips, const int64_t *row_offsets, size_t stride, int64_t *out_offsets)
{
    if (!row_offsets || !out_offsets) return ss::fail(SS_ERR_ARG, "null buffer");
    if (stride < 1 || stride > ss::kMaxContext) return ss::fail(SS_ERR_ARG, "stride must be 1 .. 32");
    if (n_clips >= ss::kCountLimit) return ss::fail(SS_ERR_ARG, "feature block too large");
    for (size_t b = 0; b < n_clips; ++b)
        if (row_offsets[b + 1] < row_offsets[b]) return ss::fail(SS_ERR_ARG, "decreasing offsets at clip " + std::to_string(b));
    // (out_offsets may be row_offsets: every entry is read before its place is written)
    const uint64_t s = stride;
    int64_t lo = row_offsets[0], acc = 0;
    out_offsets[0] = 0;
    for (size_t b = 0; b < n_clips; ++b) {
        const int64_t hi = row_offsets[b + 1];
        acc += static_cast<int64_t>((static_cast<uint64_t>(hi) - static_cast<uint64_t>(lo) + s - 1) / s);
        out_offsets[b + 1] = acc;
        lo = hi;
    }
    return SS_OK;
}

int ss_splice_packed_device(const float *d_vec, size_t n_clips, const int64_t *d_row_offsets, size_t total_rows, const int64_t *d_out_offsets,
                            size_t total_out_rows, size_t cols, size_t left, size_t right, size_t stride, float *d_out, void *stream)
{
    if (n_clips == 0) return SS_OK;
    if (!d_vec || !d_row_offsets || !d_out_offsets || !d_out) return ss::fail(SS_ERR_ARG, "null buffer");
    ss::SpliceShape sh;
    int rc = ss::check_packed_scalars(n_clips, total_rows, total_out_rows, cols, left, right, stride, sh);
    if (rc || (rc = ss::check_not_in_place(d_vec, total_rows, d_out, total_out_rows, sh))) return rc;
    if (total_rows == 0 || total_out_rows == 0) return SS_OK;  // no clip can own a row
    // one launch: gridDim.y workgroups share a long clip's tiles
    const unsigned split = ss::packed_split(n_clips, (total_out_rows + ss::kSpliceTile - 1) / ss::kSpliceTile);
    hipLaunchKernelGGL(ss::ss_splice_packed_kernel, dim3(static_cast<unsigned>(n_clips), split), dim3(256), 0, static_cast<hipStream_t>(stream), d_vec,
                       reinterpret_cast<const long long *>(d_row_offsets), reinterpret_cast<const long long *>(d_out_offsets), d_out,
                       static_cast<unsigned long long>(total_rows), static_cast<unsigned long long>(total_out_rows), sh);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return ss::hip_fail(e, "ss_splice_packed_kernel");
    ss::note_kernel("ss_splice_packed_kernel");
    return SS_OK;
}

// host-pointer form (synchronous): the table is checked on the host before the device is touched and the output table formed from
// it; the block and both tables go up, the rows the table covers come down (a host table is gap-free)
int ss_splice_packed(const float *vec, size_t n_clips, const int64_t *row_offsets, size_t total_rows, size_t cols, size_t left, size_t right, size_t stride,
                     float *out)
{
    if (n_clips == 0) return SS_OK;
    if (!vec || !row_offsets || !out) return ss::fail(SS_ERR_ARG, "null buffer");
    ss::SpliceShape sh;
    int rc = ss::check_packed_scalars(n_clips, total_rows, 0, cols, left, right, stride, sh);
    if (rc || (rc = ss::check_clip_table(row_offsets, n_clips, total_rows))) return rc;
    std::vector<int64_t> oo(n_clips + 1);
    if ((rc = ss_splice_packed_offsets(n_clips, row_offsets, stride, oo.data()))) return rc;
    const size_t out_rows = static_cast<size_t>(oo[n_clips]);  // at most total_rows
    if ((rc = ss::check_not_in_place(vec, total_rows, out, out_rows, sh))) return rc;
    if (out_rows == 0) return SS_OK;
    if (!ss::have_device()) return ss::no_device();
    const size_t bytes = total_rows * cols * sizeof(float), obytes = out_rows * sh.ocols * sizeof(float), tbytes = (n_clips + 1) * sizeof(int64_t);
    ss::HostStage st("ss_splice_packed");
    const float *d_in = st.up(vec, bytes);
    float *d_out = st.room<float>(obytes);
    const int64_t *d_ro = st.up(row_offsets, tbytes), *d_oo = st.up(oo.data(), tbytes);
    if (st.ok()) st.ran(ss_splice_packed_device(d_in, n_clips, d_ro, total_rows, d_oo, out_rows, cols, left, right, stride, d_out, nullptr));
    st.sync();
    st.down(out, d_out, obytes);
    return st.status();
}

int ss_splice_stream_state_len(size_t cols, size_t left, size_t right, size_t stride, size_t *state_len, size_t *delay_rows)
{
    if (!state_len || !delay_rows) return ss::fail(SS_ERR_ARG, "null output");
    ss::SpliceShape sh;
    size_t len = 0;
    const int rc = ss::stream_len(cols, left, right, stride, sh, len);
    if (rc) return rc;
    *state_len = len;
    *delay_rows = sh.delay;
    return SS_OK;
}

int ss_splice_stream_packed_device(const float *d_vec, size_t n_active, const int64_t *d_row_offsets, size_t total_rows, const int32_t *d_slots,
                                   size_t pool_streams, size_t cols, size_t left, size_t right, size_t stride, float *d_pool, float *d_out, void *stream)
{
    if (n_active == 0) return SS_OK;
    ss::SpliceShape sh;
    size_t len = 0;
    const int rc = ss::check_stream(false, d_vec, d_row_offsets, d_slots, n_active, total_rows, pool_streams, cols, left, right, stride, d_pool, d_out, sh, len);
    if (rc) return rc;
    if (total_rows == 0) return SS_OK;  // no entry can own a row
    return ss::launch_stream<false>(d_vec, n_active, d_row_offsets, total_rows, d_slots, pool_streams, sh, d_pool, d_out, stream);
}

int ss_splice_stream_packed(const float *vec, size_t n_active, const int64_t *row_offsets, const int32_t *slots, size_t pool_streams, size_t cols,
                            size_t left, size_t right, size_t stride, float *pool, float *out)
{
    if (n_active == 0) return SS_OK;
    if (!row_offsets) return ss::fail(SS_ERR_ARG, "null buffer");
    if (n_active >= ss::kCountLimit) return ss::fail(SS_ERR_ARG, "n_active, pool_streams and total_rows must be below 2^31");
    int rc = ss::check_row_offsets(row_offsets, n_active);
    if (rc) return rc;
    const size_t rows = static_cast<size_t>(row_offsets[n_active]);
    ss::SpliceShape sh;
    size_t len = 0;
    rc = ss::check_stream(false, vec, row_offsets, slots, n_active, rows, pool_streams, cols, left, right, stride, pool, out, sh, len);
    if (rc) return rc;
    for (size_t i = 0; i < n_active; ++i)  // (row_offsets[0] == 0: every start is then a multiple of the stride too)
        if ((row_offsets[i + 1] - row_offsets[i]) % static_cast<int64_t>(stride))
            return ss::fail(SS_ERR_ARG, "entry " + std::to_string(i) + ": " + std::to_string(row_offsets[i + 1] - row_offsets[i]) +
                                            " rows are not whole periods of " + std::to_string(stride));
    if ((rc = ss::check_slots(slots, n_active, pool_streams))) return rc;
    if (rows == 0) return SS_OK;  // entries without rows only: nothing moves
    return ss::stream_via_device(false, vec, n_active, row_offsets, slots, rows, rows / stride, sh, len, pool, out);
}

int ss_splice_stream_flush_device(size_t n_active, const int32_t *d_slots, size_t pool_streams, size_t cols, size_t left, size_t right, size_t stride,
                                  float *d_pool, float *d_out, void *stream)
{
    if (n_active == 0) return SS_OK;
    ss::SpliceShape sh;
    size_t len = 0;
    const int rc = ss::check_stream(true, nullptr, nullptr, d_slots, n_active, 0, pool_streams, cols, left, right, stride, d_pool, d_out, sh, len);
    if (rc) return rc;
    if (n_active * sh.delay >= ss::kCountLimit) return ss::fail(SS_ERR_ARG, "n_active, pool_streams and total_rows must be below 2^31");
    return ss::launch_stream<true>(nullptr, n_active, nullptr, n_active * sh.delay, d_slots, pool_streams, sh, d_pool, d_out, stream);
}

int ss_splice_stream_flush(size_t n_active, const int32_t *slots, size_t pool_streams, size_t cols, size_t left, size_t right, size_t stride, float *pool,
                           float *out)
{
    if (n_active == 0) return SS_OK;
    ss::SpliceShape sh;
    size_t len = 0;
    int rc = ss::check_stream(true, nullptr, nullptr, slots, n_active, 0, pool_streams, cols, left, right, stride, pool, out, sh, len);
    if (rc || (rc = ss::check_slots(slots, n_active, pool_streams))) return rc;
    if (n_active * sh.delay >= ss::kCountLimit) return ss::fail(SS_ERR_ARG, "n_active, pool_streams and total_rows must be below 2^31");
    return ss::stream_via_device(true, nullptr, n_active, nullptr, slots, 0, n_active * sh.delay, sh, len, pool, out);
}

}  // extern "C"
