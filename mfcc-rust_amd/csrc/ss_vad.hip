// Energy voice-activity decision (Kaldi's compute-vad-energy) and the selection of kept rows (select-voiced-frames):
// ss_vad_energy_packed* and ss_select_rows_packed* on packed variable-length clips, ss_vad_energy_stream_packed* /
// ss_vad_energy_stream_flush* over a pool of stream states that answers L = frames_context rows late.  The definition is the
// ss_vad_* comment of include/speechsauce_amd.h.  A clip's mask bytes depend on its own rows and the scalars only: the mean behind
// the threshold is summed in the order ss_cmvn_packed_kernel sums a column (ss_post.hip), counted from the clip's first row, and
// every other step is a comparison or an integer count.  The selection is a gather: every output float is a bit copy of an input
// float, no arithmetic instruction ever sees one (a NaN keeps its payload, a denormal its bits).
// The reference crate has no such stage, so this file restates nothing of it.
#include "ss_device.h"
#include "ss_hip_staging.h"
#include "ss_host_checks.h"
#include "ss_internal.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

namespace ss {

namespace {

constexpr unsigned kMaxContext = 32;  // frames_context: the bound of ss_add_deltas*' lag and ss_splice*'s context

// what the host knows about one decision call
struct VadShape {
    unsigned cols, col, L;
    float prop;        // proportion_threshold
    double thr0, scale;  // energy_threshold and energy_mean_scale, widened
};

// thr = energy_threshold + energy_mean_scale * mean in f64: a product and a sum, each rounded (never one fma)
__device__ __forceinline__ double vad_threshold(const VadShape &sh, double mean) { return __dadd_rn(sh.thr0, __dmul_rn(sh.scale, mean)); }
// Kaldi's `num_count >= den_count * proportion_threshold`: int x float is ONE f32 product
__device__ __forceinline__ bool vad_decide(unsigned num, unsigned den, float prop)
{
    return static_cast<float>(num) >= __fmul_rn(static_cast<float>(den), prop);
}

// ---- packed clips: the decision ----
// Workgroup (b, y) serves clip b.  Each of the (up to gridDim.y) workgroups that share a long clip forms the clip's mean itself, in
// ss_cmvn_packed_kernel's order: chunks = min(64, ceil(T / 32)) serial f64 sums of rpc = ceil(T / chunks) rows each, added serially
// in chunk order.  The rows are then decided in tiles of 256: the raw decisions of the tile's rows and of L rows on either side
// go to LDS, and every row counts its window there.  Tile rt belongs to workgroup rt % share; with a count table, workgroup 0 walks
// every tile (it stores only its own) so that the clip's count is one plain store: no atomic, no zeroed word in front.
constexpr unsigned kVadChunks = 64;       // kCmvnChunks
constexpr unsigned kVadTile = 256;        // rows per tile: one per lane
constexpr unsigned kVadSplitRows = 2048;  // a clip gets one workgroup per 2048 rows (up to gridDim.y), as kCmvnSplitRows

__global__ __launch_bounds__(256) void ss_vad_energy_packed_kernel(const float *__restrict__ x, const long long *__restrict__ off,
                                                                  unsigned char *__restrict__ mask, long long *__restrict__ counts,
                                                                  unsigned long long total_rows, const VadShape sh)
{
    __shared__ double part[kVadChunks];
    __shared__ unsigned char raw[kVadTile + 2 * kMaxContext];
    const Segment seg = packed_segment(off, total_rows);
    if (seg.rows == 0) {
        // a valid clip without rows has a count; a rejected segment keeps its count word
        const long long lo = off[blockIdx.x], hi = off[blockIdx.x + 1];
        if (counts && blockIdx.y == 0 && threadIdx.x == 0 && lo >= 0 && lo == hi && static_cast<unsigned long long>(hi) <= total_rows) counts[blockIdx.x] = 0;
        return;
    }
    const unsigned rows = seg.rows, L = sh.L;
    const unsigned share = min(gridDim.y, (rows + kVadSplitRows - 1) / kVadSplitRows);
    if (blockIdx.y >= share) return;
    const float *e = x + seg.row0 * sh.cols + sh.col;  // e[t * cols]: the energy of row t
    double thr = sh.thr0;
    if (sh.scale != 0.0) {  // uniform: the mean is formed only where it is used
        const unsigned chunks = min(kVadChunks, (rows + 31) / 32);
        const unsigned rpc = (rows + chunks - 1) / chunks;
        if (threadIdx.x < chunks) {
            const unsigned r0 = threadIdx.x * rpc, r1 = min(rows, r0 + rpc);
            double s1 = 0.0;
            for (unsigned r = r0; r < r1; ++r) s1 += static_cast<double>(e[static_cast<size_t>(r) * sh.cols]);
            part[threadIdx.x] = s1;
        }
        __syncthreads();
        double s1 = 0.0;
        for (unsigned k = 0; k < chunks; ++k) s1 += part[k];  // every lane, the same order
        thr = vad_threshold(sh, s1 / rows);
    }
    const bool all_tiles = counts != nullptr && blockIdx.y == 0;
    const unsigned n_tiles = (rows + kVadTile - 1) / kVadTile;
    unsigned voiced = 0;
    for (unsigned rt = all_tiles ? 0 : blockIdx.y; rt < n_tiles; rt += all_tiles ? 1 : share) {  // uniform per workgroup
        const long long t0 = static_cast<long long>(rt) * kVadTile;
        for (unsigned i = threadIdx.x; i < kVadTile + 2 * L; i += 256) {  // raw[i]: row t0 - L + i
            const long long t = t0 - L + i;
            bool v = false;
            if (t >= 0 && t < static_cast<long long>(rows)) v = static_cast<double>(e[static_cast<size_t>(t) * sh.cols]) > thr;
            raw[i] = v;
        }
        __syncthreads();
        const long long t = t0 + threadIdx.x;
        bool m = false;
        if (t < static_cast<long long>(rows)) {
            const long long lo = max(t - L, 0ll), hi = min(t + L, static_cast<long long>(rows) - 1);
            unsigned num = 0;
            for (long long u = lo; u <= hi; ++u) num += raw[u - t0 + L];
            m = vad_decide(num, static_cast<unsigned>(hi - lo + 1), sh.prop);
            if (rt % share == blockIdx.y) mask[seg.row0 + static_cast<unsigned long long>(t)] = m;
        }
        voiced += __syncthreads_count(m);  // (also the barrier in front of the next tile's raw[])
    }
    if (all_tiles && threadIdx.x == 0) counts[blockIdx.x] = voiced;
}

// ---- packed clips: the selection ----
// Three launches on one stream.  Workgroup (b, y) of the count and the move launch owns the tiles [y * per, (y + 1) * per) of clip
// b, per = ceil(n_tiles / gridDim.y): a contiguous run of rows.
//   count: part[b * Y + y] := kept rows of that run (0 for a rejected or empty segment): every word is stored, none accumulated.
//   scan:  one workgroup; oo[0] = 0, oo[b + 1] = oo[b] + sum_y part[b][y], and part[b][y] := the kept rows of clip b ahead of run y.
//   move:  the run's kept rows go to out rows oo[b] + part[b][y] .., tile by tile with a running count.
// So the mask is read twice, vec and out once, and nothing grows with a clip's length but the walk over its own bytes.
constexpr unsigned kSelTile = 256;  // rows per tile: one mask byte per lane

struct SelRun {
    unsigned long long row0;  // the clip's first row
    unsigned rows;            // the clip's rows (0: nothing to do)
    unsigned t_lo, t_hi;      // the tiles of this workgroup
};
__device__ __forceinline__ SelRun sel_run(const long long *__restrict__ ro, unsigned long long total_rows)
{
    const Segment seg = packed_segment(ro, total_rows);
    const unsigned n_tiles = (seg.rows + kSelTile - 1) / kSelTile, per = (n_tiles + gridDim.y - 1) / gridDim.y;
    const unsigned t_lo = min(n_tiles, blockIdx.y * per);  // per * gridDim.y < n_tiles + gridDim.y: no overflow
    return SelRun{seg.row0, seg.rows, t_lo, min(n_tiles, t_lo + per)};
}

__global__ __launch_bounds__(256) void ss_select_count_kernel(const long long *__restrict__ ro, const unsigned char *__restrict__ mask,
                                                             unsigned *__restrict__ part, unsigned long long total_rows)
{
    const SelRun run = sel_run(ro, total_rows);
    const unsigned char *m = mask + run.row0;
    unsigned kept = 0;
    for (unsigned rt = run.t_lo; rt < run.t_hi; ++rt) {  // uniform per workgroup
        const unsigned r = rt * kSelTile + threadIdx.x;
        kept += __syncthreads_count(r < run.rows && m[r] != 0);
    }
    if (threadIdx.x == 0) part[static_cast<size_t>(blockIdx.x) * gridDim.y + blockIdx.y] = kept;
}

__global__ __launch_bounds__(1024) void ss_select_scan_kernel(unsigned *__restrict__ part, long long *__restrict__ oo, unsigned n_clips, unsigned Y)
{
    __shared__ unsigned long long sums[1024];
    const unsigned per = (n_clips + 1023) / 1024;  // n_clips < 2^31: threadIdx.x * per stays below 2^32
    const unsigned b0 = min(n_clips, threadIdx.x * per), b1 = min(n_clips, b0 + per);
    unsigned long long mine = 0;
    for (unsigned b = b0; b < b1; ++b)
        for (unsigned y = 0; y < Y; ++y) mine += part[static_cast<size_t>(b) * Y + y];
    sums[threadIdx.x] = mine;
    __syncthreads();
    for (unsigned d = 1; d < 1024; d <<= 1) {  // inclusive scan of the 1024 sums
        const unsigned long long v = threadIdx.x >= d ? sums[threadIdx.x - d] : 0;
        __syncthreads();
        sums[threadIdx.x] += v;
        __syncthreads();
    }
    unsigned long long at = sums[threadIdx.x] - mine;  // kept rows of the clips in front of b0
    if (threadIdx.x == 0) oo[0] = 0;
    for (unsigned b = b0; b < b1; ++b) {
        unsigned ahead = 0;
        for (unsigned y = 0; y < Y; ++y) {
            const size_t i = static_cast<size_t>(b) * Y + y;
            const unsigned c = part[i];
            part[i] = ahead;
            ahead += c;
        }
        at += ahead;
        oo[b + 1] = static_cast<long long>(at);
    }
}

// One tile of the move: the lanes' mask bytes become a rank among the tile's kept rows (a wave64 ballot, the lane's prefix by mbcnt,
// the waves' totals through LDS), the kept rows' indices go to LDS in that order, and the tile's output -- one contiguous run of
// kept * cols floats -- is written as splice_tile writes: 16-byte stores from the run's first 16-byte boundary, up to three single
// floats in front and behind.  select_store is that last step, on the kept rows' indices in LDS.
template <typename I>
__device__ __forceinline__ void select_store(const float *__restrict__ src, const unsigned *rows_of, float *__restrict__ dst, unsigned kept, unsigned cols)
{
    auto value = [&](unsigned k, unsigned col) { return src[static_cast<size_t>(rows_of[k]) * cols + col]; };
    const I n = static_cast<I>(kept) * cols;
    const unsigned to_boundary = (4u - static_cast<unsigned>(reinterpret_cast<uintptr_t>(dst) >> 2)) & 3u;
    const unsigned head = n < to_boundary ? static_cast<unsigned>(n) : to_boundary;
    const I quads = (n - head) / 4;
    const unsigned tail = static_cast<unsigned>(n - head - 4 * quads);
    if (threadIdx.x < head + tail) {  // at most six single floats
        const I q = threadIdx.x < head ? static_cast<I>(threadIdx.x) : 4 * quads + threadIdx.x;
        const I k = q / cols;
        dst[q] = value(static_cast<unsigned>(k), static_cast<unsigned>(q - k * cols));
    }
    for (I i = threadIdx.x; i < quads; i += 256) {
        const I q = head + 4 * i;
        const I kq = q / cols;
        unsigned k = static_cast<unsigned>(kq), col = static_cast<unsigned>(q - kq * cols);
        float v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            v[j] = value(k, col);
            if (++col == cols) {
                col = 0;
                ++k;  // (past the last kept row only behind the last float)
            }
        }
        *reinterpret_cast<float4 *>(dst + q) = make_float4(v[0], v[1], v[2], v[3]);
    }
}

__global__ __launch_bounds__(256) void ss_select_move_kernel(const float *__restrict__ x, const long long *__restrict__ ro,
                                                            const unsigned char *__restrict__ mask, const unsigned *__restrict__ part,
                                                            const long long *__restrict__ oo, float *__restrict__ out, unsigned long long total_rows,
                                                            unsigned cols)
{
    __shared__ unsigned rows_of[kSelTile];
    __shared__ unsigned wave_kept[4];
    const SelRun run = sel_run(ro, total_rows);
    if (run.t_lo >= run.t_hi) return;
    const long long olo = oo[blockIdx.x], ohi = oo[blockIdx.x + 1];
    // the kept rows of clips that overlap each other could outgrow the block: such a clip's rows stay unwritten
    if (!(olo >= 0 && olo <= ohi && static_cast<unsigned long long>(ohi) <= total_rows)) return;
    const unsigned char *m = mask + run.row0;
    const float *src = x + run.row0 * cols;
    unsigned long long at = static_cast<unsigned long long>(olo) + part[static_cast<size_t>(blockIdx.x) * gridDim.y + blockIdx.y];
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (unsigned rt = run.t_lo; rt < run.t_hi; ++rt) {  // uniform per workgroup
        const unsigned r = rt * kSelTile + threadIdx.x;
        const bool keep = r < run.rows && m[r] != 0;
        const unsigned long long votes = __ballot(keep);
        const unsigned below = __builtin_amdgcn_mbcnt_hi(static_cast<unsigned>(votes >> 32), __builtin_amdgcn_mbcnt_lo(static_cast<unsigned>(votes), 0u));
        if (lane == 0) wave_kept[wave] = static_cast<unsigned>(__popcll(votes));
        __syncthreads();
        unsigned before = 0, kept = 0;
        for (unsigned w = 0; w < 4; ++w) {
            const unsigned c = wave_kept[w];
            before += w < wave ? c : 0u;
            kept += c;
        }
        if (keep) rows_of[before + below] = r;
        __syncthreads();
        if (at + kept <= static_cast<unsigned long long>(ohi)) {  // (always, for a part table the scan formed from this mask)
            float *dst = out + static_cast<size_t>(at) * cols;
            if (cols < (1u << 22)) select_store<unsigned>(src, rows_of, dst, kept, cols);  // a tile has fewer than 2^31 floats
            else select_store<unsigned long long>(src, rows_of, dst, kept, cols);
        }
        at += kept;
        __syncthreads();  // the next tile overwrites rows_of / wave_kept
    }
}

// ---- pool of stream states: the decision ----
// Entry i owns rows ro[i] .. ro[i+1] of x, the same bytes of mask and pool row slots[i]: len = 2 L + 4 floats -- the two halves of the
// f64 sum S of every energy the stream has brought, the rows seen N (a uint32), the stream's last 2 L energies (oldest first,
// right-aligned, zeros in front) and, in the last float, how many of them are valid (row_pool_entry, ss_device.h).  Byte k of an
// entry is the decision for stream row t = N + k - L (0 while t < 0: warm-up): its window t - L .. t + L is clipped at the stream's
// first row, its last member is the row that came with byte k, and every member is compared against thr_t = energy_threshold +
// energy_mean_scale * (S_n / n), n = t + L + 1, S_n the ONE accumulator after n rows in stream order.  The flush decides rows
// N - L .. N - 1 with n = N and the window clipped at the stream's last row, and zeroes the pool row.
constexpr unsigned kVadStreamTile = 256;  // bytes decided between two advances of the accumulator

template <bool FLUSH>
__global__ __launch_bounds__(256) void ss_vad_energy_stream_kernel(const float *__restrict__ x, const long long *__restrict__ ro, const int *__restrict__ slots,
                                                                  unsigned char *__restrict__ mask, float *pool, unsigned long long total_rows,
                                                                  unsigned pool_streams, const VadShape sh)
{
    __shared__ double thr_of[kVadStreamTile];
    const unsigned L = sh.L, H = 2 * L, state_len = H + 4;
    const RowPoolEntry en = row_pool_entry<FLUSH>(ro, slots, total_rows, pool_streams, pool, state_len, H, L);
    if (!en.state) return;  // the whole workgroup: the pool row and the entry's bytes stay as they are
    double sum = __hiloint2double(__float_as_int(en.state[1]), __float_as_int(en.state[0]));
    unsigned seen = __float_as_uint(en.state[2]), count = en.count;
    const float cw = en.state[state_len - 1];
    if (!(cw >= 0.0f && cw <= static_cast<float>(H) && cw == floorf(cw)) || seen < count) {  // a bad count word, or rows seen below the count: a fresh stream
        sum = 0.0;
        seen = 0;
        count = 0;
    }
    const long long N = seen;
    const float *hist = en.state + 3 + (H - count);  // energy of stream row r, N - count <= r < N: hist[r - (N - count)]
    const float *e = x + (FLUSH ? 0 : en.row0 * sh.cols + sh.col);  // energy of stream row r >= N: e[(r - N) * cols]; never read by the flush
    unsigned char *dst = mask + en.row0;
    const long long first = N - count;  // the oldest row the entry can see (0 for a state the calls wrote while N <= 2 L)
    auto energy = [&](long long r) { return r < N ? hist[r - first] : e[static_cast<size_t>(r - N) * sh.cols]; };
    const unsigned n_out = FLUSH ? L : en.rows;
    const long long last = N + en.rows - 1;  // the stream's newest row
    for (unsigned k0 = 0; k0 < n_out; k0 += kVadStreamTile) {  // uniform per workgroup
        const unsigned kn = min(kVadStreamTile, n_out - k0);
        if (threadIdx.x == 0) {  // the one accumulator, row by row in stream order
            for (unsigned k = 0; k < kn; ++k) {
                double mean;
                if (FLUSH) {
                    mean = sum / static_cast<double>(N);
                } else {
                    sum += static_cast<double>(e[static_cast<size_t>(k0 + k) * sh.cols]);
                    mean = sum / static_cast<double>(N + k0 + k + 1);
                }
                thr_of[k] = sh.scale != 0.0 ? vad_threshold(sh, mean) : sh.thr0;
            }
        }
        __syncthreads();
        if (threadIdx.x < kn) {
            const unsigned k = k0 + threadIdx.x;
            const long long t = N + k - L;
            bool m = false;
            if (t >= 0) {
                const double thr = thr_of[threadIdx.x];
                const long long lo = max(t - L, first), hi = min(t + L, last);
                unsigned num = 0;
                for (long long u = lo; u <= hi; ++u) num += static_cast<double>(energy(u)) > thr;
                m = vad_decide(num, static_cast<unsigned>(hi - lo + 1), sh.prop);
            }
            dst[k] = m;
        }
        __syncthreads();  // thr_of is rewritten by the next round
    }
    // every read of the pool row for the decisions lies before the last barrier above (n_out == 0: there was none to make)
    if (FLUSH) {
        if (threadIdx.x < state_len) en.state[threadIdx.x] = 0.0f;  // the stream is fresh from here on (state_len <= 68)
    } else {
        // the new history: the last 2 L energies of (history ++ entry), zeros in front where there are fewer; read whole, then written
        const long long lead = static_cast<long long>(H) - (static_cast<long long>(count) + en.rows);  // zeros in front (<= 0: none)
        float v = 0.0f;
        if (threadIdx.x < H && static_cast<long long>(threadIdx.x) >= lead) v = energy(first + (static_cast<long long>(threadIdx.x) - lead));
        __syncthreads();
        if (threadIdx.x < H) en.state[3 + threadIdx.x] = v;
        if (threadIdx.x == 0) {
            en.state[0] = __int_as_float(__double2loint(sum));
            en.state[1] = __int_as_float(__double2hiint(sum));
            en.state[2] = __uint_as_float(static_cast<unsigned>(N + en.rows));
            en.state[state_len - 1] = static_cast<float>(min(static_cast<unsigned long long>(count) + en.rows, static_cast<unsigned long long>(H)));
        }
    }
}

// ---- host side ----

constexpr unsigned long long kCountLimit = 1ull << 31;

int make_shape(size_t cols, size_t energy_col, float energy_threshold, float energy_mean_scale, size_t frames_context, float proportion_threshold, VadShape &sh)
{
    if (cols == 0) return fail(SS_ERR_ARG, "empty feature matrix (cols == 0)");
    if (cols >= kCountLimit) return fail(SS_ERR_ARG, "feature block too large");
    if (energy_col >= cols) return fail(SS_ERR_ARG, "energy_col must be below cols");
    if (frames_context > kMaxContext) return fail(SS_ERR_ARG, "frames_context must be at most 32");
    if (!(proportion_threshold > 0.0f && proportion_threshold < 1.0f)) return fail(SS_ERR_ARG, "proportion_threshold must lie strictly between 0 and 1");
    if (!std::isfinite(energy_threshold) || !std::isfinite(energy_mean_scale)) return fail(SS_ERR_ARG, "energy_threshold and energy_mean_scale must be finite");
    sh.cols = static_cast<unsigned>(cols);
    sh.col = static_cast<unsigned>(energy_col);
    sh.L = static_cast<unsigned>(frames_context);
    sh.prop = proportion_threshold;
    sh.thr0 = static_cast<double>(energy_threshold);
    sh.scale = static_cast<double>(energy_mean_scale);
    return SS_OK;
}

int check_vad_packed(const void *vec, const void *off, const void *mask, size_t n_clips, size_t total_rows, size_t cols, size_t energy_col,
                     float energy_threshold, float energy_mean_scale, size_t frames_context, float proportion_threshold, VadShape &sh)
{
    if (!vec || !off || !mask) return fail(SS_ERR_ARG, "null buffer");
    const int rc = make_shape(cols, energy_col, energy_threshold, energy_mean_scale, frames_context, proportion_threshold, sh);
    if (rc) return rc;
    if (n_clips >= kCountLimit || total_rows >= kCountLimit) return fail(SS_ERR_ARG, "feature block too large");
    return SS_OK;
}

int check_select(const float *vec, const void *ro, const uint8_t *mask, const void *oo, const float *out, size_t n_clips, size_t total_rows, size_t cols)
{
    if (!vec || !ro || !mask || !oo || !out) return fail(SS_ERR_ARG, "null buffer");
    if (cols == 0) return fail(SS_ERR_ARG, "empty feature matrix (cols == 0)");
    if (n_clips >= kCountLimit || total_rows >= kCountLimit || cols >= kCountLimit) return fail(SS_ERR_ARG, "feature block too large");
    const size_t bytes = total_rows * cols * sizeof(float);
    if (ranges_overlap(vec, bytes, out, bytes)) return fail(SS_ERR_ARG, "out overlaps vec: the call is not in place");
    if (ranges_overlap(mask, total_rows, out, bytes)) return fail(SS_ERR_ARG, "out overlaps the mask");
    return SS_OK;
}

int stream_len(size_t frames_context, size_t &len)
{
    if (frames_context > kMaxContext) return fail(SS_ERR_ARG, "frames_context must be at most 32");
    len = 2 * frames_context + 4;
    return SS_OK;
}

// what the pool calls reject before the device is touched (the tables apart).  The flush has no vec and no row offsets (cols = 1,
// energy_col = 0 stand in); its bytes of mask are n_active * L, and mask may be null where that is none.
int check_stream(bool flush, const float *vec, const void *ro, const void *slots, size_t n_active, size_t total_rows, size_t pool_streams, size_t cols,
                 size_t energy_col, float energy_threshold, float energy_mean_scale, size_t frames_context, float proportion_threshold, const float *pool,
                 const uint8_t *mask, VadShape &sh, size_t &len)
{
    const int rc = make_shape(cols, energy_col, energy_threshold, energy_mean_scale, frames_context, proportion_threshold, sh);
    if (rc) return rc;
    stream_len(frames_context, len);
    if ((!flush && (!vec || !ro)) || !slots || !pool || (!mask && !(flush && sh.L == 0))) return fail(SS_ERR_ARG, "null buffer");
    if (n_active >= kCountLimit || pool_streams >= kCountLimit || total_rows >= kCountLimit)
        return fail(SS_ERR_ARG, "n_active, pool_streams and total_rows must be below 2^31");
    if (pool_streams == 0) return fail(SS_ERR_ARG, "the pool has no rows");
    const size_t bytes = total_rows * cols * sizeof(float), mbytes = flush ? n_active * sh.L : total_rows, pbytes = pool_streams * len * sizeof(float);
    if (!flush && ranges_overlap(vec, bytes, mask, mbytes)) return fail(SS_ERR_ARG, "mask overlaps vec");
    if ((!flush && ranges_overlap(pool, pbytes, vec, bytes)) || (mask && ranges_overlap(pool, pbytes, mask, mbytes)))
        return fail(SS_ERR_ARG, "the pool overlaps vec or mask");
    return SS_OK;
}

template <bool FLUSH>
int launch_stream(const float *d_vec, size_t n_active, const int64_t *d_ro, size_t total_rows, const int32_t *d_slots, size_t pool_streams,
                  const VadShape &sh, float *d_pool, uint8_t *d_mask, void *stream)
{
    // one launch, one workgroup per entry: the grid depends on n_active only
    hipLaunchKernelGGL(ss_vad_energy_stream_kernel<FLUSH>, dim3(static_cast<unsigned>(n_active)), dim3(256), 0, static_cast<hipStream_t>(stream), d_vec,
                       reinterpret_cast<const long long *>(d_ro), reinterpret_cast<const int *>(d_slots), d_mask, d_pool,
                       static_cast<unsigned long long>(total_rows), static_cast<unsigned>(pool_streams), sh);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "ss_vad_energy_stream_kernel");
    note_kernel(FLUSH ? "ss_vad_energy_stream_kernel<flush>" : "ss_vad_energy_stream_kernel");
    return SS_OK;
}

// Host staging of both pool calls, as ss_splice.hip's: vec (in_rows rows, none for the flush) and the row offsets go up with the
// n_active named pool rows, gathered into a compact block whose row i is entry i's; out_bytes bytes of mask and the pool rows come
// down.  The caller's pool is written only once everything before it succeeded.
int stream_via_device(bool flush, const float *vec, size_t n_active, const int64_t *row_offsets, const int32_t *slots, size_t in_rows, size_t out_bytes,
                      const VadShape &sh, size_t len, float *pool, uint8_t *mask)
{
    if (!have_device()) return no_device();
    PoolRows named;
    named.gather(pool, slots, n_active, len);
    HostStage st("ss_vad_energy_stream");
    uint8_t *d_mask = st.room<uint8_t>(out_bytes);
    const auto d_named = st.up_pool(named);
    const float *d_vec = flush ? nullptr : st.up(vec, in_rows * sh.cols * sizeof(float));
    const int64_t *d_ro = flush ? nullptr : st.up(row_offsets, (n_active + 1) * sizeof(int64_t));
    if (st.ok())
        st.ran(flush ? launch_stream<true>(nullptr, n_active, nullptr, out_bytes, d_named.slots, n_active, sh, d_named.rows, d_mask, nullptr)
                     : launch_stream<false>(d_vec, n_active, d_ro, in_rows, d_named.slots, n_active, sh, d_named.rows, d_mask, nullptr));
    st.sync();
    st.down_pool(named, d_named);
    st.down(mask, d_mask, out_bytes);
    st.scatter(named, pool, slots);
    return st.status();
}

}  // namespace

}  // namespace ss

extern "C" {

int ss_vad_energy_packed_device(const float *d_vec, size_t n_clips, const int64_t *d_offsets, size_t total_rows, size_t cols, size_t energy_col,
                                float energy_threshold, float energy_mean_scale, size_t frames_context, float proportion_threshold, uint8_t *d_mask,
                                int64_t *d_counts, void *stream)
{
    if (n_clips == 0) return SS_OK;
    ss::VadShape sh;
    const int rc = ss::check_vad_packed(d_vec, d_offsets, d_mask, n_clips, total_rows, cols, energy_col, energy_threshold, energy_mean_scale, frames_context,
                                        proportion_threshold, sh);
    if (rc) return rc;
    // one launch (also where total_rows == 0 and there is a count table: every valid clip is then one without rows)
    if (total_rows == 0 && !d_counts) return SS_OK;
    const unsigned split = ss::packed_split(n_clips, (total_rows + ss::kVadSplitRows - 1) / ss::kVadSplitRows);
    hipLaunchKernelGGL(ss::ss_vad_energy_packed_kernel, dim3(static_cast<unsigned>(n_clips), split), dim3(256), 0, static_cast<hipStream_t>(stream), d_vec,
                       reinterpret_cast<const long long *>(d_offsets), d_mask, reinterpret_cast<long long *>(d_counts),
                       static_cast<unsigned long long>(total_rows), sh);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return ss::hip_fail(e, "ss_vad_energy_packed_kernel");
    ss::note_kernel("ss_vad_energy_packed_kernel");
    return SS_OK;
}

// host-pointer form (synchronous): the table is checked on the host before the device is touched; the block and the table go up, the
// bytes the table covers and the counts come down (a host table is gap-free)
int ss_vad_energy_packed(const float *vec, size_t n_clips, const int64_t *offsets, size_t total_rows, size_t cols, size_t energy_col, float energy_threshold,
                         float energy_mean_scale, size_t frames_context, float proportion_threshold, uint8_t *mask, int64_t *counts)
{
    if (n_clips == 0) return SS_OK;
    ss::VadShape sh;
    int rc = ss::check_vad_packed(vec, offsets, mask, n_clips, total_rows, cols, energy_col, energy_threshold, energy_mean_scale, frames_context,
                                  proportion_threshold, sh);
    if (rc || (rc = ss::check_clip_table(offsets, n_clips, total_rows))) return rc;
    const size_t rows = static_cast<size_t>(offsets[n_clips]);
    if (rows == 0) {  // clips without rows only: nothing for the device to do
        if (counts) std::fill(counts, counts + n_clips, int64_t{0});
        return SS_OK;
    }
    if (!ss::have_device()) return ss::no_device();
    const size_t cbytes = n_clips * sizeof(int64_t);
    ss::HostStage st("ss_vad_energy_packed");
    const float *d_in = st.up(vec, rows * cols * sizeof(float));
    uint8_t *d_mask = st.room<uint8_t>(rows);
    const int64_t *d_off = st.up(offsets, (n_clips + 1) * sizeof(int64_t));
    int64_t *d_cnt = st.room<int64_t>(cbytes);
    if (st.ok())
        st.ran(ss_vad_energy_packed_device(d_in, n_clips, d_off, rows, cols, energy_col, energy_threshold, energy_mean_scale, frames_context,
                                           proportion_threshold, d_mask, counts ? d_cnt : nullptr, nullptr));
    st.sync();
    st.down(mask, d_mask, rows);
    if (counts) st.down(counts, d_cnt, cbytes);
    return st.status();
}

int ss_select_rows_packed_device(const float *d_vec, size_t n_clips, const int64_t *d_row_offsets, size_t total_rows, size_t cols, const uint8_t *d_mask,
                                 int64_t *d_out_offsets, float *d_out, void *stream)
{
    if (n_clips == 0) return SS_OK;
    const int rc = ss::check_select(d_vec, d_row_offsets, d_mask, d_out_offsets, d_out, n_clips, total_rows, cols);
    if (rc) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (total_rows == 0) {  // no clip can own a row: the table is zeros
        const hipError_t e = hipMemsetAsync(d_out_offsets, 0, (n_clips + 1) * sizeof(int64_t), s);
        return e == hipSuccess ? SS_OK : ss::hip_fail(e, "hipMemsetAsync");
    }
    // three launches whatever the sizes; the runs' counts go through a stream-ordered scratch block
    const unsigned split = ss::packed_split(n_clips, (total_rows + ss::kSelTile - 1) / ss::kSelTile);
    const dim3 grid(static_cast<unsigned>(n_clips), split);
    const long long *ro = reinterpret_cast<const long long *>(d_row_offsets);
    long long *oo = reinterpret_cast<long long *>(d_out_offsets);
    unsigned *d_part = nullptr;
    hipError_t e = hipMallocAsync(reinterpret_cast<void **>(&d_part), n_clips * split * sizeof(unsigned), s);
    if (e != hipSuccess) return ss::hip_fail(e, "hipMallocAsync");
    hipLaunchKernelGGL(ss::ss_select_count_kernel, grid, dim3(256), 0, s, ro, d_mask, d_part, static_cast<unsigned long long>(total_rows));
    hipLaunchKernelGGL(ss::ss_select_scan_kernel, dim3(1), dim3(1024), 0, s, d_part, oo, static_cast<unsigned>(n_clips), split);
    hipLaunchKernelGGL(ss::ss_select_move_kernel, grid, dim3(256), 0, s, d_vec, ro, d_mask, d_part, oo, d_out, static_cast<unsigned long long>(total_rows),
                       static_cast<unsigned>(cols));
    e = hipFreeAsync(d_part, s);
    if (e != hipSuccess) return ss::hip_fail(e, "hipFreeAsync");
    e = hipGetLastError();
    if (e != hipSuccess) return ss::hip_fail(e, "ss_select_rows_packed kernels");
    ss::note_kernel("ss_select_move_kernel");
    return SS_OK;
}

// host-pointer form (synchronous): the table is checked first; the block, the table and the mask go up, the output table and the
// rows it covers come down
int ss_select_rows_packed(const float *vec, size_t n_clips, const int64_t *row_offsets, size_t total_rows, size_t cols, const uint8_t *mask,
                          int64_t *out_offsets, float *out)
{
    if (n_clips == 0) return SS_OK;
    int rc = ss::check_select(vec, row_offsets, mask, out_offsets, out, n_clips, total_rows, cols);
    if (rc || (rc = ss::check_clip_table(row_offsets, n_clips, total_rows))) return rc;
    const size_t rows = static_cast<size_t>(row_offsets[n_clips]);
    if (rows == 0) {  // clips without rows only: nothing for the device to do
        std::fill(out_offsets, out_offsets + n_clips + 1, int64_t{0});
        return SS_OK;
    }
    if (!ss::have_device()) return ss::no_device();
    const size_t bytes = rows * cols * sizeof(float), tbytes = (n_clips + 1) * sizeof(int64_t);
    std::vector<int64_t> oo(n_clips + 1);
    ss::HostStage st("ss_select_rows_packed");
    const float *d_in = st.up(vec, bytes);
    float *d_out = st.room<float>(bytes);
    const uint8_t *d_mask = st.up(mask, rows);
    const int64_t *d_ro = st.up(row_offsets, tbytes);
    int64_t *d_oo = st.room<int64_t>(tbytes);
    if (st.ok()) st.ran(ss_select_rows_packed_device(d_in, n_clips, d_ro, rows, cols, d_mask, d_oo, d_out, nullptr));
    st.sync();
    st.down(oo.data(), d_oo, tbytes);  // the output table first: it says how many rows come down
    if (st.ok()) st.down(out, d_out, static_cast<size_t>(oo[n_clips]) * cols * sizeof(float));
    if (st.ok()) std::copy(oo.begin(), oo.end(), out_offsets);
    return st.status();
}

int ss_vad_energy_stream_state_len(size_t frames_context, size_t *state_len)
{
    if (!state_len) return ss::fail(SS_ERR_ARG, "null output");
    size_t len = 0;
    const int rc = ss::stream_len(frames_context, len);
    if (rc) return rc;
    *state_len = len;
    return SS_OK;
}

int ss_vad_energy_stream_packed_device(const float *d_vec, size_t n_active, const int64_t *d_row_offsets, size_t total_rows, const int32_t *d_slots,
                                       size_t pool_streams, size_t cols, size_t energy_col, float energy_threshold, float energy_mean_scale,
                                       size_t frames_context, float proportion_threshold, float *d_pool, uint8_t *d_mask, void *stream)
{
    if (n_active == 0) return SS_OK;
    ss::VadShape sh;
    size_t len = 0;
    const int rc = ss::check_stream(false, d_vec, d_row_offsets, d_slots, n_active, total_rows, pool_streams, cols, energy_col, energy_threshold,
                                    energy_mean_scale, frames_context, proportion_threshold, d_pool, d_mask, sh, len);
    if (rc) return rc;
    if (total_rows == 0) return SS_OK;  // no entry can own a row
    return ss::launch_stream<false>(d_vec, n_active, d_row_offsets, total_rows, d_slots, pool_streams, sh, d_pool, d_mask, stream);
}

int ss_vad_energy_stream_packed(const float *vec, size_t n_active, const int64_t *row_offsets, const int32_t *slots, size_t pool_streams, size_t cols,
                                size_t energy_col, float energy_threshold, float energy_mean_scale, size_t frames_context, float proportion_threshold,
                                float *pool, uint8_t *mask)
{
    if (n_active == 0) return SS_OK;
    if (!row_offsets) return ss::fail(SS_ERR_ARG, "null buffer");
    if (n_active >= ss::kCountLimit) return ss::fail(SS_ERR_ARG, "n_active, pool_streams and total_rows must be below 2^31");
    int rc = ss::check_row_offsets(row_offsets, n_active);
    if (rc) return rc;
    const size_t rows = static_cast<size_t>(row_offsets[n_active]);
    ss::VadShape sh;
    size_t len = 0;
    rc = ss::check_stream(false, vec, row_offsets, slots, n_active, rows, pool_streams, cols, energy_col, energy_threshold, energy_mean_scale, frames_context,
                          proportion_threshold, pool, mask, sh, len);
    if (rc || (rc = ss::check_slots(slots, n_active, pool_streams))) return rc;
    if (rows == 0) return SS_OK;  // entries without rows only: nothing moves
    return ss::stream_via_device(false, vec, n_active, row_offsets, slots, rows, rows, sh, len, pool, mask);
}

int ss_vad_energy_stream_flush_device(size_t n_active, const int32_t *d_slots, size_t pool_streams, float energy_threshold, float energy_mean_scale,
                                      size_t frames_context, float proportion_threshold, float *d_pool, uint8_t *d_mask, void *stream)
{
    if (n_active == 0) return SS_OK;
    ss::VadShape sh;
    size_t len = 0;
    const int rc = ss::check_stream(true, nullptr, nullptr, d_slots, n_active, 0, pool_streams, 1, 0, energy_threshold, energy_mean_scale, frames_context,
                                    proportion_threshold, d_pool, d_mask, sh, len);
    if (rc) return rc;
    return ss::launch_stream<true>(nullptr, n_active, nullptr, n_active * sh.L, d_slots, pool_streams, sh, d_pool, d_mask, stream);
}

int ss_vad_energy_stream_flush(size_t n_active, const int32_t *slots, size_t pool_streams, float energy_threshold, float energy_mean_scale,
                               size_t frames_context, float proportion_threshold, float *pool, uint8_t *mask)
{
    if (n_active == 0) return SS_OK;
    ss::VadShape sh;
    size_t len = 0;
    int rc = ss::check_stream(true, nullptr, nullptr, slots, n_active, 0, pool_streams, 1, 0, energy_threshold, energy_mean_scale, frames_context,
                              proportion_threshold, pool, mask, sh, len);
    if (rc || (rc = ss::check_slots(slots, n_active, pool_streams))) return rc;
    return ss::stream_via_device(true, nullptr, n_active, nullptr, slots, 0, n_active * sh.L, sh, len, pool, mask);
}

}  // extern "C"
