// Grouped CMVN of packed rows: per-speaker and global statistics that can be accumulated, merged, stored and applied
// (ss_cmvn_stats_packed* / ss_cmvn_apply_packed* / ss_cmvn_grouped_packed* and the Kaldi accumulator conversions).  The definition
// is the "grouped CMVN" comment of include/speechsauce_amd.h; the reference crate has no such stage, so this file restates nothing
// of it.  A group's statistics are one row [ n | mean[cols] | var[cols] ] of doubles in a caller-owned block [n_groups x (2 cols + 1)].
//
// Statistics, two launches and one scratch block [n_clips x 2 cols] of doubles (stream-ordered; inside a capture see Scratch below):
//   ss_cmvn_clip_stats_kernel   workgroup (b, y) forms mean_b / var_b of clip b for the 32-column tiles y, y + gridDim.y, ...: the
//                               first two phases of ss_cmvn_packed_kernel (ss_post.hip) word for word -- tasks (chunk, column) with
//                               columns fastest, chunks = min(64, ceil(T / 32)), serial f64 sums per chunk in LDS, added in chunk
//                               order, the squares about the clip's first row -- so mean_b is the mean ss_cmvn_packed* subtracts.
//                               One workgroup owns a (clip, column tile) whatever the clip's length: a long clip is not shared, the
//                               column tiles are (a 2100-row clip is 64 chunks x 32 columns = 2048 tasks of 33 rows for 256 lanes).
//   ss_cmvn_fold_kernel         one workgroup per group, a lane per column.  The group's clips are found by a SCAN of the tables in
//                               steps of 256 clips: every lane tests one clip (valid segment, this group), a ballot / prefix over
//                               the four waves compacts the hits into LDS in ascending clip index (stable by construction, no
//                               atomics), their scratch rows are staged in LDS by all lanes, and every column lane folds them
//                               serially into its (mean, var) registers.  The
//                               scan costs n_clips / 256 steps per group, 16 at the design point of 4096 clips; it was chosen over
//                               a device-side count / prefix / scatter because it needs no second scratch table and no
//                               further launch, and its cost is below the serial fold's at every shape measured.
//                               The merge is Chan's in variance form with every operation rounded on its own (fold_weights / merge_column: no
//                               contraction), so a row's bits are those of the left fold of the header, however the clips were
//                               cut into calls.  A group without a valid clip in the call is not written.
// Apply, one launch (ss_cmvn_apply_kernel): a flat walk over the block in spans of whole rows, about 8192 elements per workgroup.
// The workgroup finds the clip of its first row by offset_find, then steps from clip to clip by offset_seek; the rows of one clip
// inside the span are one contiguous run of elements, written with 16-byte stores from the run's first 16-byte boundary of `out`
// on (the loads are dword aligned only: legal in the unaligned access mode the HSA ABI sets, as in ss_pad.hip) and element stores
// in front of it and behind the last whole store.  mean and 1 / (sqrt(var) + 2^-30) of the clip's group sit in LDS, two doubles per
// column, and are formed afresh only where the group changes along the span; above kApplyLdsCols columns they are formed per
// element from the statistics row instead (the same expressions, the same bits).  Every element is read and written by the same
// lane, so out == vec is legal.
// Containment: every kernel recomputes a clip's validity from the tables (group_clip): a segment that is reversed, starts below 0 or
// ends past total_rows, or a group id outside [0, n_groups), takes no step and has no row written; the apply walk only ever forms
// addresses of rows r with span_lo <= r < min(span_hi, total_rows) that lie inside a validated segment, and reads the statistics
// row of a validated group id only.
#include "ss_device.h"
#include "ss_hip_staging.h"
#include "ss_host_checks.h"
#include "ss_internal.h"
#include "speechsauce_amd.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <map>
#include <mutex>
#include <string>

namespace ss {

namespace {

constexpr double kEps30 = 9.313225746154785e-10;  // 2^-30, as ss_post.hip
constexpr unsigned kCmvnChunks = 64;              // as ss_post.hip: chunks = min(64, ceil(rows / 32))
constexpr unsigned kCmvnTile = 32;                // columns whose chunk partials sit in LDS at a time
constexpr unsigned kStatTilesY = 64;              // at most this many workgroups share a clip's column tiles
constexpr unsigned kApplyLdsCols = 512;           // columns whose (mean, inv) pairs sit in the apply kernel's 8 KiB of LDS
constexpr unsigned kApplySpan = 8192;             // elements of a workgroup's span of the apply walk (whole rows, at least one)

// var_about of ss_post.hip: the population variance from s2k = sum (v - K)^2, K one of the values
__device__ __forceinline__ double var_about(double s2k, double n, double mean, double K)
{
    const double d = mean - K;
    const double var = fma(-d, d, s2k / n);
    return var < 0.0 ? 0.0 : var;
}

// a statistics row's count word: not finite or below 1 is read as 0 (a fresh group)
__device__ __forceinline__ double stats_count(double n) { return n >= 1.0 && n < INFINITY ? n : 0.0; }

struct GroupClip {
    unsigned long long row0;
    unsigned rows;  // 0: the clip takes no step (empty, a rejected segment or a group id outside [0, n_groups))
    unsigned group;
};
// grp == nullptr: every clip is of group 0
__device__ __forceinline__ GroupClip group_clip(const long long *__restrict__ off, const int *__restrict__ grp, unsigned b, unsigned long long total_rows,
                                                unsigned n_groups)
{
    const long long lo = off[b], hi = off[b + 1];
    const int g = grp ? grp[b] : 0;
    GroupClip c{0, 0, 0};
    if (lo >= 0 && lo < hi && static_cast<unsigned long long>(hi) <= total_rows && g >= 0 && static_cast<unsigned>(g) < n_groups) {
        c.row0 = static_cast<unsigned long long>(lo);
        c.rows = static_cast<unsigned>(hi - lo);  // total_rows < 2^31: the row count fits
        c.group = static_cast<unsigned>(g);
    }
    return c;
}

// clipstat[b] = [ mean_b[cols] | var_b[cols] ] for every clip that takes a step
__global__ __launch_bounds__(256) void ss_cmvn_clip_stats_kernel(const float *__restrict__ x, const long long *__restrict__ off, const int *__restrict__ grp,
                                                                double *__restrict__ clipstat, unsigned long long total_rows, unsigned cols,
                                                                unsigned n_groups)
{
    __shared__ double part[kCmvnChunks * kCmvnTile * 2];
    const GroupClip gc = group_clip(off, grp, blockIdx.x, total_rows, n_groups);
    if (gc.rows == 0) return;
    const unsigned rows = gc.rows;
    const unsigned chunks = min(kCmvnChunks, (rows + 31) / 32);
    const unsigned rpc = (rows + chunks - 1) / chunks;
    const float *src = x + gc.row0 * cols;
    double *dst = clipstat + static_cast<size_t>(blockIdx.x) * 2 * cols;
    for (unsigned c0 = blockIdx.y * kCmvnTile; c0 < cols; c0 += gridDim.y * kCmvnTile) {
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
            dst[c0 + threadIdx.x] = mean;
            dst[cols + c0 + threadIdx.x] = var_about(s2, rows, mean, static_cast<double>(src[c0 + threadIdx.x]));
        }
        __syncthreads();  // the next column tile overwrites part
    }
}

// The merge of a group's running (na, mean, var) with a clip's (nb, mb, vb) is the header's six lines, each operation rounded on its
// own.  The three weights depend on the row counts only, so they are the same for every column: fold_weights forms them once per
// listed clip (one lane per clip, the divisions side by side), and merge_column is what is left for the serial walk of a column.
struct FoldWeights {
    double wa, wb, wab;
};
__device__ __forceinline__ FoldWeights fold_weights(double na, double nb)
{
#pragma clang fp contract(off)
    const double n = na + nb;
    FoldWeights w;
    w.wa = na / n;
    w.wb = nb / n;
    w.wab = w.wa * w.wb;
    return w;
}
__device__ __forceinline__ void merge_column(double &mean, double &var, double na, const FoldWeights &w, double mb, double vb)
{
#pragma clang fp contract(off)
    const double d = mb - mean;
    const double m = mean + d * w.wb;
    const double v = (w.wa * var + w.wb * vb) + (d * d) * w.wab;
    const bool fresh = na == 0.0;  // a fresh group: the clip's statistics are copied (a select, not a branch: the walk stays straight-line)
    mean = fresh ? mb : m;
    var = fresh ? vb : v;
}

constexpr unsigned kFoldStage = 4096;  // doubles of LDS that stage the listed clips' scratch rows: 32 KiB, at least 8 clips of 256 columns

__global__ __launch_bounds__(256) void ss_cmvn_fold_kernel(const long long *__restrict__ off, const int *__restrict__ grp,
                                                          const double *__restrict__ clipstat, double *__restrict__ stats, unsigned n_clips,
                                                          unsigned long long total_rows, unsigned cols, unsigned n_groups)
{
    __shared__ unsigned list[256], list_rows[256], wave_hits[4];
    __shared__ unsigned long long wave_rows[4];
    __shared__ double s_na[256];  // the group's count in front of listed clip k
    __shared__ double s_n;        // ... and behind the last one
    __shared__ FoldWeights s_w[256];
    __shared__ double stage[kFoldStage];
    const unsigned g = blockIdx.x, lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    double *row = stats + static_cast<size_t>(g) * (2 * static_cast<size_t>(cols) + 1);
    const double n0 = stats_count(row[0]);
    double n_end = n0;
    bool any = false;
    for (unsigned c0 = 0; c0 < cols; c0 += 256) {  // one scan of the tables per 256 columns
        const unsigned cw = min(256u, cols - c0), c = c0 + threadIdx.x;
        const bool mine = threadIdx.x < cw;
        double n_run = n0, mean = 0.0, var = 0.0;  // n_run: the same in every lane
        if (mine && n0 > 0.0) {
            mean = row[1 + c];
            var = row[1 + cols + c];
        }
        for (unsigned b0 = 0; b0 < n_clips; b0 += 256) {
            const unsigned b = b0 + threadIdx.x;
            unsigned rows = 0;
            if (b < n_clips) {
                const GroupClip gc = group_clip(off, grp, b, total_rows, n_groups);
                if (gc.rows != 0 && gc.group == g) rows = gc.rows;
            }
            const unsigned long long hits = __ballot(rows != 0);
            if (lane == 0) wave_hits[wave] = static_cast<unsigned>(__popcll(hits));
            __syncthreads();
            unsigned at = static_cast<unsigned>(__popcll(hits & ((1ull << lane) - 1ull))), total = 0;
            for (unsigned w = 0; w < 4; ++w) {
                if (w < wave) at += wave_hits[w];
                total += wave_hits[w];
            }
            if (total != 0) {  // the same in every lane
                if (rows != 0) {
                    list[at] = b;  // ascending clip index
                    list_rows[at] = rows;
                }
                __syncthreads();
                // The counts in front of every listed clip are a serial sum too.  A whole-numbered count of at most 2^52 plus at
                // most 256 x 2^31 rows is exact in f64 in any order, so the lanes form it as an integer prefix sum; any other count
                // (a row the caller wrote by hand) takes the serial walk in one lane.
                const bool whole = n_run <= 4503599627370496.0 && n_run == floor(n_run);
                const unsigned own = threadIdx.x < total ? list_rows[threadIdx.x] : 0u;
                if (whole) {
                    unsigned long long incl = own;
                    for (unsigned d = 1; d < 64; d <<= 1) {
                        const unsigned long long up = __shfl_up(incl, d, 64);
                        if (lane >= d) incl += up;
                    }
                    if (lane == 63) wave_rows[wave] = incl;
                    __syncthreads();
                    unsigned long long before = incl - own, all = 0;
                    for (unsigned w = 0; w < 4; ++w) {
                        if (w < wave) before += wave_rows[w];
                        all += wave_rows[w];
                    }
                    const double na = n_run + static_cast<double>(before);
                    if (threadIdx.x < total) {
                        s_na[threadIdx.x] = na;
                        s_w[threadIdx.x] = fold_weights(na, static_cast<double>(own));
                    }
                    n_run = n_run + static_cast<double>(all);
                } else {
                    if (threadIdx.x == 0) {
                        double n = n_run;
                        for (unsigned k = 0; k < total; ++k) {
                            s_na[k] = n;
                            n = n + static_cast<double>(list_rows[k]);
                        }
                        s_n = n;
                    }
                    __syncthreads();
                    if (threadIdx.x < total) s_w[threadIdx.x] = fold_weights(s_na[threadIdx.x], static_cast<double>(own));
                    n_run = s_n;
                }
                // The listed clips' scratch rows go through LDS, as many clips at a time as fit: all lanes fetch a batch into registers
                // while the column lanes fold the batch before it, eight clips' operands read from LDS side by side.
                const unsigned fit = kFoldStage / (2 * cw);
                double next[kFoldStage / 256];
                auto fetch = [&](unsigned k0) {
                    const unsigned sub = min(fit, total - k0);
#pragma unroll
                    for (unsigned j = 0; j < kFoldStage / 256; ++j) {
                        const unsigned i = threadIdx.x + 256 * j;
                        next[j] = 0.0;
                        if (i < sub * 2 * cw) {
                            const unsigned k = i / (2 * cw), rem = i - k * 2 * cw, half = rem >= cw ? 1u : 0u;
                            next[j] = clipstat[static_cast<size_t>(list[k0 + k]) * 2 * cols + half * cols + c0 + (rem - half * cw)];
                        }
                    }
                };
                fetch(0);
                for (unsigned k0 = 0; k0 < total; k0 += fit) {
                    const unsigned sub = min(fit, total - k0);
                    __syncthreads();  // s_na / s_w are written; the lanes are done with the stage of the batch before
#pragma unroll
                    for (unsigned j = 0; j < kFoldStage / 256; ++j) stage[threadIdx.x + 256 * j] = next[j];
                    __syncthreads();
                    if (k0 + fit < total) fetch(k0 + fit);
                    if (mine) {
                        for (unsigned k1 = 0; k1 < sub; k1 += 8) {
                            double na[8], mb[8], vb[8];
                            FoldWeights w[8];
#pragma unroll
                            for (unsigned j = 0; j < 8; ++j) {  // past the batch's end: its last clip again, not folded
                                const unsigned k = min(k1 + j, sub - 1);
                                na[j] = s_na[k0 + k];
                                w[j] = s_w[k0 + k];
                                mb[j] = stage[k * 2 * cw + threadIdx.x];
                                vb[j] = stage[k * 2 * cw + cw + threadIdx.x];
                            }
#pragma unroll
                            for (unsigned j = 0; j < 8; ++j)
                                if (k1 + j < sub) merge_column(mean, var, na[j], w[j], mb[j], vb[j]);
                        }
                    }
                }
                any = true;
            }
            __syncthreads();  // the next step overwrites the lists and the wave words
        }
        if (mine && any) {
            row[1 + c] = mean;
            row[1 + cols + c] = var;
        }
        n_end = n_run;
    }
    if (threadIdx.x == 0 && any) row[0] = n_end;
}

typedef float float4u __attribute__((ext_vector_type(4), aligned(4)));   // a dword-aligned 16-byte load
typedef float float4a __attribute__((ext_vector_type(4), aligned(16)));

template <bool WIDE>
__global__ __launch_bounds__(256) void ss_cmvn_apply_kernel(const float *x, const long long *__restrict__ off, const int *__restrict__ grp,
                                                           const double *__restrict__ stats, float *out, unsigned n_clips,
                                                           unsigned long long total_rows, unsigned cols, unsigned n_groups, unsigned span_rows,
                                                           int variance)
{
    __shared__ double stat[WIDE ? 2 : 2 * kApplyLdsCols];  // mean, 1 / (std + 2^-30) per column
    const size_t len = 2 * static_cast<size_t>(cols) + 1;
    const unsigned long long span_lo = static_cast<unsigned long long>(blockIdx.x) * span_rows;
    const unsigned long long span_hi = min(total_rows, span_lo + span_rows);
    unsigned long long r = span_lo;
    if (r >= span_hi) return;
    unsigned c = offset_find(off, n_clips, static_cast<long long>(r));
    long long cached = -1;  // the group whose pair sits in LDS
    while (r < span_hi) {   // every value that steers this loop is the same in all lanes
        c = offset_seek(off, n_clips, c, static_cast<long long>(r));
        const long long lo = off[c], hi = off[c + 1];
        if (lo > static_cast<long long>(r)) {  // rows in front of the table's first clip
            r = min(span_hi, static_cast<unsigned long long>(lo));
            continue;
        }
        if (static_cast<long long>(r) >= hi) break;  // rows behind the table's last clip
        const unsigned long long r_end = min(span_hi, static_cast<unsigned long long>(hi));
        const GroupClip gc = group_clip(off, grp, c, total_rows, n_groups);
        const double *row = stats + gc.group * len;  // group 0 of a rejected clip: inside the block (n_groups >= 1), read only if rows != 0
        if (gc.rows != 0 && stats_count(row[0]) > 0.0) {
            if (!WIDE && cached != static_cast<long long>(gc.group)) {
                __syncthreads();  // the lanes still read the pair of the group before
                for (unsigned k = threadIdx.x; k < cols; k += 256) {
                    stat[2 * k] = row[1 + k];
                    stat[2 * k + 1] = variance ? 1.0 / (sqrt(row[1 + cols + k]) + kEps30) : 1.0;
                }
                __syncthreads();
                cached = static_cast<long long>(gc.group);
            }
            auto norm = [&](float v, unsigned col) {
                if (WIDE) {
                    const double inv = variance ? 1.0 / (sqrt(row[1 + cols + col]) + kEps30) : 1.0;
                    return static_cast<float>((static_cast<double>(v) - row[1 + col]) * inv);
                }
                return static_cast<float>((static_cast<double>(v) - stat[2 * col]) * stat[2 * col + 1]);
            };
            // rows r .. r_end of the clip: one run of n elements that starts at a column 0
            // (n <= max(kApplySpan, cols) < 2^30: 32-bit indices inside the run)
            const size_t e0 = static_cast<size_t>(r) * cols;
            const unsigned n = static_cast<unsigned>(r_end - r) * cols;
            const float *src = x + e0;
            float *dst = out + e0;
            const unsigned tb = ((16u - static_cast<unsigned>(reinterpret_cast<uintptr_t>(dst) & 15u)) & 15u) / 4u;
            const unsigned head = n < tb ? n : tb;
            const unsigned quads = (n - head) / 4;
            const unsigned tail = n - head - quads * 4;
            if (threadIdx.x < head + tail) {  // at most 6 single elements
                const unsigned e = threadIdx.x < head ? threadIdx.x : quads * 4 + threadIdx.x;
                dst[e] = norm(src[e], e % cols);
            }
            for (unsigned q = threadIdx.x; q < quads; q += 256) {
                const unsigned e = head + 4 * q;
                const float4u v = *reinterpret_cast<const float4u *>(src + e);
                unsigned col = e % cols;
                float4a w;
                for (int j = 0; j < 4; ++j) {
                    w[j] = norm(v[j], col);
                    if (++col == cols) col = 0;
                }
                *reinterpret_cast<float4a *>(dst + e) = w;
            }
        }
        r = r_end;
    }
}

int check_group_args(const void *vec, const void *off, const void *stats_or_out, size_t n_clips, size_t total_rows, size_t cols, size_t n_groups)
{
    if (!vec || !off || !stats_or_out) return fail(SS_ERR_ARG, "null buffer");
    if (cols == 0) return fail(SS_ERR_ARG, "empty feature matrix (cols == 0)");
    if (n_groups == 0) return fail(SS_ERR_ARG, "n_groups must be >= 1");
    if (total_rows >= (1ull << 31) || cols >= (1ull << 30) || n_clips >= (1ull << 31) || n_groups >= (1ull << 31))
        return fail(SS_ERR_ARG, "feature block too large: total_rows, n_clips and n_groups must be below 2^31, cols below 2^30");
    return SS_OK;
}

size_t stats_bytes(size_t n_groups, size_t cols) { return n_groups * (2 * cols + 1) * sizeof(double); }

// what the apply call rejects beyond check_group_args: out == vec is the in-place call, any other overlap is refused
int check_apply_ranges(const float *vec, const double *stats, const float *out, size_t total_rows, size_t cols, size_t n_groups)
{
    if (!out) return fail(SS_ERR_ARG, "null buffer");
    const size_t bytes = total_rows * cols * sizeof(float);
    if (out != vec && ranges_overlap(vec, bytes, out, bytes)) return fail(SS_ERR_ARG, "out overlaps vec partially: only out == vec is in place");
    if (ranges_overlap(stats, stats_bytes(n_groups, cols), out, bytes)) return fail(SS_ERR_ARG, "the statistics block overlaps out");
    return SS_OK;
}

// ---- the scratch blocks of the statistics pass ----
// Outside a stream capture a scratch block is a stream-ordered allocation (hipMallocAsync / hipFreeAsync), as everywhere in the
// library.  Inside a capture it is NOT: an allocation node in front of the per-clip kernel made replays after the first read rows
// of an earlier replay from the block once the memory pool had other free blocks to hand out (measured), so a captured
// call takes its scratch from one plain device block per device instead -- the capture block.  Every call outside a capture makes
// sure the capture block is at least as large as its own scratch (hipMalloc on growth only; an outgrown block is kept, captured
// graphs may still name it), so the usual warm-up call in front of a capture is what sizes it; a captured call that finds it too
// small fails with SS_ERR_HIP and says so.  Graphs that hold the statistics call share the block: they must not replay concurrently.
struct CaptureBlock {
    void *p = nullptr;
    size_t bytes = 0;
};
std::mutex g_capture_mutex;
std::map<int, CaptureBlock> g_capture_blocks;  // by device

struct Scratch {
    void *p = nullptr;
    bool stream_ordered = false;
    hipStream_t s = nullptr;
    int take(size_t bytes, hipStream_t stream)
    {
        s = stream;
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        if (stream && hipStreamIsCapturing(stream, &cs) != hipSuccess) (void)hipGetLastError();  // (the null stream cannot capture)
        int dev = 0;
        hipError_t e = hipGetDevice(&dev);
        if (e != hipSuccess) return hip_fail(e, "hipGetDevice");
        {
            std::lock_guard<std::mutex> lock(g_capture_mutex);
            CaptureBlock &b = g_capture_blocks[dev];
            if (cs == hipStreamCaptureStatusActive) {
                if (b.bytes < bytes)
                    return fail(SS_ERR_HIP, "grouped CMVN statistics inside a stream capture need " + std::to_string(bytes) + " bytes of scratch and " +
                                                std::to_string(b.bytes) + " are set aside: run the call once with these sizes outside the capture");
                p = b.p;
                return SS_OK;
            }
            if (b.bytes < bytes) {
                size_t want = 1 << 16;
                while (want < bytes) want *= 2;
                void *fresh = nullptr;
                if (hipMalloc(&fresh, want) == hipSuccess) b = CaptureBlock{fresh, want};  // the outgrown block stays allocated
                else (void)hipGetLastError();  // (another thread's capture may forbid it: the next call tries again)
            }
        }
        e = hipMallocAsync(&p, bytes, stream);
        if (e != hipSuccess) return hip_fail(e, "hipMallocAsync");
        stream_ordered = true;
        return SS_OK;
    }
    int give()
    {
        if (!stream_ordered) return SS_OK;
        stream_ordered = false;
        const hipError_t e = hipFreeAsync(p, s);
        return e == hipSuccess ? SS_OK : hip_fail(e, "hipFreeAsync");
    }
};

// d_clip: [n_clips x 2 cols] doubles of scratch (mean_b, var_b)
int launch_stats(const float *d_vec, size_t n_clips, const long long *off, size_t total_rows, size_t cols, const int *grp, size_t n_groups,
                 double *d_stats, double *d_clip, hipStream_t s)
{
    const unsigned tiles = static_cast<unsigned>(std::min<size_t>(kStatTilesY, (cols + kCmvnTile - 1) / kCmvnTile));
    hipLaunchKernelGGL(ss_cmvn_clip_stats_kernel, dim3(static_cast<unsigned>(n_clips), tiles), dim3(256), 0, s, d_vec, off, grp, d_clip,
                       static_cast<unsigned long long>(total_rows), static_cast<unsigned>(cols), static_cast<unsigned>(n_groups));
    hipLaunchKernelGGL(ss_cmvn_fold_kernel, dim3(static_cast<unsigned>(n_groups)), dim3(256), 0, s, off, grp, d_clip, d_stats,
                       static_cast<unsigned>(n_clips), static_cast<unsigned long long>(total_rows), static_cast<unsigned>(cols),
                       static_cast<unsigned>(n_groups));
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? SS_OK : hip_fail(e, "ss_cmvn_stats kernels");
}

size_t clip_bytes(size_t n_clips, size_t cols) { return n_clips * 2 * cols * sizeof(double); }

int launch_apply(const float *d_vec, size_t n_clips, const long long *off, size_t total_rows, size_t cols, const int *grp, size_t n_groups,
                 const double *d_stats, int variance, float *d_out, hipStream_t s)
{
    const unsigned span_rows = static_cast<unsigned>(std::max<size_t>(1, kApplySpan / cols));
    const dim3 grid(static_cast<unsigned>((total_rows + span_rows - 1) / span_rows));
    const unsigned n = static_cast<unsigned>(n_clips), c = static_cast<unsigned>(cols), ng = static_cast<unsigned>(n_groups);
    const unsigned long long tr = total_rows;
    if (cols <= kApplyLdsCols) hipLaunchKernelGGL(ss_cmvn_apply_kernel<false>, grid, dim3(256), 0, s, d_vec, off, grp, d_stats, d_out, n, tr, c, ng, span_rows, variance);
    else hipLaunchKernelGGL(ss_cmvn_apply_kernel<true>, grid, dim3(256), 0, s, d_vec, off, grp, d_stats, d_out, n, tr, c, ng, span_rows, variance);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? SS_OK : hip_fail(e, "ss_cmvn_apply_kernel");
}

// the tables of a host-pointer call: the segment table, then the group ids (clip_group may be null where the call allows it)
int check_host_tables(const int64_t *offsets, const int32_t *clip_group, size_t n_clips, size_t total_rows, size_t n_groups)
{
    int rc = check_clip_table(offsets, n_clips, total_rows);
    if (rc == SS_OK && clip_group) rc = check_clip_groups(clip_group, n_clips, n_groups);
    return rc;
}

}  // namespace

}  // namespace ss

extern "C" {

int ss_cmvn_stats_len(size_t cols, size_t *len)
{
    if (!len) return ss::fail(SS_ERR_ARG, "null output");
    if (cols == 0) return ss::fail(SS_ERR_ARG, "empty feature matrix (cols == 0)");
    if (cols >= (1ull << 30)) return ss::fail(SS_ERR_ARG, "cols must be below 2^30");
    *len = 2 * cols + 1;
    return SS_OK;
}

int ss_cmvn_stats_to_kaldi(const double *stats, size_t cols, double *kaldi)
{
#pragma clang fp contract(off)
    if (!stats || !kaldi) return ss::fail(SS_ERR_ARG, "null buffer");
    if (cols == 0 || cols >= (1ull << 30)) return ss::fail(SS_ERR_ARG, "cols must be in [1, 2^30)");
    const double n = stats[0] >= 1.0 && stats[0] < INFINITY ? stats[0] : 0.0;
    for (size_t c = 0; c < cols; ++c) {
        const double mean = stats[1 + c], var = stats[1 + cols + c];
        kaldi[c] = n > 0.0 ? n * mean : 0.0;
        kaldi[cols + 1 + c] = n > 0.0 ? n * (var + mean * mean) : 0.0;
    }
    kaldi[cols] = n;
    kaldi[2 * cols + 1] = 0.0;
    return SS_OK;
}

int ss_cmvn_stats_from_kaldi(const double *kaldi, size_t cols, double *stats)
{
#pragma clang fp contract(off)
    if (!stats || !kaldi) return ss::fail(SS_ERR_ARG, "null buffer");
    if (cols == 0 || cols >= (1ull << 30)) return ss::fail(SS_ERR_ARG, "cols must be in [1, 2^30)");
    const double count = kaldi[cols];
    const double n = count >= 1.0 && count < INFINITY ? count : 0.0;
    stats[0] = n;
    for (size_t c = 0; c < cols; ++c) {
        const double mean = n > 0.0 ? kaldi[c] / n : 0.0;
        const double var = n > 0.0 ? kaldi[cols + 1 + c] / n - mean * mean : 0.0;
        stats[1 + c] = mean;
        stats[1 + cols + c] = var < 0.0 ? 0.0 : var;  // a NaN passes
    }
    return SS_OK;
}

int ss_cmvn_stats_packed_device(const float *d_vec, size_t n_clips, const int64_t *d_offsets, size_t total_rows, size_t cols,
                                const int32_t *d_clip_group, size_t n_groups, double *d_stats, void *stream)
{
    if (n_clips == 0) return SS_OK;
    const int rc = ss::check_group_args(d_vec, d_offsets, d_stats, n_clips, total_rows, cols, n_groups);
    if (rc) return rc;
    if (ss::ranges_overlap(d_stats, ss::stats_bytes(n_groups, cols), d_vec, total_rows * cols * sizeof(float)))
        return ss::fail(SS_ERR_ARG, "the statistics block overlaps vec");
    if (total_rows == 0) return SS_OK;  // no clip can own a row
    hipStream_t st = static_cast<hipStream_t>(stream);
    ss::Scratch clip;
    int rc2 = clip.take(ss::clip_bytes(n_clips, cols), st);
    if (rc2) return rc2;
    rc2 = ss::launch_stats(d_vec, n_clips, reinterpret_cast<const long long *>(d_offsets), total_rows, cols, reinterpret_cast<const int *>(d_clip_group),
                           n_groups, d_stats, static_cast<double *>(clip.p), st);
    const int rc3 = clip.give();
    return rc2 ? rc2 : rc3;
}

int ss_cmvn_apply_packed_device(const float *d_vec, size_t n_clips, const int64_t *d_offsets, size_t total_rows, size_t cols,
                                const int32_t *d_clip_group, size_t n_groups, const double *d_stats, int variance_normalization, float *d_out,
                                void *stream)
{
    if (n_clips == 0) return SS_OK;
    int rc = ss::check_group_args(d_vec, d_offsets, d_stats, n_clips, total_rows, cols, n_groups);
    if (rc || (rc = ss::check_apply_ranges(d_vec, d_stats, d_out, total_rows, cols, n_groups))) return rc;
    if (total_rows == 0) return SS_OK;
    return ss::launch_apply(d_vec, n_clips, reinterpret_cast<const long long *>(d_offsets), total_rows, cols, reinterpret_cast<const int *>(d_clip_group),
                            n_groups, d_stats, variance_normalization, d_out, static_cast<hipStream_t>(stream));
}

int ss_cmvn_grouped_packed_device(const float *d_vec, size_t n_clips, const int64_t *d_offsets, size_t total_rows, size_t cols,
                                  const int32_t *d_clip_group, size_t n_groups, int variance_normalization, float *d_out, void *stream)
{
    if (n_clips == 0) return SS_OK;
    int rc = ss::check_group_args(d_vec, d_offsets, d_out, n_clips, total_rows, cols, n_groups);
    if (rc) return rc;
    const size_t bytes = total_rows * cols * sizeof(float);
    if (d_out != d_vec && ss::ranges_overlap(d_vec, bytes, d_out, bytes)) return ss::fail(SS_ERR_ARG, "out overlaps vec partially: only out == vec is in place");
    if (total_rows == 0) return SS_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    // one scratch block: the per-clip rows, then the zeroed statistics block of this call
    const size_t cb = ss::clip_bytes(n_clips, cols), sb = ss::stats_bytes(n_groups, cols);
    ss::Scratch block;
    if ((rc = block.take(cb + sb, s))) return rc;
    double *d_clip = static_cast<double *>(block.p), *d_stats = d_clip + cb / sizeof(double);
    const hipError_t e = hipMemsetAsync(d_stats, 0, sb, s);
    if (e != hipSuccess) rc = ss::hip_fail(e, "hipMemsetAsync");
    const long long *off = reinterpret_cast<const long long *>(d_offsets);
    const int *grp = reinterpret_cast<const int *>(d_clip_group);
    if (rc == SS_OK) rc = ss::launch_stats(d_vec, n_clips, off, total_rows, cols, grp, n_groups, d_stats, d_clip, s);
    if (rc == SS_OK) rc = ss::launch_apply(d_vec, n_clips, off, total_rows, cols, grp, n_groups, d_stats, variance_normalization, d_out, s);
    const int rc_give = block.give();
    if (rc == SS_OK) rc = rc_give;
    return rc;
}

// host-pointer forms (synchronous): the tables are checked on the host before the device is touched

int ss_cmvn_stats_packed(const float *vec, size_t n_clips, const int64_t *offsets, size_t total_rows, size_t cols, const int32_t *clip_group,
                         size_t n_groups, double *stats)
{
    if (n_clips == 0) return SS_OK;
    int rc = ss::check_group_args(vec, offsets, stats, n_clips, total_rows, cols, n_groups);
    if (rc) return rc;
    if (ss::ranges_overlap(stats, ss::stats_bytes(n_groups, cols), vec, total_rows * cols * sizeof(float)))
        return ss::fail(SS_ERR_ARG, "the statistics block overlaps vec");
    if ((rc = ss::check_host_tables(offsets, clip_group, n_clips, total_rows, n_groups))) return rc;
    if (offsets[n_clips] == 0) return SS_OK;
    if (!ss::have_device()) return ss::no_device();
    const size_t sb = ss::stats_bytes(n_groups, cols);
    ss::HostStage st("ss_cmvn_stats_packed");
    const float *d_vec = st.up(vec, total_rows * cols * sizeof(float));
    const int64_t *d_off = st.up(offsets, (n_clips + 1) * sizeof(int64_t));
    const int32_t *d_grp = clip_group ? st.up(clip_group, n_clips * sizeof(int32_t)) : nullptr;
    double *d_stats = st.up(stats, sb);
    if (st.ok()) st.ran(ss_cmvn_stats_packed_device(d_vec, n_clips, d_off, total_rows, cols, d_grp, n_groups, d_stats, nullptr));
    st.sync();
    st.down(stats, d_stats, sb);
    return st.status();
}

int ss_cmvn_apply_packed(const float *vec, size_t n_clips, const int64_t *offsets, size_t total_rows, size_t cols, const int32_t *clip_group,
                         size_t n_groups, const double *stats, int variance_normalization, float *out)
{
    if (n_clips == 0) return SS_OK;
    int rc = ss::check_group_args(vec, offsets, stats, n_clips, total_rows, cols, n_groups);
    if (rc || (rc = ss::check_apply_ranges(vec, stats, out, total_rows, cols, n_groups)) ||
        (rc = ss::check_host_tables(offsets, clip_group, n_clips, total_rows, n_groups)))
        return rc;
    if (offsets[n_clips] == 0) return SS_OK;
    if (!ss::have_device()) return ss::no_device();
    // the rows of a clip that is left out (id -1, a group without statistics) keep the caller's bytes: out goes up first
    const size_t bytes = total_rows * cols * sizeof(float), written = static_cast<size_t>(offsets[n_clips]) * cols * sizeof(float);
    ss::HostStage st("ss_cmvn_apply_packed");
    const float *d_vec = st.up(vec, bytes);
    const int64_t *d_off = st.up(offsets, (n_clips + 1) * sizeof(int64_t));
    const int32_t *d_grp = clip_group ? st.up(clip_group, n_clips * sizeof(int32_t)) : nullptr;
    const double *d_stats = st.up(stats, ss::stats_bytes(n_groups, cols));
    float *d_out = st.room<float>(bytes);
    st.fill(d_out, out, written);
    if (st.ok())
        st.ran(ss_cmvn_apply_packed_device(d_vec, n_clips, d_off, total_rows, cols, d_grp, n_groups, d_stats, variance_normalization, d_out, nullptr));
    st.sync();
    st.down(out, d_out, written);
    return st.status();
}

int ss_cmvn_grouped_packed(const float *vec, size_t n_clips, const int64_t *offsets, size_t total_rows, size_t cols, const int32_t *clip_group,
                           size_t n_groups, int variance_normalization, float *out)
{
    if (n_clips == 0) return SS_OK;
    int rc = ss::check_group_args(vec, offsets, out, n_clips, total_rows, cols, n_groups);
    if (rc) return rc;
    const size_t bytes = total_rows * cols * sizeof(float);
    if (out != vec && ss::ranges_overlap(vec, bytes, out, bytes)) return ss::fail(SS_ERR_ARG, "out overlaps vec partially: only out == vec is in place");
    if ((rc = ss::check_host_tables(offsets, clip_group, n_clips, total_rows, n_groups))) return rc;
    if (offsets[n_clips] == 0) return SS_OK;
    if (!ss::have_device()) return ss::no_device();
    const size_t written = static_cast<size_t>(offsets[n_clips]) * cols * sizeof(float);
    ss::HostStage st("ss_cmvn_grouped_packed");
    const float *d_vec = st.up(vec, bytes);
    const int64_t *d_off = st.up(offsets, (n_clips + 1) * sizeof(int64_t));
    const int32_t *d_grp = clip_group ? st.up(clip_group, n_clips * sizeof(int32_t)) : nullptr;
    float *d_out = st.room<float>(bytes);
    st.fill(d_out, out, written);
    if (st.ok()) st.ran(ss_cmvn_grouped_packed_device(d_vec, n_clips, d_off, total_rows, cols, d_grp, n_groups, variance_normalization, d_out, nullptr));
    st.sync();
    st.down(out, d_out, written);
    return st.status();
}

}  // extern "C"
