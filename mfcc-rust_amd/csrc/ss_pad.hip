// Padded-batch collation of packed rows: ss_pad_packed* turns the packed dialect (a float block [total_rows x cols] and a device
// table row_offsets[n_clips + 1]) into the rectangular batch a model takes -- [n_clips x max_rows x cols] (BTC) or [n_clips x cols x
// max_rows] (BCT), f32 / f16 / bf16 -- with the conversion, the transpose, the pad filling and the per-clip lengths in ONE launch
// whose grid depends on n_clips, max_rows and cols only.  The definition is the ss_pad_* comment of include/speechsauce_amd.h; the
// reference crate has no such stage, so this file restates nothing of it.
//
// Work split.  Workgroup (b, y) serves clip b = blockIdx.x together with the gridDim.y - 1 others of that clip (packed_split); the
// first of them writes lengths[b].  A clip's bits depend on its own rows, max_rows and the scalars: every output element is written
// by exactly one lane from values it selected itself, whichever workgroup that lane sits in.
//
// BTC, and the block of an empty or bad clip in either layout (pad_flat): the clip's block is one contiguous run of max_rows * cols
// output elements, the first kept * cols of them the conversion of one contiguous input run, the rest pad.  It is walked as a flat
// stream: 16-byte stores (4 floats, or 8 halves packed pairwise into dwords) from the block's first 16-byte boundary on, element
// stores for the up to VE - 1 elements in front of it and behind the last whole store, and for the one group that the end of the
// source run cuts (every other group is all source or all pad).  The source run starts at ro[b] * cols floats
// -- dword aligned only -- and is read with dword-aligned wide loads (legal in the unaligned access mode the HSA ABI sets; ss_kaldi_body.h's
// load_pair4 relies on the same).  No LDS, no barrier.
//
// BCT (pad_transpose): a per-clip transpose through LDS in tiles of kTileT = 128 time rows x kTileC = 32 columns, column tiles
// fastest so that neighbouring workgroups share input rows.  Output row c of the clip starts at element c * max_rows of the block:
// with odd max_rows every row has its own 16-byte phase, so row c's 16-byte stores cover t = head_c + VE * g, head_c = the elements
// up to the row's first 16-byte boundary (0 .. VE - 1).  Tile k therefore serves t in [head_c + 128 k, head_c + 128 (k + 1)) of every
// row and holds the kTileT + 8 = 136 time rows [128 k, 128 k + 136) that all these windows lie in; tile 0 also serves the heads, and
// a row's last partial group goes out as element stores.  Rows at and past `kept` hold pad_value in the tile, so the row tails need
// no second pass.  The tile is tall because the stores want long runs: a tile writes 512 (f32) or 256 (halves) contiguous bytes of
// every output row, and against a tile of 64 rows, in one process, that took 17 % (f32) and 19 % / 14 % (halves, cols 80 / 240)
// off the call.
//   LDS layout: 136 rows of 32 floats, no padding; the float of (r, c) lives at word r * 32 + (c ^ swz(r)), swz(r) = 4 * ((r >> lg
//   VE) & 7).  Bank derivation (cdna_hip_programming.md section 2: ds_write_b32 / ds_read_b32 / ds_read2_b32 use bank = word % 32, and only
//   lanes of the same 32-lane half conflict):
//   - write side: thread tid stores column tid & 31 of row (tid >> 5) + 8 i.  The 32 lanes of a half share r, so their banks are
//     (tid & 31) ^ swz(r): a permutation of 0 .. 31 -- conflict-free.
//   - read side: lane l of wave w holds column c = 8 w + 4 (l >> 5) + (l & 3) and group tg = (l >> 2) & 7; its j-th read is row r
//     = head_c + VE * (tg + 8 p) + j, so (r >> lg VE) & 7 = (tg + d_c) & 7 with d_c = (head_c + j) >> lg VE in {0, 1}, the same for
//     every lane of that column.  Bank = c ^ 4 * ((tg + d_c) & 7) = (l & 3) + 4 * ((2 w + (l >> 5)) ^ ((tg + d_c) & 7)): within a half the
//     eight tg of one column give eight distinct multiples of 4 and the four columns differ in the low two bits -- 32 distinct
//     banks, conflict-free whatever the rows' phases are.  (A padded pitch cannot give that: the per-row shift head_c moves whole
//     columns onto each other's banks.)
//   Stores: eight consecutive lanes (tg) of one column write 8 x 16 = 128 contiguous bytes per pass p (four passes in f32, two in
//   the halves); a 16-bit lane packs two consecutive t into each dword, so there is no 2-byte store outside the heads and tails.
//
// Conversion: f32 is moved as bits (no arithmetic instruction sees it); f16 is v_cvt_f16_f32 in the default round-to-nearest-even
// mode with f16 denormals enabled (the HIP default: results in the denormal range are produced, not flushed); bf16 is the integer
// formula (bits + 0x7FFF + ((bits >> 16) & 1)) >> 16 of the header -- no float instruction, so f32 denormal inputs are not flushed
// -- with a NaN kept a NaN: the truncated pattern with the quiet bit set (the formula would carry a payload of all ones into the
// exponent and sign).
#include "ss_device.h"
#include "ss_hip_staging.h"
#include "ss_host_checks.h"
#include "ss_internal.h"

#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

namespace ss {

namespace {

constexpr unsigned kTileT = 128, kTileC = 32;  // the BCT tile: time rows x columns
constexpr unsigned kTileRows = kTileT + 8;    // the time rows a tile holds: the rows' windows are shifted by up to VE - 1 <= 7
constexpr unsigned kFlatChunk = 1024;         // 16-byte groups per workgroup step of the flat walk: four per lane

template <int DT>
struct PadType {
    static constexpr unsigned ES = DT == SS_PAD_F32 ? 4 : 2;  // bytes of an output element
    static constexpr unsigned VE = 16 / ES;                  // elements of a 16-byte store
    static constexpr unsigned LG = DT == SS_PAD_F32 ? 2 : 3;  // lg VE
};

// conv of the header, as the low bits of a word
template <int DT>
__device__ __forceinline__ unsigned conv_bits(float v)
{
    const unsigned u = __float_as_uint(v);
    if constexpr (DT == SS_PAD_F32) {
        return u;
    } else if constexpr (DT == SS_PAD_F16) {
        const _Float16 h = static_cast<_Float16>(v);
        unsigned short s;
        __builtin_memcpy(&s, &h, sizeof s);
        return s;
    } else {
        if ((u & 0x7fffffffu) > 0x7f800000u) return (u >> 16) | 0x40u;  // NaN stays NaN
        return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
    }
}

template <int DT>
__device__ __forceinline__ void store_elem(unsigned char *p, size_t e, float v)
{
    if constexpr (DT == SS_PAD_F32) reinterpret_cast<unsigned *>(p)[e] = conv_bits<DT>(v);
    else reinterpret_cast<unsigned short *>(p)[e] = static_cast<unsigned short>(conv_bits<DT>(v));
}

// VE elements, the first at the 16-byte aligned element e of p
template <int DT>
__device__ __forceinline__ void store_group(unsigned char *p, size_t e, const float *v)
{
    uint4 w;
    if constexpr (DT == SS_PAD_F32) {
        w = make_uint4(conv_bits<DT>(v[0]), conv_bits<DT>(v[1]), conv_bits<DT>(v[2]), conv_bits<DT>(v[3]));
    } else {
        w = make_uint4(conv_bits<DT>(v[0]) | conv_bits<DT>(v[1]) << 16, conv_bits<DT>(v[2]) | conv_bits<DT>(v[3]) << 16,
                       conv_bits<DT>(v[4]) | conv_bits<DT>(v[5]) << 16, conv_bits<DT>(v[6]) | conv_bits<DT>(v[7]) << 16);
    }
    *reinterpret_cast<uint4 *>(p + e * PadType<DT>::ES) = w;
}

// elements from p up to its first 16-byte boundary (p is aligned to its element)
template <int DT>
__device__ __forceinline__ unsigned to_boundary(const unsigned char *p)
{
    return ((16u - static_cast<unsigned>(reinterpret_cast<uintptr_t>(p) & 15u)) & 15u) / PadType<DT>::ES;
}

// dst[e] = conv(e < n_src ? src[e] : pad) for e < n: the flat walk
template <int DT>
__device__ __forceinline__ void pad_flat(const float *__restrict__ src, size_t n_src, unsigned char *__restrict__ dst, size_t n, float pad)
{
    constexpr unsigned VE = PadType<DT>::VE;
    const unsigned tb = to_boundary<DT>(dst);
    const unsigned head = n < tb ? static_cast<unsigned>(n) : tb;
    const size_t groups = (n - head) / VE;
    const unsigned tail = static_cast<unsigned>(n - head - groups * VE);
    // the one group that the end of the source run cuts goes out as single elements too: every other group is all source or all pad
    const size_t none = ~static_cast<size_t>(0);
    const size_t cut = n_src > head && (n_src - head) % VE != 0 && (n_src - head) / VE < groups ? (n_src - head) / VE : none;
    const unsigned singles = head + tail + (cut != none ? VE : 0u);
    if (blockIdx.y == 0 && threadIdx.x < singles) {  // at most 3 (VE - 1) + 1 single elements
        const unsigned i = threadIdx.x;
        const size_t e = i < head ? i : i < head + tail ? groups * VE + i : head + cut * VE + (i - head - tail);
        store_elem<DT>(dst, e, e < n_src ? src[e] : pad);
    }
    // Four groups per lane and step, their loads issued back to back: a group that takes no source loads group 0 instead (in bounds
    // whenever any group is all source), so that no load sits behind a branch and waits for the one before it.
    const bool any_src = n_src >= head + VE && groups > 0;  // uniform per workgroup
    for (size_t g0 = static_cast<size_t>(blockIdx.y) * kFlatChunk; g0 < groups; g0 += static_cast<size_t>(gridDim.y) * kFlatChunk) {
        constexpr unsigned U = kFlatChunk / 256;
        float v[U][VE] = {};
        size_t q[U];
        bool live[U], from_src[U];
#pragma unroll
        for (unsigned u = 0; u < U; ++u) {
            const size_t g = g0 + u * 256 + threadIdx.x;
            live[u] = g < groups && g != cut;
            q[u] = head + g * VE;
            from_src[u] = live[u] && q[u] + VE <= n_src;
        }
        if (any_src) {
#pragma unroll
            for (unsigned u = 0; u < U; ++u)
                __builtin_memcpy(v[u], __builtin_assume_aligned(src + (from_src[u] ? q[u] : head), 4), sizeof v[u]);  // dword-aligned wide loads
        }
#pragma unroll
        for (unsigned u = 0; u < U; ++u) {
#pragma unroll
            for (unsigned j = 0; j < VE; ++j) v[u][j] = from_src[u] ? v[u][j] : pad;
            if (live[u]) store_group<DT>(dst, q[u], v[u]);
        }
    }
}

template <int DT>
__device__ __forceinline__ unsigned swz(unsigned r)
{
    return ((r >> PadType<DT>::LG) & 7u) << 2;
}

// dst[c][t] = conv(t < kept ? src[t][c] : pad) for c < cols, t < max_rows: the transpose through LDS (kept >= 1)
template <int DT>
__device__ __forceinline__ void pad_transpose(const float *__restrict__ src, unsigned kept, unsigned char *__restrict__ dst, unsigned cols,
                                              unsigned max_rows, float pad)
{
    constexpr unsigned VE = PadType<DT>::VE, ES = PadType<DT>::ES;
    __shared__ float tile[kTileRows * kTileC];
    const unsigned n_ct = (cols + kTileC - 1) / kTileC;
    const unsigned long long n_tiles = static_cast<unsigned long long>((max_rows + kTileT - 1) / kTileT) * n_ct;
    const unsigned tid = threadIdx.x, lc = tid & 31u, lane = tid & 63u;
    const unsigned ci = (tid >> 6) * 8u + ((lane >> 5) << 2) + (lane & 3u), tg = (lane >> 2) & 7u;
    for (unsigned long long ti = blockIdx.y; ti < n_tiles; ti += gridDim.y) {  // uniform per workgroup
        const unsigned k = static_cast<unsigned>(ti / n_ct), c0 = static_cast<unsigned>(ti - static_cast<unsigned long long>(k) * n_ct) * kTileC;
        const unsigned t0 = k * kTileT;
        // Seventeen loads per lane, issued back to back: the row and the column are clamped into the clip (kept >= 1), so no load sits
        // behind a branch and waits for the one before it; what a clamped load fetched is replaced by pad (rows) or never read (columns).
        float in[kTileRows / 8] = {};
        const unsigned cl = min(c0 + lc, cols - 1);
        if (t0 < kept) {  // uniform per workgroup: a tile behind the clip's rows loads nothing
#pragma unroll
            for (unsigned i = 0; i < kTileRows / 8; ++i) in[i] = src[static_cast<size_t>(min(t0 + (tid >> 5) + 8 * i, kept - 1)) * cols + cl];
        }
#pragma unroll
        for (unsigned i = 0; i < kTileRows / 8; ++i) {
            const unsigned r = (tid >> 5) + 8 * i;
            tile[r * kTileC + (lc ^ swz<DT>(r))] = t0 + r < kept ? in[i] : pad;
        }
        __syncthreads();
        const unsigned c = c0 + ci;
        if (c < cols) {
            unsigned char *rowp = dst + static_cast<size_t>(c) * max_rows * ES;
            const unsigned head = to_boundary<DT>(rowp);
            if (k == 0 && tg == 0) {  // the elements in front of the row's first 16-byte boundary
                const unsigned n = head < max_rows ? head : max_rows;
                for (unsigned e = 0; e < n; ++e) store_elem<DT>(rowp, e, tile[e * kTileC + (ci ^ swz<DT>(e))]);
            }
#pragma unroll
            for (unsigned p = 0; p < kTileT / (8 * VE); ++p) {
                const unsigned r = head + VE * (tg + 8 * p), t = t0 + r;
                if (t >= max_rows) continue;
                float v[VE];
#pragma unroll
                for (unsigned j = 0; j < VE; ++j) v[j] = tile[(r + j) * kTileC + (ci ^ swz<DT>(r + j))];
                if (max_rows - t >= VE) {
                    store_group<DT>(rowp, t, v);
                } else {  // the row's last partial group
#pragma unroll
                    for (unsigned j = 0; j < VE - 1; ++j)
                        if (j < max_rows - t) store_elem<DT>(rowp, t + j, v[j]);
                }
            }
        }
        __syncthreads();
    }
}

template <int LAYOUT, int DT>
__global__ __launch_bounds__(256) void ss_pad_packed_kernel(const float *__restrict__ x, const long long *__restrict__ ro, unsigned char *__restrict__ out,
                                                           int *lengths, unsigned long long total_rows, unsigned cols, unsigned max_rows, float pad)
{
    const unsigned b = blockIdx.x;
    const long long lo = ro[b], hi = ro[b + 1];
    // unlike packed_segment this tells an empty clip (0 rows) from a bad one (-1); total_rows < 2^31: the row count fits
    const bool good = lo >= 0 && lo <= hi && static_cast<unsigned long long>(hi) <= total_rows;
    const unsigned rows = good ? static_cast<unsigned>(hi - lo) : 0u, kept = rows < max_rows ? rows : max_rows;
    if (blockIdx.y == 0 && threadIdx.x == 0) lengths[b] = good ? static_cast<int>(kept) : -1;
    const size_t block = static_cast<size_t>(max_rows) * cols;
    unsigned char *dst = out + static_cast<size_t>(b) * block * PadType<DT>::ES;
    const float *src = x + (kept ? static_cast<size_t>(lo) * cols : 0);  // never formed from a bad offset
    if constexpr (LAYOUT == SS_PAD_BTC) {
        pad_flat<DT>(src, static_cast<size_t>(kept) * cols, dst, block, pad);
    } else {
        if (kept == 0) pad_flat<DT>(src, 0, dst, block, pad);  // uniform per workgroup: the barriers of the other branch are safe
        else pad_transpose<DT>(src, kept, dst, cols, max_rows, pad);
    }
}

// ---- host side ----

constexpr unsigned long long kCountLimit = 1ull << 31;

int out_bytes(size_t n_clips, size_t max_rows, size_t cols, int dtype, size_t &bytes)
{
    if (dtype != SS_PAD_F32 && dtype != SS_PAD_F16 && dtype != SS_PAD_BF16) return fail(SS_ERR_ARG, "dtype must be SS_PAD_F32, SS_PAD_F16 or SS_PAD_BF16");
    size_t n = 0;
    if (__builtin_mul_overflow(n_clips, max_rows, &n) || __builtin_mul_overflow(n, cols, &n) ||
        __builtin_mul_overflow(n, static_cast<size_t>(dtype == SS_PAD_F32 ? 4 : 2), &n))
        return fail(SS_ERR_ARG, "the padded batch is too large: n_clips * max_rows * cols bytes overflow size_t");
    bytes = n;
    return SS_OK;
}

// what both forms reject before the device is touched (the table and the overlap rule apart)
int check_scalars(size_t n_clips, size_t total_rows, size_t cols, size_t max_rows, int layout, int dtype, const void *out, size_t &bytes)
{
    if (cols == 0) return fail(SS_ERR_ARG, "empty feature matrix (cols == 0)");
    if (max_rows == 0) return fail(SS_ERR_ARG, "max_rows must be at least 1");
    if (layout != SS_PAD_BTC && layout != SS_PAD_BCT) return fail(SS_ERR_ARG, "layout must be SS_PAD_BTC or SS_PAD_BCT");
    if (n_clips >= kCountLimit || total_rows >= kCountLimit || cols >= kCountLimit || max_rows >= kCountLimit)
        return fail(SS_ERR_ARG, "n_clips, total_rows, cols and max_rows must be below 2^31");
    const int rc = out_bytes(n_clips, max_rows, cols, dtype, bytes);
    if (rc) return rc;
    if (reinterpret_cast<uintptr_t>(out) % (dtype == SS_PAD_F32 ? 4u : 2u)) return fail(SS_ERR_ARG, "out is not aligned to its element size");
    return SS_OK;
}

template <int LAYOUT, int DT>
void launch(const float *d_vec, size_t n_clips, const int64_t *d_ro, size_t total_rows, size_t cols, size_t max_rows, float pad, void *d_out,
            int32_t *d_lengths, unsigned split, hipStream_t stream)
{
    hipLaunchKernelGGL((ss_pad_packed_kernel<LAYOUT, DT>), dim3(static_cast<unsigned>(n_clips), split), dim3(256), 0, stream, d_vec,
                       reinterpret_cast<const long long *>(d_ro), static_cast<unsigned char *>(d_out), reinterpret_cast<int *>(d_lengths),
                       static_cast<unsigned long long>(total_rows), static_cast<unsigned>(cols), static_cast<unsigned>(max_rows), pad);
}

}  // namespace

}  // namespace ss

extern "C" {

int ss_pad_packed_out_bytes(size_t n_clips, size_t max_rows, size_t cols, int dtype, size_t *bytes)
{
    if (!bytes) return ss::fail(SS_ERR_ARG, "null output");
    size_t n = 0;
    const int rc = ss::out_bytes(n_clips, max_rows, cols, dtype, n);
    if (rc) return rc;
    *bytes = n;
    return SS_OK;
}

int ss_pad_packed_device(const float *d_vec, size_t n_clips, const int64_t *d_row_offsets, size_t total_rows, size_t cols, size_t max_rows, int layout,
                         int dtype, float pad_value, void *d_out, int32_t *d_lengths, void *stream)
{
    if (n_clips == 0) return SS_OK;
    if (!d_vec || !d_row_offsets || !d_out || !d_lengths) return ss::fail(SS_ERR_ARG, "null buffer");
    size_t bytes = 0;
    const int rc = ss::check_scalars(n_clips, total_rows, cols, max_rows, layout, dtype, d_out, bytes);
    if (rc) return rc;
    const size_t vbytes = total_rows * cols * sizeof(float);
    if (ss::ranges_overlap(d_vec, vbytes, d_out, bytes)) return ss::fail(SS_ERR_ARG, "out overlaps vec: the call is not in place");
    if (ss::ranges_overlap(d_vec, vbytes, d_lengths, n_clips * sizeof(int32_t))) return ss::fail(SS_ERR_ARG, "lengths overlaps vec");
    // one launch: gridDim.y workgroups share a clip's block -- its 16-byte groups (flat walk) or its tiles (transpose)
    const unsigned long long block = static_cast<unsigned long long>(max_rows) * cols;
    const unsigned long long useful = layout == SS_PAD_BCT
                                          ? static_cast<unsigned long long>((max_rows + ss::kTileT - 1) / ss::kTileT) * ((cols + ss::kTileC - 1) / ss::kTileC)
                                          : (block / (dtype == SS_PAD_F32 ? 4 : 8) + ss::kFlatChunk - 1) / ss::kFlatChunk;
    const unsigned split = ss::packed_split(n_clips, useful);
    const hipStream_t st = static_cast<hipStream_t>(stream);
    static const char *const names[2][3] = {{"ss_pad_packed_kernel<btc,f32>", "ss_pad_packed_kernel<btc,f16>", "ss_pad_packed_kernel<btc,bf16>"},
                                            {"ss_pad_packed_kernel<bct,f32>", "ss_pad_packed_kernel<bct,f16>", "ss_pad_packed_kernel<bct,bf16>"}};
#define SS_PAD_LAUNCH(L, D) ss::launch<L, D>(d_vec, n_clips, d_row_offsets, total_rows, cols, max_rows, pad_value, d_out, d_lengths, split, st)
    if (layout == SS_PAD_BTC) {
        if (dtype == SS_PAD_F32) SS_PAD_LAUNCH(SS_PAD_BTC, SS_PAD_F32);
        else if (dtype == SS_PAD_F16) SS_PAD_LAUNCH(SS_PAD_BTC, SS_PAD_F16);
        else SS_PAD_LAUNCH(SS_PAD_BTC, SS_PAD_BF16);
    } else {
        if (dtype == SS_PAD_F32) SS_PAD_LAUNCH(SS_PAD_BCT, SS_PAD_F32);
        else if (dtype == SS_PAD_F16) SS_PAD_LAUNCH(SS_PAD_BCT, SS_PAD_F16);
        else SS_PAD_LAUNCH(SS_PAD_BCT, SS_PAD_BF16);
    }
#undef SS_PAD_LAUNCH
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return ss::hip_fail(e, "ss_pad_packed_kernel");
    ss::note_kernel(names[layout][dtype]);
    return SS_OK;
}

// host-pointer form (synchronous): the table is checked on the host before the device is touched; the block and the table go up,
// the padded batch and the lengths come down
int ss_pad_packed(const float *vec, size_t n_clips, const int64_t *row_offsets, size_t total_rows, size_t cols, size_t max_rows, int layout, int dtype,
                  float pad_value, void *out, int32_t *lengths)
{
    if (n_clips == 0) return SS_OK;
    if (!vec || !row_offsets || !out || !lengths) return ss::fail(SS_ERR_ARG, "null buffer");
    size_t bytes = 0;
    int rc = ss::check_scalars(n_clips, total_rows, cols, max_rows, layout, dtype, out, bytes);
    if (rc || (rc = ss::check_clip_table(row_offsets, n_clips, total_rows))) return rc;
    if (!ss::have_device()) return ss::no_device();
    const size_t lbytes = n_clips * sizeof(int32_t);
    ss::HostStage st("ss_pad_packed");
    const float *d_in = st.up(vec, total_rows * cols * sizeof(float));
    void *d_out = st.room<void>(bytes);
    const int64_t *d_ro = st.up(row_offsets, (n_clips + 1) * sizeof(int64_t));
    int32_t *d_len = st.room<int32_t>(lbytes);
    if (st.ok()) st.ran(ss_pad_packed_device(d_in, n_clips, d_ro, total_rows, cols, max_rows, layout, dtype, pad_value, d_out, d_len, nullptr));
    st.sync();
    st.down(out, d_out, bytes);
    st.down(lengths, d_len, lbytes);
    return st.status();
}

}  // extern "C"
