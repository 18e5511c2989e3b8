// A fused splice + affine transform of packed rows (Kaldi's splice-feats | transform-feats: LDA / LDA+MLLT, a PCA or whitening
// matrix, the input projection of a low-frame-rate front end, a folded global CMVN): ss_affine_* and ss_affine_splice_packed*.
// The spliced row of ss_splice_packed* is never written: output row g of the block is M * s_g + bias, where s_g is the spliced row
// the splice call would have put at row g.  The definition (include/speechsauce_amd.h) is ONE serial f32 fmaf chain per output
// element over k = 0 .. K4 - 1 ascending, K4 = 4 * ceil(K / 4), both factors +0.0 at and past K -- which is what the f32-input
// matrix instruction of gfx950 computes: v_mfma_f32_16x16x4_f32 is D = fma(a3, b3, fma(a2, b2, fma(a1, b1, fma(a0, b0, C)))), one
// rounding per product, so a chain of K4 / 4 such steps into the same accumulator is the chain of the definition.  K is never split
// across accumulators, lanes or waves, so a row's bits depend on its clip's rows, the matrix and the scalars only: not on its place
// in a tile, the tile's place in the grid or the launch shape.
// The reference crate has no such stage, so this file restates nothing of it.
//
// Operands.  D[16 x 16] = A[16 x 4] * B[4 x 16] + C, lane l: A[i = l & 15][k = l >> 4], B[k = l >> 4][j = l & 15], C/D registers r =
// 0 .. 3 of lane l: D[i = 4 * (l >> 4) + r][j = l & 15].  The MATRIX is A (i: 16 output features), the SPLICED ROWS are B (j: 16
// output rows), so a lane ends with four consecutive output features of one output row: one 16-byte store where out_dim is a
// multiple of 4 and out is 16-byte aligned, single floats otherwise.
//   The k-steps go in groups of four (16 elements of the spliced row); the last group runs only the steps that are left.
//   A comes from the handle's device table in operand order, [feature tile][group][lane][step of the group] (re-laid once at
//   creation, zeros where the feature is >= out_dim or k >= K): one coalesced 16-byte load per lane, group and feature tile, served
//   by L2 (a 40 x 440 matrix is 84 KiB, a 256 x 4096 one 4 MiB).  Staging it in LDS would take the table through LDS once per
//   workgroup and tile of rows -- the same L2 traffic at four waves per workgroup unless the workgroup grew, plus a barrier per
//   slice of k: not built.
//   B is gathered straight from the packed block.  Where cols is a multiple of 4 (and vec 16-byte aligned) four consecutive
//   elements lie in one input row: lane (q, j) loads elements 16 g + 4 q .. + 3 of output row j's spliced row as one 16-byte load
//   and two half exchanges per register pair (v_permlane32_swap, v_permlane16_swap: a 4 x 4 transpose across the wave's four
//   rows of 16 lanes) hand every step its element 16 g + 4 i + q -- the k order of the chain is untouched.  Otherwise a lane loads
//   its element of every step by itself.  Either way the element is column col of the clip's row clamp(j's centre + c - left),
//   (c, col) = divmod(element, cols), kept per lane and advanced without a division.  At stride 1 neighbouring output rows share
//   W - 1 of their W input rows; the vector L1 and L2 serve that reuse (a tile of 16 output rows at +-5 x 40 touches 26 input
//   rows = 4 KiB), HBM sees a row about once.  Staging the tile's input rows in LDS would make the loads one coalesced pass and
//   the operand reads ds_read with the same per-lane (c, col) walk; it would add a barrier per tile and a second path for tiles
//   that straddle clips: not built.  (Measured: the single loads ran 0.31 of the f32 matrix rate, bound by their address
//   arithmetic and cache lookups -- 16 lines per load; the 16-byte loads 0.60.  DESIGN.md section 4.)
// Work split.  A wave owns kRowTiles tiles of 16 output rows and NF <= 4 feature tiles of 16 features: NF * kRowTiles independent
// accumulators (the 16x16x4 form wants two or more: 40 cycles of dependent latency against a 32-cycle issue interval), every A
// value used kRowTiles times and every B value NF times.  Feature tiles beyond four go to blockIdx.y; a workgroup is four waves
// on consecutive row tiles, and the workgroups stride over the block.  The grid depends on total_out_rows, out_dim and in_dim
// only.  No LDS, no barrier, no scratch.
// Per row, not per tile: the clip of output row g comes from the output table (offset_find), is checked against both tables exactly
// as ss_splice_packed_kernel checks it, and gives the row its own clamp; a lane whose row does not exist or whose clip is not
// served supplies +0.0 and stores nothing (its loads are redirected to row 0 of the block and dropped: fetch_b below).
#include "ss_device.h"
#include "ss_hip_staging.h"
#include "ss_host_checks.h"
#include "ss_internal.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

namespace ss {

namespace {

constexpr unsigned kMaxContext = 32;       // left, right and stride: the bounds of ss_splice_packed*
constexpr unsigned kMaxOutDim = 256, kMaxInDim = 4096;
constexpr unsigned kRowTiles = 4;          // tiles of 16 output rows per wave
constexpr unsigned kWaveRows = 16 * kRowTiles, kGroupRows = 4 * kWaveRows;  // output rows per wave / per workgroup pass
constexpr unsigned kMaxGroups = 1024;      // workgroups along x: the rest of a long block is reached by striding
constexpr unsigned long long kCountLimit = 1ull << 31;

typedef float f32x4 __attribute__((ext_vector_type(4)));

// One output row as a lane sees it: where its clip's rows start, how many there are, and the row's centre.  A lane without a row
// (past the block, or a clip that is not served) stands on row 0 of the block, so that every address it forms is a float of vec.
struct AffineRow {
    const float *src;   // the clip's first row
    unsigned last;      // T - 1
    unsigned centre;    // k * stride
    unsigned limit;     // W: the context rows of a spliced row; 0: a lane without a row
};

__device__ __forceinline__ AffineRow affine_row(const AffineArgs &a, unsigned long long g)
{
    AffineRow r{a.x, 0u, 0u, 0u};
    if (g >= a.total_out_rows) return r;
    const unsigned b = offset_find(a.oo, a.n_clips, static_cast<long long>(g));
    const long long lo = a.ro[b], hi = a.ro[b + 1], olo = a.oo[b], ohi = a.oo[b + 1];
    // the served-clip rule of ss_splice_packed_kernel (total_rows, total_out_rows < 2^31: the differences fit once both ends are inside)
    if (!(lo >= 0 && lo < hi && static_cast<unsigned long long>(hi) <= a.total_rows)) return r;
    if (!(olo >= 0 && olo <= static_cast<long long>(g) && static_cast<long long>(g) < ohi && static_cast<unsigned long long>(ohi) <= a.total_out_rows)) return r;
    const unsigned rows = static_cast<unsigned>(hi - lo);
    if (ohi - olo != static_cast<long long>((rows + a.stride - 1) / a.stride)) return r;
    r.src = a.x + static_cast<size_t>(lo) * a.cols;
    r.last = rows - 1;
    r.centre = static_cast<unsigned>(static_cast<long long>(g) - olo) * a.stride;  // < rows
    r.limit = a.width;
    return r;
}

// The 4 x 4 transpose of four registers across the four DPP rows of a wave (lane l = 16 * row + j): afterwards register i of row
// q holds what register q of row i held.  Two half exchanges per pair: v_permlane32_swap trades lanes 32 .. 63 of its first operand
// for lanes 0 .. 31 of its second (bit 1 of the row), v_permlane16_swap the odd rows of its first for the even rows of its second
// (bit 0).
__device__ __forceinline__ void transpose_rows(f32x4 &v)
{
    typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
    unsigned r[4] = {__float_as_uint(v[0]), __float_as_uint(v[1]), __float_as_uint(v[2]), __float_as_uint(v[3])};
    u32x2 p = __builtin_amdgcn_permlane32_swap(r[0], r[2], false, false);
    r[0] = p[0], r[2] = p[1];
    p = __builtin_amdgcn_permlane32_swap(r[1], r[3], false, false);
    r[1] = p[0], r[3] = p[1];
    p = __builtin_amdgcn_permlane16_swap(r[0], r[1], false, false);
    r[0] = p[0], r[1] = p[1];
    p = __builtin_amdgcn_permlane16_swap(r[2], r[3], false, false);
    r[2] = p[0], r[3] = p[1];
    v = f32x4{__uint_as_float(r[0]), __uint_as_float(r[1]), __uint_as_float(r[2]), __uint_as_float(r[3])};
}

// NF feature tiles x kRowTiles row tiles per wave.  The k axis goes in groups of four k-steps (16 elements): the table holds a lane's
// four A values of a group side by side (one 16-byte load per feature tile and group), and B comes in one of two ways.
//   VEC (cols % 4 == 0 and vec 16-byte aligned): four consecutive elements of a spliced row lie in one input row, so lane (q, j)
//   loads elements 16 g + 4 q .. + 3 of row j as ONE 16-byte load -- a quarter of the loads, of the address arithmetic and of the
//   cache lookups -- and transpose_rows turns them into what the four steps want: element 16 g + 4 i + q in register i.  K is a
//   multiple of 4 here, so there is no pad element among the steps that run.
//   Otherwise four single loads per group, element 16 g + 4 i + q for step i, each with its own (context row, column).
template <unsigned NF, bool VEC>
__global__ __launch_bounds__(256) void ss_affine_splice_kernel(const AffineArgs a)
{
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const unsigned kq = lane >> 4, j = lane & 15u;   // the operands' k within a step; the B / D column (output row of a tile)
    const unsigned ft0 = blockIdx.y * NF;            // first feature tile of this workgroup (the table is padded to gridDim.y * NF)
    const unsigned tile_stride = a.groups * 256u;    // floats between two feature tiles of the table
    const float *wt = a.table + a.bias_len + static_cast<size_t>(ft0) * tile_stride + 4u * lane;
    const unsigned e0 = VEC ? 4u * kq : kq;          // the lane's first element
    const unsigned c0 = e0 / a.cols, col0 = e0 - c0 * a.cols;
    const unsigned last_group = (a.steps - 1) / 4u, tail_steps = a.steps - 4u * last_group;  // 1 .. 4 steps in the last group

    for (unsigned long long g0 = static_cast<unsigned long long>(blockIdx.x) * kGroupRows + wave * kWaveRows; g0 < a.total_out_rows;
         g0 += static_cast<unsigned long long>(gridDim.x) * kGroupRows) {  // uniform per wave
        AffineRow row[kRowTiles];
#pragma unroll
        for (unsigned t = 0; t < kRowTiles; ++t) row[t] = affine_row(a, g0 + t * 16u + j);

        f32x4 acc[kRowTiles][NF];
#pragma unroll
        for (unsigned f = 0; f < NF; ++f) {
            const f32x4 bias = *reinterpret_cast<const f32x4 *>(a.table + (ft0 + f) * 16u + 4u * kq);
#pragma unroll
            for (unsigned t = 0; t < kRowTiles; ++t) acc[t][f] = bias;
        }

        // the lane's next element of the spliced row: context row c, column col
        unsigned c = c0, col = col0;
        // One group's operands as they come from memory.  The loads are unconditional and every address is a float of the lane's
        // clip (col < cols, the row clamped): a branch around a load would make the count of loads in flight unknown to the
        // compiler, which then waits for all of them ahead of every group.  What a lane without a row (limit 0) or a pad element (c
        // >= W) has read is replaced by +0.0 where the products are issued -- not here, which would wait for the load at once.
        struct Operands {
            f32x4 a[NF], b[kRowTiles];
            bool live[kRowTiles][VEC ? 1 : 4];
        };
        auto row_of = [&](const AffineRow &r) {  // the clip's row under (the lane's output row, c)
            const unsigned u = r.centre + c;                                // + left: the unclamped row
            return min((u > a.left ? u : a.left) - a.left, r.last);         // clamped to the clip
        };
        auto walk = [&]() {  // on by 16 (VEC) / 4 elements
            col += a.step_col;
            c += a.step_c;
            if (col >= a.cols) {
                col -= a.cols;
                ++c;
            }
        };
        auto fetch = [&](unsigned g, Operands &o) {  // group g; the walk moves on to g + 1
#pragma unroll
            for (unsigned f = 0; f < NF; ++f) o.a[f] = *reinterpret_cast<const f32x4 *>(wt + static_cast<size_t>(f) * tile_stride + g * 256u);
            if (VEC) {
#pragma unroll
                for (unsigned t = 0; t < kRowTiles; ++t) {
                    o.b[t] = *reinterpret_cast<const f32x4 *>(row[t].src + static_cast<size_t>(row_of(row[t])) * a.cols + col);
                    o.live[t][0] = row[t].limit != 0;
                }
                walk();
            } else {
#pragma unroll
                for (unsigned i = 0; i < 4; ++i) {
#pragma unroll
                    for (unsigned t = 0; t < kRowTiles; ++t) {
                        o.b[t][i] = row[t].src[static_cast<size_t>(row_of(row[t])) * a.cols + col];
                        o.live[t][i] = c < row[t].limit;
                    }
                    walk();
                }
            }
        };
        // the B registers of a group, one per step
        auto ready = [&](Operands &o) {
#pragma unroll
            for (unsigned t = 0; t < kRowTiles; ++t) {
#pragma unroll
                for (unsigned i = 0; i < 4; ++i) o.b[t][i] = o.live[t][VEC ? 0 : i] ? o.b[t][i] : 0.0f;
                if (VEC) transpose_rows(o.b[t]);
            }
        };
        auto step = [&](const Operands &o, unsigned i) {
#pragma unroll
            for (unsigned t = 0; t < kRowTiles; ++t)
#pragma unroll
                for (unsigned f = 0; f < NF; ++f) acc[t][f] = __builtin_amdgcn_mfma_f32_16x16x4f32(o.a[f][i], o.b[t][i], acc[t][f], 0, 0, 0);
        };
        auto products = [&](Operands &o) {
            ready(o);
#pragma unroll
            for (unsigned i = 0; i < 4; ++i) step(o, i);
        };
        auto tail = [&](Operands &o) {  // the last group: exactly the steps that are left -- one more on zeros would turn a -0.0
            ready(o);                   // result into +0.0
            step(o, 0);
            if (tail_steps > 1) step(o, 1);
            if (tail_steps > 2) step(o, 2);
            if (tail_steps > 3) step(o, 3);
        };
        // Two operand sets take turns, so a group's loads are in flight under the products of the group before it and no register
        // is copied; the loop body has no branch (one around a fetch would again hide the count of loads in flight).
        Operands o0, o1;
        fetch(0, o0);
        unsigned g = 0;
        for (; g + 2 <= last_group; g += 2) {  // uniform: groups g and g + 1 are whole, g + 2 exists
            fetch(g + 1, o1);
            __builtin_amdgcn_sched_barrier(0);  // (left alone, the scheduler sinks the loads to just ahead of their use)
            products(o0);
            __builtin_amdgcn_sched_barrier(0);
            fetch(g + 2, o0);
            __builtin_amdgcn_sched_barrier(0);
            products(o1);
            __builtin_amdgcn_sched_barrier(0);
        }
        if (g < last_group) {  // one or two groups are left, the first of them in o0
            fetch(g + 1, o1);
            products(o0);
            tail(o1);
        } else {
            tail(o0);
        }

#pragma unroll
        for (unsigned t = 0; t < kRowTiles; ++t) {
            if (!row[t].limit) continue;
            float *o = a.out + static_cast<size_t>(g0 + t * 16u + j) * a.out_dim;
#pragma unroll
            for (unsigned f = 0; f < NF; ++f) {
                const unsigned i0 = (ft0 + f) * 16u + 4u * kq;  // the lane's four features
                if (a.store16) {
                    if (i0 < a.out_dim) *reinterpret_cast<f32x4 *>(o + i0) = acc[t][f];  // out_dim % 4 == 0: all four or none
                } else {
#pragma unroll
                    for (unsigned r = 0; r < 4; ++r)
                        if (i0 + r < a.out_dim) o[i0 + r] = acc[t][f][r];
                }
            }
        }
    }
}

// feature tiles of 16, the groups of at most four that share a wave, and the tiles per group (level: 5 tiles are 3 + 3, not 4 + 4)
struct AffineTiling {
    unsigned groups, per_group;
};
AffineTiling affine_tiling(size_t out_dim)
{
    const unsigned tiles = static_cast<unsigned>((out_dim + 15) / 16), groups = (tiles + 3) / 4;
    return AffineTiling{groups, (tiles + groups - 1) / groups};
}

}  // namespace

hipError_t launch_affine_splice(const AffineArgs &a, hipStream_t stream)
{
    const AffineTiling tl = affine_tiling(a.out_dim);
    const unsigned long long passes = (a.total_out_rows + kGroupRows - 1) / kGroupRows;
    const dim3 grid(static_cast<unsigned>(std::min<unsigned long long>(passes, kMaxGroups)), tl.groups), block(256);
    switch (tl.per_group * 2 + (a.vec4 ? 1 : 0)) {
    case 2: hipLaunchKernelGGL((ss_affine_splice_kernel<1, false>), grid, block, 0, stream, a); break;
    case 3: hipLaunchKernelGGL((ss_affine_splice_kernel<1, true>), grid, block, 0, stream, a); break;
    case 4: hipLaunchKernelGGL((ss_affine_splice_kernel<2, false>), grid, block, 0, stream, a); break;
    case 5: hipLaunchKernelGGL((ss_affine_splice_kernel<2, true>), grid, block, 0, stream, a); break;
    case 6: hipLaunchKernelGGL((ss_affine_splice_kernel<3, false>), grid, block, 0, stream, a); break;
    case 7: hipLaunchKernelGGL((ss_affine_splice_kernel<3, true>), grid, block, 0, stream, a); break;
    case 8: hipLaunchKernelGGL((ss_affine_splice_kernel<4, false>), grid, block, 0, stream, a); break;
    default: hipLaunchKernelGGL((ss_affine_splice_kernel<4, true>), grid, block, 0, stream, a); break;
    }
    return hipGetLastError();
}

}  // namespace ss

// The handle: the matrix in the kernel's operand order behind the padded bias, and its device copy (made by the first device
// call, on the device that is current then).
struct ss_affine {
    size_t out_dim = 0, in_dim = 0;
    unsigned steps = 0;            // K4 / 4
    unsigned groups = 0;           // ceil(steps / 4): the k-steps go in groups of four
    unsigned bias_len = 0;         // 16 * feature tiles of the table
    std::vector<float> table;      // bias [bias_len] (zeros without one and past out_dim), then [feature tile][group][lane][step of the group]
    std::mutex mu;
    float *d_table = nullptr;
    int device = -1;
};

namespace ss {

namespace {

int check_dims(size_t out_dim, size_t in_dim)
{
    if (out_dim < 1 || out_dim > kMaxOutDim) return fail(SS_ERR_UNSUPPORTED, "out_dim must be 1 .. 256");
    if (in_dim < 1 || in_dim > kMaxInDim) return fail(SS_ERR_UNSUPPORTED, "in_dim must be 1 .. 4096");
    return SS_OK;
}

int device_table(const ss_affine *t_c, const float **d_table)
{
    ss_affine *t = const_cast<ss_affine *>(t_c);  // the lazy upload is the handle's one mutable part
    std::lock_guard<std::mutex> lock(t->mu);
    int dev = -1;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return no_device();
    if (!t->d_table) {
        void *p = nullptr;
        e = hipMalloc(&p, t->table.size() * sizeof(float));
        if (e == hipSuccess) e = hipMemcpy(p, t->table.data(), t->table.size() * sizeof(float), hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            if (p) (void)hipFree(p);
            return hip_fail(e, "affine table upload");
        }
        t->d_table = static_cast<float *>(p);
        t->device = dev;
    } else if (dev != t->device) {
        return fail(SS_ERR_ARG, "the transform's table lives on device " + std::to_string(t->device) + ", the current device is " + std::to_string(dev));
    }
    *d_table = t->d_table;
    return SS_OK;
}

// What both forms reject before the device is touched, the tables apart: the rules and the messages of ss_splice_packed*, then the
// transform's own.  (The splice's checks live in ss_splice.hip's unnamed namespace beside its kernels' argument structure.)
int check_scalars(const ss_affine *t, size_t n_clips, size_t total_rows, size_t total_out_rows, size_t cols, size_t left, size_t right, size_t stride)
{
    if (cols == 0) return fail(SS_ERR_ARG, "empty feature matrix (cols == 0)");
    if (left > kMaxContext || right > kMaxContext) return fail(SS_ERR_ARG, "left and right must be at most 32");
    if (stride < 1 || stride > kMaxContext) return fail(SS_ERR_ARG, "stride must be 1 .. 32");
    const size_t width = left + 1 + right;
    if (cols >= kCountLimit || width * cols >= kCountLimit) return fail(SS_ERR_ARG, "row too wide: (left + 1 + right) * cols must be below 2^31");
    if (n_clips >= kCountLimit || total_rows >= kCountLimit || total_out_rows >= kCountLimit) return fail(SS_ERR_ARG, "feature block too large");
    if (width * cols != t->in_dim)
        return fail(SS_ERR_ARG, "the transform takes " + std::to_string(t->in_dim) + " inputs, a spliced row has (left + 1 + right) * cols = " +
                                    std::to_string(width * cols));
    return SS_OK;
}

int check_not_in_place(const ss_affine *t, const float *vec, size_t total_rows, size_t cols, const float *out, size_t total_out_rows)
{
    if (ranges_overlap(vec, total_rows * cols * sizeof(float), out, total_out_rows * t->out_dim * sizeof(float)))
        return fail(SS_ERR_ARG, "out overlaps vec: the call is not in place");
    return SS_OK;
}

}  // namespace

}  // namespace ss

extern "C" {

int ss_affine_chain_len(size_t in_dim, size_t *k4)
{
    if (!k4) return ss::fail(SS_ERR_ARG, "null output");
    if (in_dim < 1 || in_dim > ss::kMaxInDim) return ss::fail(SS_ERR_UNSUPPORTED, "in_dim must be 1 .. 4096");
    *k4 = (in_dim + 3) / 4 * 4;
    return SS_OK;
}

int ss_affine_create(const float *matrix, size_t out_dim, size_t in_dim, size_t ld, const float *bias_or_null, ss_affine **out)
{
    if (!out) return ss::fail(SS_ERR_ARG, "null output");
    *out = nullptr;
    const int rc = ss::check_dims(out_dim, in_dim);
    if (rc) return rc;
    if (!matrix) return ss::fail(SS_ERR_ARG, "null buffer");
    if (ld < in_dim) return ss::fail(SS_ERR_ARG, "ld must be at least in_dim");
    const ss::AffineTiling tl = ss::affine_tiling(out_dim);
    ss_affine *t = new ss_affine;
    t->out_dim = out_dim;
    t->in_dim = in_dim;
    t->steps = static_cast<unsigned>((in_dim + 3) / 4);
    const unsigned tiles = tl.groups * tl.per_group;  // the last group's spare tiles are zero weights
    t->bias_len = 16 * tiles;
    t->groups = (t->steps + 3) / 4;
    t->table.assign(t->bias_len + static_cast<size_t>(tiles) * t->groups * 256, 0.0f);
    if (bias_or_null) std::memcpy(t->table.data(), bias_or_null, out_dim * sizeof(float));
    float *w = t->table.data() + t->bias_len;
    for (size_t i = 0; i < out_dim; ++i)
        for (size_t k = 0; k < in_dim; ++k)  // A[i & 15][k & 3] of step k / 4 sits in lane 16 * (k & 3) + (i & 15), the group's steps side by side
            w[(((i / 16) * t->groups + k / 16) * 64 + 16 * (k % 4) + i % 16) * 4 + k / 4 % 4] = matrix[i * ld + k];
    *out = t;
    return SS_OK;
}

void ss_affine_destroy(ss_affine *t)
{
    if (!t) return;
    if (t->d_table) (void)hipFree(t->d_table);
    delete t;
}

int ss_affine_dims(const ss_affine *t, size_t *out_dim, size_t *in_dim)
{
    if (!t || !out_dim || !in_dim) return ss::fail(SS_ERR_ARG, "null argument");
    *out_dim = t->out_dim;
    *in_dim = t->in_dim;
    return SS_OK;
}

int ss_affine_splice_packed_device(const ss_affine *t, const float *d_vec, size_t n_clips, const int64_t *d_row_offsets, size_t total_rows,
                                   const int64_t *d_out_offsets, size_t total_out_rows, size_t cols, size_t left, size_t right, size_t stride,
                                   float *d_out, void *stream)
{
    if (n_clips == 0) return SS_OK;
    if (!t || !d_vec || !d_row_offsets || !d_out_offsets || !d_out) return ss::fail(SS_ERR_ARG, "null buffer");
    int rc = ss::check_scalars(t, n_clips, total_rows, total_out_rows, cols, left, right, stride);
    if (rc || (rc = ss::check_not_in_place(t, d_vec, total_rows, cols, d_out, total_out_rows))) return rc;
    if (total_rows == 0 || total_out_rows == 0) return SS_OK;  // no clip can own a row
    ss::AffineArgs a;
    if ((rc = ss::device_table(t, &a.table))) return rc;
    a.x = d_vec;
    a.ro = reinterpret_cast<const long long *>(d_row_offsets);
    a.oo = reinterpret_cast<const long long *>(d_out_offsets);
    a.out = d_out;
    a.total_rows = total_rows;
    a.total_out_rows = total_out_rows;
    a.n_clips = static_cast<unsigned>(n_clips);
    a.cols = static_cast<unsigned>(cols);
    a.left = static_cast<unsigned>(left);
    a.stride = static_cast<unsigned>(stride);
    a.width = static_cast<unsigned>(left + 1 + right);
    a.vec4 = cols % 4 == 0 && reinterpret_cast<uintptr_t>(d_vec) % 16 == 0;
    const unsigned advance = a.vec4 ? 16u : 4u;
    a.step_c = advance / a.cols;
    a.step_col = advance % a.cols;
    a.steps = t->steps;
    a.groups = t->groups;
    a.bias_len = t->bias_len;
    a.out_dim = static_cast<unsigned>(t->out_dim);
    a.store16 = t->out_dim % 4 == 0 && reinterpret_cast<uintptr_t>(d_out) % 16 == 0;
    const hipError_t e = ss::launch_affine_splice(a, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return ss::hip_fail(e, "ss_affine_splice_kernel");
    ss::note_kernel("ss_affine_splice_kernel");
    return SS_OK;
}

// host-pointer form (synchronous): the table is checked on the host before the device is touched and the output table formed from
// it; the block and both tables go up, the rows the table covers come down (a host table is gap-free)
int ss_affine_splice_packed(const ss_affine *t, const float *vec, size_t n_clips, const int64_t *row_offsets, size_t total_rows, size_t cols, size_t left,
                            size_t right, size_t stride, float *out)
{
    if (n_clips == 0) return SS_OK;
    if (!t || !vec || !row_offsets || !out) return ss::fail(SS_ERR_ARG, "null buffer");
    int rc = ss::check_scalars(t, n_clips, total_rows, 0, cols, left, right, stride);
    if (rc || (rc = ss::check_clip_table(row_offsets, n_clips, total_rows))) return rc;
    std::vector<int64_t> oo(n_clips + 1);
    if ((rc = ss_splice_packed_offsets(n_clips, row_offsets, stride, oo.data()))) return rc;
    const size_t out_rows = static_cast<size_t>(oo[n_clips]);  // at most total_rows
    if ((rc = ss::check_not_in_place(t, vec, total_rows, cols, out, out_rows))) return rc;
    if (out_rows == 0) return SS_OK;
    if (!ss::have_device()) return ss::no_device();
    const size_t bytes = total_rows * cols * sizeof(float), obytes = out_rows * t->out_dim * sizeof(float), tbytes = (n_clips + 1) * sizeof(int64_t);
    ss::HostStage st("ss_affine_splice_packed");
    const float *d_in = st.up(vec, bytes);
    float *d_out = st.room<float>(obytes);
    const int64_t *d_ro = st.up(row_offsets, tbytes), *d_oo = st.up(oo.data(), tbytes);
    if (st.ok()) st.ran(ss_affine_splice_packed_device(t, d_in, n_clips, d_ro, total_rows, d_oo, out_rows, cols, left, right, stride, d_out, nullptr));
    st.sync();
    st.down(out, d_out, obytes);
    return st.status();
}

}  // extern "C"
