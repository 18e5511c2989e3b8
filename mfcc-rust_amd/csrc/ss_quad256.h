// The 256-point quad skeleton of the side kernels ss_mfcc_c256w, ss_kaldi_c256, ss_mel_c256 and ss_mfcc_c256x2 (gfx950, wave64).
// 16 lanes (one DPP row) own one 256-point complex transform, 16 points per lane; a wave carries four of them, each with a
// wave-private slot of 576 floats.  One iteration of a kernel's persistent loop is
//     claim_next | the kernel's own conditioning of v | pass1 | the kernel's prefetch of the next unit | pass2 |
//     fetch_partners + untangle per register | the kernel's own epilogue over the P row (mel_raw_sums, DCT, stores)
// around which sit stage_tables (the table block, once per workgroup) and locate_frame (flat frame index -> clip and frame).
// ss_mfcc512.hip, the benchmark kernel, does not use this header: its exchange and untangle have diverged on purpose.
//
// The top part (locate_frame, plan_groups) is plain C++: tools/hosttest/test_launch_plan.cpp builds it with a host compiler.
#pragma once

#include <cstddef>
#include <cstdint>
#include "ss_launch_plan.h"
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define SS_Q256_HD __host__ __device__ __forceinline__
#else
#define SS_Q256_HD inline
#endif

namespace ss {
namespace q256 {

constexpr int kSlotFloats = 576;  // per transform: the exchange slot (288 float2); afterwards the kernel's P and ln(mel) rows
constexpr int kWaveFloats = 4 * kSlotFloats;

// (clip, t) of flat frame first + fl, first = the group's first frame (uniform), fl < group its lane's frame within the group.
// magic != 0: scalar quotient of `first` by multiply-high (frame_reciprocal), then ONE conditional wrap per lane -- exact for
// n_frames >= group and first + group < 2^31, which plan_groups guarantees.  magic == 0: the lane divides.
SS_Q256_HD void locate_frame(uint32_t first, uint32_t fl, uint32_t n_frames, uint32_t magic, uint32_t shift, uint32_t &clip, uint32_t &t)
{
    if (magic) {
#if defined(__HIP_DEVICE_COMPILE__)
        clip = __umulhi(first, magic) >> shift;
#else
        clip = static_cast<uint32_t>((static_cast<uint64_t>(first) * magic) >> 32) >> shift;
#endif
        t = first - clip * n_frames + fl;
        const bool wrap = t >= n_frames;
        t -= wrap ? n_frames : 0u;
        clip += wrap ? 1u : 0u;
    } else {
        const uint32_t gf = first + fl;
        clip = gf / n_frames;
        t = gf - clip * n_frames;
    }
}

constexpr size_t kLdsLimit = 160 * 1024;

// What a launcher over groups of `group` frames (4: quads, 8: octs) hands its kernel: the reciprocal of n_frames where
// locate_frame's one-wrap fix-up holds (never for a packed launch, dense = false), and the CU-capped grid.
struct GroupPlan { uint32_t nf_magic, nf_shift; unsigned grid; };
enum class PlanStatus { Launch, Empty, Invalid };
inline PlanStatus plan_groups(unsigned long long total, uint32_t n_frames, unsigned group, bool dense, size_t lds, int waves, int num_cus,
                              GroupPlan &p)
{
    p = GroupPlan{0u, 0u, 0u};
    if (dense && n_frames >= group && n_frames < (1u << 31) && total + group < (1ull << 31)) {
        const FrameReciprocal r = frame_reciprocal(n_frames);
        p.nf_magic = r.magic;
        p.nf_shift = r.shift;
    }
    if (lds > kLdsLimit) return PlanStatus::Invalid;
    if (total == 0) return PlanStatus::Empty;
    if (total + 8 >= 0xffffffffull) return PlanStatus::Invalid;  // the kernels count frames in 32 bits
    p.grid = cu_capped_grid((total + group - 1) / group, waves, num_cus);
    return PlanStatus::Launch;
}

}  // namespace q256
}  // namespace ss

#if defined(__HIPCC__)
#include "ss_fft_reg.h"
#include "ss_wave.h"
namespace ss {
namespace q256 {
using namespace wv;

__device__ __forceinline__ int partner_addr(int lane, int j) { return ((lane & 48) | ((16 - j) & 15)) << 2; }  // lane holding Z[256 - k]
__device__ __forceinline__ int exchange_write_base(int j) { return 34 * (j >> 1) + (j & 1); }                  // float2 units

// (stage_tables and claim_next: ss_wave.h, shared with the frame stages of ss_frame32.h)

// first radix-16 pass and the transposing scatter into the slot; v is dead afterwards (the caller's prefetch goes here)
__device__ __forceinline__ void pass1(float2 (&v)[16], float2 *zh, int wbase1)
{
    fft16_reg(v);
#pragma unroll
    for (int r = 0; r < 16; ++r) zh[wbase1 + 2 * r] = v[r];
    wave_order();
}

// ds_read_b128 gather, pass-2 twiddles, second radix-16 pass: u[r] = Z[j + 16 r].  tw2: the LDS table, or (RES) the lane's
// eight entries kept in registers
template <bool RES = false>
__device__ __forceinline__ void pass2(float2 (&u)[16], const float2 *zh, int j, const float4 *tw2)
{
#pragma unroll
    for (int p = 0; p < 8; ++p) {
        const float4 t4 = *reinterpret_cast<const float4 *>(&zh[34 * p + 2 * j]);
        u[2 * p] = make_float2(t4.x, t4.y);
        u[2 * p + 1] = make_float2(t4.z, t4.w);
    }
    wave_order();
#pragma unroll
    for (int p = 0; p < 8; ++p) {
        const float4 w2 = tw2[RES ? p : p * 16 + j];
        u[2 * p + 1] = cmul(u[2 * p + 1], make_float2(w2.x, w2.y));
        if (p < 7) u[2 * p + 2] = cmul(u[2 * p + 2], make_float2(w2.z, w2.w));
    }
    fft16_reg(u);
}

// zcs[r] = Z[256 - (j + 16 r)] of the lanes j != 0: register 15 - r of lane 16 - j, by ds_bpermute_b32
__device__ __forceinline__ void fetch_partners(const float2 (&u)[16], int paddr, float2 (&zcs)[8])
{
#pragma unroll
    for (int r = 0; r < 8; ++r) zcs[r] = make_float2(bperm(paddr, u[15 - r].x), bperm(paddr, u[15 - r].y));
}
// lane 0 pairs with itself: Z[256 - 16 r] = own register (16 - r) & 15
__device__ __forceinline__ float2 partner(const float2 (&u)[16], const float2 (&zcs)[8], int j, int r) { return j == 0 ? u[(16 - r) & 15] : zcs[r]; }

// Real-FFT untangle (untangle_bin, ss_wave.h) of k = j + 16 r with w = exp(-2 pi i k / 512): 2 X[k] = (xr, xi), s = 2 E[k].  The
// mirrored bin is the caller's: 2 conj X[256-k] = 2 s - 2 X[k].
__device__ __forceinline__ Bin untangle(const float2 (&u)[16], const float2 (&zcs)[8], float2 w, int j, int r)
{
    return untangle_bin(u[r], partner(u, zcs, j, r), w);
}

// raw banded-mel sums of a lane's N slots over the P row: slot k starts at bin st[k] and takes q4[k] float4s of the lane's
// weight row, which holds the slots back to back.  Scale, zero handling and log stay with the kernel.
template <int N>
__device__ __forceinline__ void mel_raw_sums(const float4 *w4, const float *prow, const int (&st)[N], const int32_t *q4, float (&m)[N])
{
    int off = 0;
#pragma unroll
    for (int k = 0; k < N; ++k) {
        m[k] = mel_slot1(w4 + off, prow + st[k], q4[k]);
        off += q4[k];
    }
}

}  // namespace q256
}  // namespace ss
#endif
