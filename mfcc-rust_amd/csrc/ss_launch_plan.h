// The launch arithmetic the fused kernels' launchers share: the CU-capped grid of a persistent kernel, the balanced split of its
// work units over the workgroups, the multiply-high reciprocal of n_frames and the 32-bit address-range test of the 512-point
// kernel's quad_src.  Plain C++ (no HIP header): tools/hosttest/test_launch_plan.cpp builds it alone with a host compiler.
#pragma once

#include <cstddef>
#include <cstdint>

namespace ss {

// workgroups a persistent kernel may occupy: one per CU (256 where the caller knows no count)
inline unsigned cu_cap(int num_cus)
{
    return static_cast<unsigned>(num_cus > 0 ? num_cus : 256);
}

// one persistent workgroup of `waves` waves per CU; fewer when there is not a work unit per wave (0 for no units)
inline unsigned cu_capped_grid(unsigned long long units, int waves, int num_cus)
{
    const unsigned long long cap = cu_cap(num_cus), blocks = (units + waves - 1) / waves;
    return static_cast<unsigned>(blocks < cap ? blocks : cap);
}

// workgroup b owns units [b * q_base + min(b, q_rem), + q_base + (b < q_rem)): the balanced contiguous split, without a division
// in the kernel's prologue.  units < 2^32, grid >= 1
struct UnitSplit {
    uint32_t q_base, q_rem;
};
inline UnitSplit split_units(unsigned long long units, unsigned grid)
{
    return UnitSplit{static_cast<uint32_t>(units / grid), static_cast<uint32_t>(units % grid)};
}

// floor(x / d) for x < 2^31 as umulhi(x, magic) >> shift: magic = ceil(2^(31+l) / d), shift = l - 1, l = ceil(log2 d)
// (Granlund-Montgomery; magic < 2^32).  d >= 2.  The kernels' one-wrap lane fix-ups need more (d >= 4 or 8) and a bound on
// the largest x: those guards differ per kernel and stay with the launchers.
struct FrameReciprocal {
    uint32_t magic, shift;
};
inline FrameReciprocal frame_reciprocal(uint32_t d)
{
    unsigned l = 0;
    while ((1ull << l) < d) ++l;
    const unsigned long long num = 1ull << (31 + l);  // l <= 32
    return FrameReciprocal{static_cast<uint32_t>((num + d - 1) / d), l - 1};
}

// quad_src of the 512-point kernel (the SPREAD builds' sample addresses): a lane's 32-bit byte offset from the quad's uniform base
// reaches 3 frames + one step into the next clip + its 16 sample pairs + the sixteen 128-byte strides of the loads, and the
// frame-in-quad product is a 24-bit multiply.  False: the clip rows overlap (ld < n_frames * step) or a row stride / hop goes
// beyond that, and the kernel's 32-bit offsets could wrap.
inline bool quad_src_in_range(uint32_t n_frames, uint32_t step, unsigned long long ld)
{
    const unsigned long long span = static_cast<unsigned long long>(n_frames) * step;
    return ld >= span && static_cast<unsigned long long>(step) * 4ull < (1ull << 24) &&
           3ull * step * 4ull + (ld - span) * 4ull + 16ull * 8ull + 16ull * 128ull < (1ull << 32);
}

}  // namespace ss
