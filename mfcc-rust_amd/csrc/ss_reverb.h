// What the host side (ss_host.cpp) and the kernels (ss_reverb.hip) share of the reverberation stage (ss_reverb_* of
// include/speechsauce_amd.h, whose comment is the definition): the sizes of the partitioned overlap-save scheme and the layout of
// the bank's device block.  Plain C++ (no HIP header): the host compiler builds it into ss_host.cpp.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

namespace ss {
namespace reverb {

constexpr unsigned kBlock = 512;                  // B: taps of a partition, outputs of one real window
constexpr unsigned kFft = 2 * kBlock;             // N: points of the transform, 32 x 32 on 32 lanes
constexpr unsigned kMaxTaps = 16384;              // K_c of a response
constexpr unsigned kMaxParts = kMaxTaps / kBlock;  // partitions of the longest response
constexpr unsigned kPartFloats = 2 * kFft;        // floats of one partition spectrum, and of the twiddle block

// Lane j (< 32) of a transform holds the points n = j + 32 e before it and the bins k = j + 32 q behind it.  A partition spectrum
// and the twiddle block lie as [16][32] float4: entry (t, j) = the complex values of index (2t, j) and (2t + 1, j), so that a lane
// fetches two of its values per 16-byte LDS read and the 32 lanes of a read cover 512 consecutive bytes (conflict-free, and the
// two halves of a wave read the same addresses).  Spectrum: H[j + 32 r] at r = 2t, 2t + 1.  Twiddles: exp(-2 pi i j r / 1024).
inline size_t part_slot(unsigned r, unsigned j) { return ((r >> 1) * 32u + j) * 4u + (r & 1u) * 2u; }

// one response of the bank as the kernels see it (16 bytes)
struct RirMeta {
    int32_t taps;   // K_c
    int32_t parts;  // ceil(K_c / B)
    int32_t shift;  // the handle's shift: peak_c with align_peak, else 0
    int32_t first;  // index of partition 0 among the bank's partition spectra
};

// the twiddle block of the 1024-point transform, kPartFloats floats
void build_twiddles(std::vector<float> &tw);
// The spectra of the partitions of taps[0 .. n): partition p = taps[pB .. pB + B) zero-padded to N points, transformed in f64
// (radix-2, exp(-2 pi i nk / N)) and rounded once to f32, appended to `out` in the lane layout above.
void append_partition_spectra(const float *taps, size_t n, std::vector<float> &out);
// peak = first index of max |h|; the normalised taps (mode 0: as given; 1: unit energy; 2: peak magnitude 1), sums and quotients in f64
size_t normalise_taps(const float *h, size_t n, int mode, std::vector<float> &out);

}  // namespace reverb
}  // namespace ss
