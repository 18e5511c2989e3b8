// Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11; the Random123 generator):
// a counter-based generator -- four output words are a pure function of a 4-word counter and a 2-word key, so a lane draws
// its numbers from what it already knows (which clip, which mask, which epoch) and no generator state lives on the device.
// Integer arithmetic only: host and device give the same words.  Known answers (counter | key | output), pinned by
// tests/test_specaug_cpu.py:
//   00000000 x4                          | 00000000 x2        | 6627e8d5 e169c58d bc57ac4c 9b00dbd8
//   ffffffff x4                          | ffffffff x2        | 408f276d 41c83b0e a20bc7c6 6d5451fd
//   243f6a88 85a308d3 13198a2e 03707344  | a4093822 299f31d0  | d16cfe09 94fdcceb 5001e420 24126ea1
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define SS_PHILOX_HD __host__ __device__
#else
#define SS_PHILOX_HD
#endif

namespace ss {

struct Philox4 {
    uint32_t w[4];
};

SS_PHILOX_HD inline Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1)
{
    constexpr uint64_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u;  // the multipliers
    constexpr uint32_t W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;  // the Weyl constants of the key schedule
    for (int round = 0; round < 10; ++round) {
        const uint64_t p0 = M0 * c0, p1 = M1 * c2;
        const uint32_t n0 = static_cast<uint32_t>(p1 >> 32) ^ c1 ^ k0, n2 = static_cast<uint32_t>(p0 >> 32) ^ c3 ^ k1;
        c1 = static_cast<uint32_t>(p1);
        c3 = static_cast<uint32_t>(p0);
        c0 = n0;
        c2 = n2;
        k0 += W0;
        k1 += W1;
    }
    return Philox4{{c0, c1, c2, c3}};
}

}  // namespace ss
