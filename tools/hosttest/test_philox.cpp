// The known answers of Philox4x32-10 through mfcc-rust_amd/csrc/ss_philox.h itself (plain C++: the header needs no HIP), for the
// counters no ss_specaug_* call can form (a mask index of ffffffff or 85a308d3).  Host only, no GPU:
//   g++ -O1 -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -Imfcc-rust_amd/csrc tools/hosttest/test_philox.cpp -o /tmp/ph && /tmp/ph
// (tests/test_specaug_cpu.py does exactly that)
#include <cstdint>
#include <cstdio>

#include "ss_philox.h"

int main()
{
    struct Case {
        uint32_t ctr[4], key[2], want[4];
    };
    const Case cases[] = {
        {{0u, 0u, 0u, 0u}, {0u, 0u}, {0x6627e8d5u, 0xe169c58du, 0xbc57ac4cu, 0x9b00dbd8u}},
        {{0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu}, {0xffffffffu, 0xffffffffu}, {0x408f276du, 0x41c83b0eu, 0xa20bc7c6u, 0x6d5451fdu}},
        {{0x243f6a88u, 0x85a308d3u, 0x13198a2eu, 0x03707344u}, {0xa4093822u, 0x299f31d0u}, {0xd16cfe09u, 0x94fdccebu, 0x5001e420u, 0x24126ea1u}},
    };
    int bad = 0;
    for (const Case &c : cases) {
        const ss::Philox4 r = ss::philox4x32_10(c.ctr[0], c.ctr[1], c.ctr[2], c.ctr[3], c.key[0], c.key[1]);
        for (int i = 0; i < 4; ++i) {
            if (r.w[i] != c.want[i]) {
                std::printf("counter %08x %08x %08x %08x word %d: got %08x, want %08x\n", c.ctr[0], c.ctr[1], c.ctr[2], c.ctr[3], i, r.w[i], c.want[i]);
                ++bad;
            }
        }
    }
    if (bad) return 1;
    std::printf("all checks passed\n");
    return 0;
}
