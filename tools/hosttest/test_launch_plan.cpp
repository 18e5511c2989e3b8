// Host-side check of the launch arithmetic in mfcc-rust_amd/csrc/ss_launch_plan.h (no GPU, no HIP header): the multiply-high
// reciprocal divides exactly, the CU-capped grid and the unit split keep their invariants, the quad_src address-range test flips
// at its three boundaries, the plans of the headline shapes are the pinned ones, and the quad kernels' shared frame locate and
// launch plan (the plain C++ part of ss_quad256.h) agree with plain division.  tests/test_launch_plan.py builds it with
// AddressSanitizer + UBSan and runs it:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -Imfcc-rust_amd/csrc
//       tools/hosttest/test_launch_plan.cpp -o /tmp/lp && /tmp/lp
#include "ss_launch_plan.h"
#include "ss_quad256.h"

#include <cstdio>
#include <initializer_list>

static int g_failed = 0;
#define CHECK(cond, ...)                                  \
    do {                                                  \
        if (!(cond)) {                                    \
            if (++g_failed <= 20) {                       \
                std::printf("FAILED %s: ", #cond);        \
                std::printf(__VA_ARGS__);                 \
                std::printf("\n");                        \
            }                                             \
        }                                                 \
    } while (0)

static uint64_t g_state = 0x9e3779b97f4a7c15ull;
static uint64_t rnd()  // splitmix64
{
    uint64_t z = (g_state += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

constexpr uint64_t kTwo31 = 1ull << 31;

// what the kernels compute: umulhi(x, magic) >> shift
static uint32_t div_by(uint32_t x, ss::FrameReciprocal r)
{
    return static_cast<uint32_t>((static_cast<uint64_t>(x) * r.magic) >> 32) >> r.shift;
}

static void check_reciprocal(uint32_t d)
{
    const ss::FrameReciprocal r = ss::frame_reciprocal(d);
    // the untruncated ceil(2^(31+l) / d), l = shift + 1, is the 32-bit magic
    const unsigned __int128 num = static_cast<unsigned __int128>(1) << (32 + r.shift);
    const unsigned __int128 full = (num + d - 1) / d;
    CHECK(r.shift < 31 && full <= 0xffffffffull && static_cast<uint32_t>(full) == r.magic, "d %u: magic %u shift %u", d, r.magic, r.shift);
    CHECK((1ull << r.shift) < d && d <= (2ull << r.shift), "d %u: shift %u is not ceil(log2 d) - 1", d, r.shift);
    const uint64_t top = (kTwo31 - 1) / d * d;  // the multiple of d nearest 2^31 from below
    const uint64_t xs[] = {0, 1, d - 1ull, d, d + 1ull, kTwo31 - 1, top, top - 1, top >= d ? top - d : 0, top >= d ? top - d + 1 : 0,
                           top + d - 1, rnd() % kTwo31, rnd() % kTwo31, rnd() % kTwo31, rnd() % kTwo31};
    for (uint64_t x : xs) {
        if (x >= kTwo31) continue;  // (d + 1 or top + d - 1 beyond the range the kernels divide in)
        const uint32_t x32 = static_cast<uint32_t>(x);
        CHECK(div_by(x32, r) == x32 / d, "x %u / d %u: %u, want %u", x32, d, div_by(x32, r), x32 / d);
    }
}

static void check_grid_and_split()
{
    const int cus[] = {-1, 0, 1, 8, 255, 256, 304}, waves[] = {8, 9, 12, 16};
    CHECK(ss::cu_cap(0) == 256 && ss::cu_cap(-3) == 256 && ss::cu_cap(1) == 1 && ss::cu_cap(304) == 304, "cu_cap");
    for (int it = 0; it < 20000; ++it) {
        const int nc = cus[rnd() % 7], w = waves[rnd() % 4];
        const unsigned cap = nc > 0 ? static_cast<unsigned>(nc) : 256u;
        // small counts, counts around cap * waves, counts up to 2^32 - 2
        const uint64_t pick = rnd() % 3, units = pick == 0 ? 1 + rnd() % 64 : pick == 1 ? 1 + rnd() % (2ull * cap * w) : 1 + rnd() % 0xfffffffeull;
        const unsigned grid = ss::cu_capped_grid(units, w, nc);
        const uint64_t blocks = (units + w - 1) / w;
        CHECK(grid >= 1 && grid <= cap, "units %llu waves %d cus %d: grid %u", (unsigned long long)units, w, nc, grid);
        CHECK(grid == (blocks < cap ? blocks : cap), "units %llu waves %d cus %d: grid %u", (unsigned long long)units, w, nc, grid);
        const ss::UnitSplit s = ss::split_units(units, grid);
        CHECK(static_cast<uint64_t>(s.q_base) * grid + s.q_rem == units && s.q_rem < grid, "units %llu grid %u: %u, %u", (unsigned long long)units,
              grid, s.q_base, s.q_rem);
    }
    CHECK(ss::cu_capped_grid(0, 12, 256) == 0, "no units, no workgroup: the launchers that want one for an empty block say so");
}

// The launchers reject a launch where this expression of the parent launcher is true (launch_w / launch_mfcc_c256_multi):
//   ld < span || step * 4 >= 2^24 || 3 * step * 4 + (ld - span) * 4 + 16 * 8 + 16 * 128 >= 2^32,   span = n_frames * step
// i.e. quad_src_in_range is its negation.
static void check_quad_src_range()
{
    // ld == span: 99 frames at hop 160, span = 15840
    CHECK(ss::quad_src_in_range(99, 160, 15840), "ld == span");
    CHECK(!ss::quad_src_in_range(99, 160, 15839), "ld == span - 1");
    // 4 * step == 2^24: step = 4194304; 4 frames, ld = span (sum = 12 * step + 2176, far below 2^32)
    CHECK(ss::quad_src_in_range(4, 4194303, 16777212), "4 * step == 2^24 - 4");
    CHECK(!ss::quad_src_in_range(4, 4194304, 16777216), "4 * step == 2^24");
    // the sum: 12 * 160 + 4 * (ld - 15840) + 2176 >= 2^32  <=>  ld - 15840 >= (2^32 - 4096) / 4 = 1073740800
    CHECK(ss::quad_src_in_range(99, 160, 1073756639ull), "sum == 2^32 - 4");
    CHECK(!ss::quad_src_in_range(99, 160, 1073756640ull), "sum == 2^32");
    // the headline layout: clips of 16000 samples, 99 frames
    CHECK(ss::quad_src_in_range(99, 160, 16000), "headline shape");
}

// The plan of a 512-point launch as the parent launcher wrote it out (12 waves, quads of 4 frames):
//   quads = (total + 3) / 4, blocks = (quads + 11) / 12, grid = min(blocks, num_cus > 0 ? num_cus : 256),
//   q_base = quads / grid, q_rem = quads % grid;
//   l = ceil(log2 n_frames), nf_magic = ceil(2^(31+l) / n_frames), nf_shift = l - 1
struct Pinned {
    uint32_t n_frames, clips;  // total = clips * n_frames
    unsigned grid;
    uint32_t q_base, q_rem, nf_magic, nf_shift;
};
static void check_pinned()
{
    const Pinned pins[] = {
        // one clip of `total` frames (the 320 / 160 shape: n_frames = (n_samples - 320) / 160 + 1)
        // total 3: 1 quad, 1 block; l = 2, ceil(2^33 / 3) = ceil(8589934592 / 3) = 2863311531 (launch_w itself takes magic = 0 below 4)
        {3, 1, 1, 1, 0, 2863311531u, 1},
        // total 4: 1 quad, 1 block; l = 2, 2^33 / 4 = 2^31
        {4, 1, 1, 1, 0, 2147483648u, 1},
        // total 255: 64 quads, ceil(64 / 12) = 6 blocks, 64 = 6 * 10 + 4; l = 8, 2^39 = 255 * 2155905152 + 128 -> 2155905153
        {255, 1, 6, 10, 4, 2155905153u, 7},
        // total 256 * 12 * 4 = 12288: 3072 quads, 256 blocks of 12; l = 14, 2^45 / (3 * 2^12) = 2^33 / 3 -> 2863311531
        {12288, 1, 256, 12, 0, 2863311531u, 13},
        // total 12289: 3073 quads, 257 blocks capped to 256, 3073 = 256 * 12 + 1; l = 14, 2^45 = 12289 * 2863078532 + 9084 -> 2863078533
        {12289, 1, 256, 12, 1, 2863078533u, 13},
        // the benchmark's cfg2: 1024 clips of 1 s at 16 kHz, 99 frames each: 101376 frames, 25344 quads, 2112 blocks capped to 256,
        // 25344 = 256 * 99; l = 7, 2^38 = 99 * 2776544514 + 58 -> 2776544515
        {99, 1024, 256, 99, 0, 2776544515u, 6},
    };
    for (const Pinned &p : pins)
        for (int num_cus : {256, 0}) {  // (no CU count known: 256)
            const uint64_t total = static_cast<uint64_t>(p.clips) * p.n_frames, quads = (total + 3) / 4;
            const unsigned grid = ss::cu_capped_grid(quads, 12, num_cus);
            const ss::UnitSplit s = ss::split_units(quads, grid);
            const ss::FrameReciprocal r = ss::frame_reciprocal(p.n_frames);
            CHECK(grid == p.grid && s.q_base == p.q_base && s.q_rem == p.q_rem && r.magic == p.nf_magic && r.shift == p.nf_shift,
                  "n_frames %u x %u clips, num_cus %d: grid %u q_base %u q_rem %u magic %u shift %u", p.n_frames, p.clips, num_cus, grid, s.q_base,
                  s.q_rem, r.magic, r.shift);
        }
    // total 1 (one frame: no reciprocal, launch_w's guard is n_frames >= 4): 1 quad, 1 block
    for (int num_cus : {256, 0}) {
        const unsigned grid = ss::cu_capped_grid(1, 12, num_cus);
        const ss::UnitSplit s = ss::split_units(1, grid);
        CHECK(grid == 1 && s.q_base == 1 && s.q_rem == 0, "one frame, num_cus %d: grid %u q_base %u q_rem %u", num_cus, grid, s.q_base, s.q_rem);
    }
}

// locate_frame of ss_quad256.h, the frame locate the quad kernels share, against plain division: with the reciprocal exactly where
// plan_groups enables it (n_frames >= group, n_frames < 2^31, total + group < 2^31) and with the dividing fallback elsewhere.
// Group starts: the first groups, the last ones, and every group at or next to a clip boundary of the first and last clips.
static void check_locate(uint32_t n_frames, unsigned group)
{
    const uint64_t room = kTwo31 - group - 1;  // the largest total with a reciprocal
    const uint64_t batches[] = {1, 2, 3, 1000, room / n_frames, room / n_frames + 1};
    for (uint64_t batch : batches) {
        const uint64_t total = batch * n_frames;
        if (batch == 0 || total + 8 >= 0xffffffffull) continue;
        ss::q256::GroupPlan p;
        const ss::q256::PlanStatus st = ss::q256::plan_groups(total, n_frames, group, true, 1024, 12, 256, p);
        const bool want_magic = n_frames >= group && total + group < kTwo31;
        CHECK(st == ss::q256::PlanStatus::Launch && (p.nf_magic != 0) == want_magic && p.grid == ss::cu_capped_grid((total + group - 1) / group, 12, 256),
              "n_frames %u x %llu, group %u: status %d magic %u grid %u", n_frames, (unsigned long long)batch, group, static_cast<int>(st), p.nf_magic, p.grid);
        if (want_magic) {
            const ss::FrameReciprocal r = ss::frame_reciprocal(n_frames);
            CHECK(p.nf_magic == r.magic && p.nf_shift == r.shift, "n_frames %u: magic %u shift %u", n_frames, p.nf_magic, p.nf_shift);
        }
        ss::q256::GroupPlan packed;
        ss::q256::plan_groups(total, n_frames, group, false, 1024, 12, 256, packed);
        CHECK(packed.nf_magic == 0 && packed.grid == p.grid, "a packed launch takes no reciprocal");
        const uint64_t groups = (total + group - 1) / group;
        auto check_group = [&](uint64_t gi) {
            if (gi >= groups) return;
            const uint32_t first = static_cast<uint32_t>(gi * group);
            for (uint32_t fl = 0; fl < group && first + static_cast<uint64_t>(fl) < total; ++fl) {
                uint32_t clip = ~0u, t = ~0u;
                ss::q256::locate_frame(first, fl, n_frames, p.nf_magic, p.nf_shift, clip, t);
                const uint32_t g = first + fl;
                CHECK(clip == g / n_frames && t == g % n_frames, "frame %u of %u-frame clips (group %u, magic %u): clip %u t %u", g, n_frames, group,
                      p.nf_magic, clip, t);
            }
        };
        for (uint64_t gi = 0; gi < 40; ++gi) check_group(gi);
        for (uint64_t gi = groups > 40 ? groups - 40 : 0; gi < groups; ++gi) check_group(gi);
        const uint64_t clips[] = {1, 2, 3, batch / 2, batch - 2, batch - 1, batch};
        for (uint64_t c : clips) {
            if (c > batch) continue;
            const uint64_t at = c * n_frames / group;  // the group that holds (or ends at) the boundary, and its neighbours
            for (uint64_t gi = at >= 2 ? at - 2 : 0; gi <= at + 2; ++gi) check_group(gi);
        }
    }
}

static void check_plan_status()
{
    using namespace ss::q256;
    GroupPlan p;
    CHECK(plan_groups(400, 100, 4, true, kLdsLimit, 12, 256, p) == PlanStatus::Launch && p.grid == 9, "LDS at the limit");
    CHECK(plan_groups(400, 100, 4, true, kLdsLimit + 1, 12, 256, p) == PlanStatus::Invalid, "LDS beyond the limit");
    CHECK(plan_groups(0, 100, 4, true, kLdsLimit + 1, 12, 256, p) == PlanStatus::Invalid, "the LDS check comes before the empty launch");
    CHECK(plan_groups(0, 100, 4, true, 1024, 12, 256, p) == PlanStatus::Empty && p.grid == 0, "no frames");
    CHECK(plan_groups(0xffffffffull - 9, 1, 8, true, 1024, 12, 256, p) == PlanStatus::Launch && p.nf_magic == 0, "the largest total");
    CHECK(plan_groups(0xffffffffull - 8, 1, 8, true, 1024, 12, 256, p) == PlanStatus::Invalid, "total + 8 reaches 2^32 - 1");
    // the reciprocal's three conditions, each at its edge (group 4 and 8)
    for (unsigned group : {4u, 8u}) {
        CHECK(plan_groups(10ull * (group - 1), group - 1, group, true, 1024, 12, 256, p) == PlanStatus::Launch && p.nf_magic == 0, "n_frames < group");
        CHECK(plan_groups(10ull * group, group, group, true, 1024, 12, 256, p) == PlanStatus::Launch && p.nf_magic != 0, "n_frames == group");
        CHECK(plan_groups(kTwo31 - group - 1, static_cast<uint32_t>(kTwo31 - group - 1), group, true, 1024, 12, 256, p) == PlanStatus::Launch && p.nf_magic != 0,
              "total + group == 2^31 - 1");
        CHECK(plan_groups(kTwo31 - group, static_cast<uint32_t>(kTwo31 - group), group, true, 1024, 12, 256, p) == PlanStatus::Launch && p.nf_magic == 0,
              "total + group == 2^31");
    }
}

int main()
{
    for (unsigned group : {4u, 8u})
        for (uint32_t n : {1u, 3u, 4u, 5u, 7u, 8u, 9u, 98u, static_cast<uint32_t>(kTwo31 - 1)}) check_locate(n, group);
    check_plan_status();
    for (uint32_t d = 2; d <= 4096; ++d) check_reciprocal(d);
    for (int i = 0; i < 4000; ++i) check_reciprocal(2 + static_cast<uint32_t>(rnd() % (kTwo31 - 2)));
    for (int s = 2; s < 31; ++s)
        for (int o = -1; o <= 1; ++o) check_reciprocal((1u << s) + o);  // around the powers of two
    check_reciprocal(static_cast<uint32_t>(kTwo31 - 1));
    check_grid_and_split();
    check_quad_src_range();
    check_pinned();
    if (g_failed) {
        std::printf("%d checks failed\n", g_failed);
        return 1;
    }
    std::printf("all checks passed\n");
    return 0;
}
