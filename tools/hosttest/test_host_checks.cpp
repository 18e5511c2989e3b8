// Host-side check of the table and pool rules in mfcc-rust_amd/csrc/ss_host_checks.h (no GPU, no HIP header): the slot rule, the
// clip-table and row-offset rules with their messages as exact strings (the first offending clip / entry is the one named),
// ranges_overlap at its boundaries, and the pool-row gather / scatter bit for bit.  ss::fail is supplied here: it records the
// message.  tests/test_host_checks.py builds it with AddressSanitizer + UBSan and runs it:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Imfcc-rust_amd/csrc
//       tools/hosttest/test_host_checks.cpp -o /tmp/hc && /tmp/hc
#include "ss_host_checks.h"

#include <climits>
#include <cstdio>

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

static std::string g_msg;
namespace ss {
int fail(int status, const std::string &msg)
{
    g_msg = msg;
    return status;
}
}  // namespace ss

// rc is SS_OK and nothing was reported, or rc is SS_ERR_ARG with exactly `want`
static void expect(int rc, const char *want, const char *what)
{
    if (!want) CHECK(rc == SS_OK && g_msg.empty(), "%s: rc %d, message \"%s\"", what, rc, g_msg.c_str());
    else CHECK(rc == SS_ERR_ARG && g_msg == want, "%s: rc %d, message \"%s\", want \"%s\"", what, rc, g_msg.c_str(), want);
    g_msg.clear();
}

static void check_slot_rule()
{
    const int32_t none[1] = {0};
    expect(ss::check_slots(none, 0, 4), nullptr, "n_active == 0");
    const int32_t one[] = {3};
    expect(ss::check_slots(one, 1, 4), nullptr, "a single slot");
    const int32_t dup[] = {2, 0, 3, 0};
    expect(ss::check_slots(dup, 4, 4), "entry 3: slot 0 is named twice in one call", "duplicate in the last position");
    const int32_t neg[] = {1, -1, 1};
    expect(ss::check_slots(neg, 3, 4), "entry 1: slot -1 is outside the pool of 4 rows", "-1");
    const int32_t edge[] = {3, 4};
    expect(ss::check_slots(edge, 2, 4), "entry 1: slot 4 is outside the pool of 4 rows", "== pool_streams");
    const int32_t big[] = {INT32_MAX};
    expect(ss::check_slots(big, 1, 4), "entry 0: slot 2147483647 is outside the pool of 4 rows", "INT32_MAX");
    const int32_t perm[] = {5, 2, 0, 4, 1, 3};
    expect(ss::check_slots(perm, 6, 6), nullptr, "a permutation of the whole pool");
}

static void check_clip_table_rule()
{
    const int64_t first[] = {1, 2, 3, 4};
    expect(ss::check_clip_table(first, 3, 10), "offsets[0] must be 0 (clip 0)", "offsets[0] != 0");
    const int64_t dec[] = {0, 5, 4, 9};
    expect(ss::check_clip_table(dec, 3, 10), "decreasing offsets at clip 1", "a decrease at clip 1 of 3");
    const int64_t past[] = {0, 4, 11, 12};
    expect(ss::check_clip_table(past, 3, 10), "clip 1 ends past total_rows", "two clips past total_rows");
    const int64_t dec_and_past[] = {0, 20, 4, 30};  // the decrease is decided first, as before
    expect(ss::check_clip_table(dec_and_past, 3, 10), "decreasing offsets at clip 1", "a decrease and a clip past total_rows");
    const int64_t empty[] = {0, 0, 4, 4, 4, 7};
    expect(ss::check_clip_table(empty, 5, 10), nullptr, "equal neighbours");
    const int64_t full[] = {0, 3, 10};
    expect(ss::check_clip_table(full, 2, 10), nullptr, "last offset == total_rows");
    const int64_t zero[] = {0, 0};
    expect(ss::check_clip_table(zero, 1, 0), nullptr, "an empty block");
}

static void check_clip_group_rule()
{
    const int32_t ok[] = {0, 3, -1, 2, 3, 0};
    expect(ss::check_clip_groups(ok, 6, 4), nullptr, "ids inside the groups, -1 leaves a clip out");
    expect(ss::check_clip_groups(ok, 0, 4), nullptr, "n_clips == 0");
    const int32_t edge[] = {0, 4, 5};
    expect(ss::check_clip_groups(edge, 3, 4), "clip 1: group 4 is outside the 4 groups (-1 leaves a clip out)", "== n_groups: the first is named");
    const int32_t neg[] = {1, -1, -2};
    expect(ss::check_clip_groups(neg, 3, 4), "clip 2: group -2 is outside the 4 groups (-1 leaves a clip out)", "below -1");
    const int32_t big[] = {2147483647};
    expect(ss::check_clip_groups(big, 1, 1), "clip 0: group 2147483647 is outside the 1 groups (-1 leaves a clip out)", "INT32_MAX");
}

static void check_row_offset_rule()
{
    const int64_t first[] = {1, 2, 3, 4};
    expect(ss::check_row_offsets(first, 3), "row_offsets[0] must be 0 (entry 0)", "row_offsets[0] != 0");
    const int64_t dec[] = {0, 5, 4, 9};
    expect(ss::check_row_offsets(dec, 3), "decreasing row offsets at entry 1", "a decrease at entry 1 of 3");
    const int64_t two[] = {0, 5, 4, 3};
    expect(ss::check_row_offsets(two, 3), "decreasing row offsets at entry 1", "two decreases: the first is named");
    const int64_t empty[] = {0, 0, 4, 4, 4, 7};
    expect(ss::check_row_offsets(empty, 5), nullptr, "equal neighbours");
    const int64_t single[] = {0, 0};
    expect(ss::check_row_offsets(single, 1), nullptr, "one entry without rows");
}

static void check_overlap()
{
    const char buf[64] = {};
    CHECK(!ss::ranges_overlap(buf, 16, buf + 16, 16), "adjacent ranges");
    CHECK(!ss::ranges_overlap(buf + 16, 16, buf, 16), "adjacent ranges, swapped");
    CHECK(ss::ranges_overlap(buf, 17, buf + 16, 16), "a one-byte overlap");
    CHECK(ss::ranges_overlap(buf + 16, 16, buf, 17), "a one-byte overlap, swapped");
    // a zero-length range overlaps nothing at either end of another; strictly inside it counts (the interval test, as it always was)
    CHECK(!ss::ranges_overlap(buf, 0, buf, 16), "a zero-length range at the start of another");
    CHECK(!ss::ranges_overlap(buf, 16, buf + 16, 0), "a zero-length range at the end of another");
    CHECK(!ss::ranges_overlap(buf + 8, 0, buf + 8, 0), "two zero-length ranges at one address");
    CHECK(ss::ranges_overlap(buf + 8, 0, buf, 16), "a zero-length range strictly inside another");
    CHECK(ss::ranges_overlap(buf, 64, buf + 8, 8), "one range contains the other");
    CHECK(ss::ranges_overlap(buf + 8, 8, buf, 64), "one range contains the other, swapped");
}

// a pool of 6 rows x len floats of distinct bit patterns (a NaN payload among them), slots {2, 0, 5}
static void check_pool_rows(size_t len)
{
    constexpr size_t kRows = 6, kNamed = 3;
    const int32_t slots[kNamed] = {2, 0, 5};
    std::vector<uint32_t> bits(kRows * len);
    for (size_t i = 0; i < bits.size(); ++i) bits[i] = 0x3f800000u + 0x01010101u * static_cast<uint32_t>(i);
    if (len) bits[2 * len + len - 1] = 0x7fc12345u;  // a quiet NaN with a payload, in a named row
    if (len) bits[3 * len] = 0xffa00001u;            // a signalling NaN pattern, in an unnamed row
    std::vector<float> pool(kRows * len);
    if (len) std::memcpy(pool.data(), bits.data(), bits.size() * sizeof(uint32_t));
    const std::vector<float> before = pool;
    float *p = len ? pool.data() : nullptr;  // a pool without state may be a null pointer
    auto row_bytes = [&](const std::vector<float> &v, size_t r) { return reinterpret_cast<const char *>(v.data()) + r * len * sizeof(float); };

    ss::PoolRows named;
    named.gather(p, slots, kNamed, len);
    CHECK(named.iota.size() == kNamed && named.rows_host.size() == kNamed * len && named.bytes() == kNamed * len * sizeof(float), "len %zu: sizes", len);
    for (size_t i = 0; i < kNamed; ++i) {
        CHECK(named.iota[i] == static_cast<int32_t>(i), "len %zu: iota[%zu]", len, i);
        CHECK(len == 0 || std::memcmp(row_bytes(named.rows_host, i), row_bytes(before, slots[i]), len * sizeof(float)) == 0,
              "len %zu: compact row %zu is not pool row %d", len, i, slots[i]);
    }
    CHECK(len == 0 || std::memcmp(pool.data(), before.data(), pool.size() * sizeof(float)) == 0, "len %zu: gather wrote the pool", len);

    std::vector<uint32_t> fresh(kNamed * len);
    for (size_t i = 0; i < fresh.size(); ++i) fresh[i] = 0xc0000000u + 0x00010203u * static_cast<uint32_t>(i + 1);
    if (len) fresh[0] = 0x7fc54321u;
    if (len) std::memcpy(named.rows_host.data(), fresh.data(), fresh.size() * sizeof(uint32_t));
    const std::vector<float> compact = named.rows_host;
    named.scatter(p, slots);
    for (size_t r = 0; r < kRows && len; ++r) {
        size_t i = 0;
        while (i < kNamed && static_cast<size_t>(slots[i]) != r) ++i;
        if (i < kNamed)
            CHECK(std::memcmp(row_bytes(pool, r), row_bytes(compact, i), len * sizeof(float)) == 0, "len %zu: pool row %zu is not compact row %zu", len, r, i);
        else
            CHECK(std::memcmp(row_bytes(pool, r), row_bytes(before, r), len * sizeof(float)) == 0, "len %zu: unnamed pool row %zu changed", len, r);
    }
}

int main()
{
    check_slot_rule();
    check_clip_table_rule();
    check_clip_group_rule();
    check_row_offset_rule();
    check_overlap();
    for (size_t len : {size_t{4}, size_t{1}, size_t{0}}) check_pool_rows(len);
    if (g_failed) {
        std::printf("%d checks FAILED\n", g_failed);
        return 1;
    }
    std::printf("all checks passed\n");
    return 0;
}
