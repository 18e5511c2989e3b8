// Host-side check of the host-pointer calls' stager in mfcc-rust_amd/csrc/ss_host_stage.h (no GPU, no HIP header): HostStageT over a
// malloc-backed backend that logs every call and fails its k-th one.  Two calls in the shape the library's wrappers have -- a packed
// call (block and table up, the covered rows down) and a pool call (output room, slot table and named rows, block and row offsets
// up; rows and output down; scatter) -- are held to their exact call logs, and then failed at every k in turn: the status and the
// message are the first failure's, nothing but frees reaches the backend after it, the caller's output and pool keep every bit
// (NaN payloads among them) and every block is freed (the leak check).  ss::fail is supplied here: it records the message.
// tests/test_host_stage.py builds it with AddressSanitizer + UBSan and runs it:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Imfcc-rust_amd/csrc
//       tools/hosttest/test_host_stage.cpp -o /tmp/hs && /tmp/hs
#include "ss_host_stage.h"

#include <cstdio>
#include <cstdlib>

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

// The backend: "device" blocks are malloc blocks.  Every call is logged as its letter and size ("A16 U16 S D8 F"); the fail_at-th
// call that is not a free fails without doing anything.
struct FakeDevice {
    std::string log;
    int calls = 0, fail_at = 0, live = 0;
    const char *step(char kind, size_t bytes)
    {
        log += (log.empty() ? "" : " ") + std::string(1, kind) + (kind == 'S' ? "" : std::to_string(bytes));
        return ++calls == fail_at ? "injected" : nullptr;
    }
};
struct FakeBackend {
    FakeDevice *d;
    const char *alloc(void **p, size_t bytes)
    {
        if (const char *e = d->step('A', bytes)) return e;
        *p = std::malloc(bytes);
        ++d->live;
        return nullptr;
    }
    void free(void *p)
    {
        d->log += " F";
        --d->live;
        std::free(p);
    }
    const char *up(void *dev, const void *host, size_t bytes)
    {
        if (const char *e = d->step('U', bytes)) return e;
        std::memcpy(dev, host, bytes);
        return nullptr;
    }
    const char *down(void *host, const void *dev, size_t bytes)
    {
        if (const char *e = d->step('D', bytes)) return e;
        std::memcpy(host, dev, bytes);
        return nullptr;
    }
    const char *sync() { return d->step('S', 0); }
};
using Stage = ss::HostStageT<FakeBackend>;

// distinct bit patterns with NaN payloads among them
static std::vector<float> pattern(size_t n, uint32_t seed)
{
    std::vector<uint32_t> bits(n);
    for (size_t i = 0; i < n; ++i) bits[i] = (i % 3 == 1 ? 0x7fc00000u : 0x3f800000u) + seed + 0x00010203u * static_cast<uint32_t>(i);
    std::vector<float> v(n);
    if (n) std::memcpy(v.data(), bits.data(), n * sizeof(float));
    return v;
}
static bool same_bits(const std::vector<float> &a, const std::vector<float> &b)
{
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(float)) == 0);
}
// what the stand-in device forms compute: every bit flipped
static void flip(float *dst, const float *src, size_t n)
{
    for (size_t i = 0; i < n; ++i) {
        uint32_t u;
        std::memcpy(&u, src + i, 4);
        u = ~u;
        std::memcpy(dst + i, &u, 4);
    }
}

// ---- a packed call: 3 clips (one empty) of 3 columns in a block of 6 rows, the table ends at row 4 ----
constexpr size_t kCols = 3, kRows = 6, kClips = 3;
static const int64_t kOffsets[kClips + 1] = {0, 3, 3, 4};

static int packed_call(FakeDevice &dev, const std::vector<float> &vec, std::vector<float> &out, int device_rc = SS_OK)
{
    const size_t bytes = kRows * kCols * sizeof(float);
    Stage st("demo_packed", FakeBackend{&dev});
    const float *d_in = st.up(vec.data(), bytes);
    const int64_t *d_off = st.up(kOffsets, sizeof(kOffsets));
    float *d_out = st.room<float>(bytes);
    if (st.ok()) {
        CHECK(std::memcmp(d_off, kOffsets, sizeof(kOffsets)) == 0, "the table on the device");
        flip(d_out, d_in, kRows * kCols);
        st.ran(device_rc == SS_OK ? SS_OK : ss::fail(device_rc, "device form"));
    }
    st.sync();
    st.down(out.data(), d_out, static_cast<size_t>(kOffsets[kClips]) * kCols * sizeof(float));  // the rows the table covers
    return st.status();
}

static void check_packed()
{
    const std::vector<float> vec = pattern(kRows * kCols, 0x100u), before = pattern(kRows * kCols, 0x7000u);
    std::vector<float> want = before;
    flip(want.data(), vec.data(), 4 * kCols);
    const char *kLog = "A72 U72 A32 U32 A72 S D48 F F F";
    {
        FakeDevice dev;
        std::vector<float> out = before;
        const int rc = packed_call(dev, vec, out);
        CHECK(rc == SS_OK && g_msg.empty(), "packed: rc %d, message \"%s\"", rc, g_msg.c_str());
        CHECK(dev.log == kLog, "packed: log \"%s\"", dev.log.c_str());
        CHECK(same_bits(out, want), "packed: the covered rows come down, the rows past the table keep the caller's bytes");
        CHECK(dev.live == 0, "packed: %d blocks live", dev.live);
    }
    // every k: allocation / upload -> "host staging", the synchronise -> "<name>: device error", the download -> "hipMemcpy D2H"
    const char *kMsg[] = {"host staging: injected", "host staging: injected", "host staging: injected", "host staging: injected",
                          "host staging: injected", "demo_packed: device error", "hipMemcpy D2H: injected"};
    const char *kFailLog[] = {"A72", "A72 U72 F", "A72 U72 A32 F", "A72 U72 A32 U32 F F", "A72 U72 A32 U32 A72 F F", "A72 U72 A32 U32 A72 S F F F",
                              "A72 U72 A32 U32 A72 S D48 F F F"};
    for (int k = 1; k <= 7; ++k) {
        FakeDevice dev;
        dev.fail_at = k;
        std::vector<float> out = before;
        const int rc = packed_call(dev, vec, out);
        CHECK(rc == SS_ERR_HIP && g_msg == kMsg[k - 1], "packed, k = %d: rc %d, message \"%s\"", k, rc, g_msg.c_str());
        CHECK(dev.log == kFailLog[k - 1], "packed, k = %d: log \"%s\"", k, dev.log.c_str());
        CHECK(same_bits(out, before), "packed, k = %d: out was written", k);
        CHECK(dev.live == 0, "packed, k = %d: %d blocks live", k, dev.live);
        g_msg.clear();
    }
    {  // the device form's own status stays: no synchronise, nothing comes down
        FakeDevice dev;
        std::vector<float> out = before;
        const int rc = packed_call(dev, vec, out, SS_ERR_ARG);
        CHECK(rc == SS_ERR_ARG && g_msg == "device form", "packed, device form fails: rc %d, message \"%s\"", rc, g_msg.c_str());
        CHECK(dev.log == "A72 U72 A32 U32 A72 F F F" && same_bits(out, before) && dev.live == 0, "packed, device form fails: log \"%s\"", dev.log.c_str());
        g_msg.clear();
    }
}

// ---- a pool call: a pool of 6 rows of len floats, slots {2, 0, 5}; 5 rows of 2 columns in, the same out ----
constexpr size_t kPool = 6, kNamed = 3, kInRows = 5, kInCols = 2;
static const int32_t kSlots[kNamed] = {2, 0, 5};
static const int64_t kRowOffsets[kNamed + 1] = {0, 2, 2, 5};

static int pool_call(FakeDevice &dev, const std::vector<float> &vec, size_t len, std::vector<float> &pool, std::vector<float> &out, const char *what = "")
{
    const size_t bytes = kInRows * kInCols * sizeof(float);
    float *p = len ? pool.data() : nullptr;  // a pool without state may be a null pointer
    ss::PoolRows named;
    named.gather(p, kSlots, kNamed, len);
    Stage st("demo_pool", FakeBackend{&dev});
    float *d_out = st.room<float>(bytes);
    const auto d_named = st.up_pool(named);
    const float *d_vec = st.up(vec.data(), bytes);
    const int64_t *d_ro = st.up(kRowOffsets, sizeof(kRowOffsets));
    if (st.ok()) {
        CHECK(d_ro[kNamed] == 5 && d_named.slots[0] == 0 && d_named.slots[1] == 1 && d_named.slots[2] == 2, "the tables on the device");
        CHECK((d_named.rows != nullptr) == (len > 0), "len %zu: the staged rows", len);
        flip(d_out, d_vec, kInRows * kInCols);
        if (len) flip(d_named.rows, d_named.rows, kNamed * len);
        st.ran(SS_OK);
    }
    st.sync();
    st.down_pool(named, d_named, what);
    st.down(out.data(), d_out, bytes);
    st.scatter(named, p, kSlots);
    return st.status();
}

static void check_pool(size_t len)
{
    const std::vector<float> vec = pattern(kInRows * kInCols, 0x200u), out_before = pattern(kInRows * kInCols, 0x6000u), pool_before = pattern(kPool * len, 0x300u);
    std::vector<float> out_want(out_before.size()), pool_want = pool_before;
    flip(out_want.data(), vec.data(), out_want.size());
    for (size_t i = 0; i < kNamed && len; ++i) flip(pool_want.data() + kSlots[i] * len, pool_before.data() + kSlots[i] * len, len);
    // 4 floats per row: 48 bytes of rows; no state: the rows are neither allocated nor copied
    const std::string log = len ? "A40 A12 U12 A48 U48 A40 U40 A32 U32 S D48 D40 F F F F F" : "A40 A12 U12 A40 U40 A32 U32 S D40 F F F F";
    const int n_calls = len ? 12 : 9, sync_at = len ? 10 : 8;
    {
        FakeDevice dev;
        std::vector<float> out = out_before, pool = pool_before;
        const int rc = pool_call(dev, vec, len, pool, out);
        CHECK(rc == SS_OK && g_msg.empty(), "pool, len %zu: rc %d, message \"%s\"", len, rc, g_msg.c_str());
        CHECK(dev.log == log, "pool, len %zu: log \"%s\"", len, dev.log.c_str());
        CHECK(same_bits(out, out_want), "pool, len %zu: out", len);
        CHECK(same_bits(pool, pool_want), "pool, len %zu: exactly the named rows change", len);
        CHECK(dev.live == 0, "pool, len %zu: %d blocks live", len, dev.live);
    }
    for (int k = 1; k <= n_calls; ++k) {
        FakeDevice dev;
        dev.fail_at = k;
        std::vector<float> out = out_before, pool = pool_before;
        const int rc = pool_call(dev, vec, len, pool, out, k == sync_at + 1 ? " (pool rows)" : "");
        const std::string want = k < sync_at    ? "host staging: injected"
                                 : k == sync_at ? "demo_pool: device error"
                                 : k == sync_at + 1 && len ? "hipMemcpy D2H (pool rows): injected"
                                                           : "hipMemcpy D2H: injected";
        CHECK(rc == SS_ERR_HIP && g_msg == want, "pool, len %zu, k = %d: rc %d, message \"%s\"", len, k, rc, g_msg.c_str());
        // the log: what the whole call logs up to its k-th call, then frees only
        size_t cut = 0;
        for (int c = 0; c < k; ++c) cut = log.find(' ', cut + 1);
        const size_t tail = dev.log.find(" F");
        CHECK(dev.log.substr(0, std::min(tail, dev.log.size())) == log.substr(0, cut), "pool, len %zu, k = %d: log \"%s\"", len, k, dev.log.c_str());
        CHECK(tail == std::string::npos || dev.log.find_first_not_of(" F", tail) == std::string::npos, "pool, len %zu, k = %d: a call after the failure: \"%s\"", len, k,
              dev.log.c_str());
        CHECK(same_bits(pool, pool_before), "pool, len %zu, k = %d: the pool was written", len, k);
        // the rows come down before out, so out keeps its bytes on every failure too
        CHECK(same_bits(out, out_before), "pool, len %zu, k = %d: out was written", len, k);
        CHECK(dev.live == 0, "pool, len %zu, k = %d: %d blocks live", len, k, dev.live);
        g_msg.clear();
    }
}

// a zero-byte item: the block alone (16 bytes, never null), nothing is copied either way
static void check_zero_bytes()
{
    FakeDevice dev;
    float host = 1.0f;
    {
        Stage st("demo_zero", FakeBackend{&dev});
        float *d_a = st.up(&host, 0), *d_b = st.up(static_cast<const float *>(nullptr), 0), *d_c = st.room<float>(0);
        CHECK(st.ok() && d_a && d_b && d_c, "zero bytes: the blocks");
        st.fill(d_a, &host, 0);
        st.down(&host, d_a, 0);
        st.down(nullptr, d_c, 0);
        CHECK(st.status() == SS_OK && g_msg.empty(), "zero bytes: rc %d, message \"%s\"", st.status(), g_msg.c_str());
    }
    CHECK(dev.log == "A16 A16 A16 F F F" && dev.live == 0, "zero bytes: log \"%s\"", dev.log.c_str());
}

int main()
{
    check_packed();
    for (size_t len : {size_t{4}, size_t{0}}) check_pool(len);
    check_zero_bytes();
    if (g_failed) {
        std::printf("%d checks FAILED\n", g_failed);
        return 1;
    }
    std::printf("all checks passed\n");
    return 0;
}
