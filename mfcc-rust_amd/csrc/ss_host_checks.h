// The table and pool rules of the host-pointer calls, each in one place: what a call rejects before the device is touched (the fixed
// messages that tests pin) and the pool-row gather / scatter around a staged pool call.  Pure host C++17 -- no HIP include, nothing
// but ss::fail from ss_internal.h -- so tools/hosttest/test_host_checks.cpp runs it under the sanitizers without a device.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>
#include <unordered_set>
#include <vector>

#include "ss_internal.h"

namespace ss {

inline bool ranges_overlap(const void *a, size_t a_bytes, const void *b, size_t b_bytes)
{
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
    return a0 < b0 + b_bytes && b0 < a0 + a_bytes;
}

// the sample scale of a 16-bit PCM call: a power of two in [2^-64, 2^64] -- the product with an int16 is exact (and never subnormal)
inline bool pcm_scale_ok(float scale)
{
    int ex = 0;
    return std::isfinite(scale) && scale > 0.0f && std::frexp(scale, &ex) == 0.5f && ex - 1 >= -64 && ex - 1 <= 64;
}
// the _i16 / ss_kpcm_* entry points' check of it, before anything runs
inline int check_pcm_scale(float scale)
{
    return pcm_scale_ok(scale) ? SS_OK : fail(SS_ERR_ARG, "scale must be a power of two in [2^-64, 2^64]");
}

// the slots of a host-pointer pool call: inside the pool, none named twice
inline int check_slots(const int32_t *slots, size_t n_active, size_t pool_streams)
{
    std::unordered_set<int32_t> seen;
    seen.reserve(n_active);
    for (size_t i = 0; i < n_active; ++i) {
        if (slots[i] < 0 || static_cast<size_t>(slots[i]) >= pool_streams)
            return fail(SS_ERR_ARG, "entry " + std::to_string(i) + ": slot " + std::to_string(slots[i]) + " is outside the pool of " +
                                        std::to_string(pool_streams) + " rows");
        if (!seen.insert(slots[i]).second)
            return fail(SS_ERR_ARG, "entry " + std::to_string(i) + ": slot " + std::to_string(slots[i]) + " is named twice in one call");
    }
    return SS_OK;
}

// the segment table of a host-pointer packed call (n_clips + 1 offsets): starts at 0, does not decrease, no clip ends past
// total_rows; the first offending clip is named
inline int check_clip_table(const int64_t *off, size_t n_clips, size_t total_rows)
{
    if (off[0] != 0) return fail(SS_ERR_ARG, "offsets[0] must be 0 (clip 0)");
    for (size_t b = 0; b < n_clips; ++b)
        if (off[b + 1] < off[b]) return fail(SS_ERR_ARG, "decreasing offsets at clip " + std::to_string(b));
    for (size_t b = 0; b < n_clips; ++b)
        if (static_cast<uint64_t>(off[b + 1]) > total_rows) return fail(SS_ERR_ARG, "clip " + std::to_string(b) + " ends past total_rows");
    return SS_OK;
}

// the group table of a host-pointer grouped-CMVN call: every id in [0, n_groups), or -1 (the clip is left out)
inline int check_clip_groups(const int32_t *groups, size_t n_clips, size_t n_groups)
{
    for (size_t b = 0; b < n_clips; ++b)
        if (groups[b] < -1 || (groups[b] >= 0 && static_cast<size_t>(groups[b]) >= n_groups))
            return fail(SS_ERR_ARG, "clip " + std::to_string(b) + ": group " + std::to_string(groups[b]) + " is outside the " +
                                        std::to_string(n_groups) + " groups (-1 leaves a clip out)");
    return SS_OK;
}

// the row offsets of a host-pointer pool call (n_active + 1 of them; the block's row count is their last)
inline int check_row_offsets(const int64_t *ro, size_t n_active)
{
    if (ro[0] != 0) return fail(SS_ERR_ARG, "row_offsets[0] must be 0 (entry 0)");
    for (size_t i = 0; i < n_active; ++i)
        if (ro[i + 1] < ro[i]) return fail(SS_ERR_ARG, "decreasing row offsets at entry " + std::to_string(i));
    return SS_OK;
}

// The pool rows a host-pointer pool call stages: the n_active named rows of the caller's pool as a compact block whose row i is
// entry i's, and the slot table 0 .. n_active - 1 the device call runs on.  scatter() copies the block back to the named rows and
// to nowhere else; the caller runs it only once everything before it succeeded.  len == 0 (a pool without state) moves nothing.
struct PoolRows {
    std::vector<float> rows_host;
    std::vector<int32_t> iota;
    size_t len = 0;

    void gather(const float *pool, const int32_t *slots, size_t n_active, size_t row_len)
    {
        len = row_len;
        rows_host.resize(n_active * len);
        iota.resize(n_active);
        for (size_t i = 0; i < n_active; ++i) {
            iota[i] = static_cast<int32_t>(i);
            if (len > 0) std::memcpy(rows_host.data() + i * len, pool + static_cast<size_t>(slots[i]) * len, len * sizeof(float));
        }
    }
    void scatter(float *pool, const int32_t *slots) const
    {
        for (size_t i = 0; len > 0 && i < iota.size(); ++i)
            std::memcpy(pool + static_cast<size_t>(slots[i]) * len, rows_host.data() + i * len, len * sizeof(float));
    }
    size_t bytes() const { return rows_host.size() * sizeof(float); }
};

}  // namespace ss
