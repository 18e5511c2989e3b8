// The stream-pool builds of ss_nemo_c256 (ss_nstream_log_mel_packed*_device, ss_nstream_flush_device): the NeMo / Parakeet log-mel
// front end over a pool of stream states, fed ragged float or 16-bit PCM chunks, and the flush of a stream's last rows.  The kernel
// is ss_nemo_body.h's one template -- the same pre-emphasis, window, FFT, untangle, mel and ln as the dense and packed builds of
// ss_nemo512.hip, which is what makes a stream's rows bit for bit the dense call's -- with the pool's row lookup and loaders
// (load_quad_npool, load_quad_nflush) in front.  A translation unit of its own: nine more builds, {NE 10, 13, 16} x {float, PCM, flush},
// next to the six of ss_nemo512.hip.  The state advance is not here: it is the frame pool's second launch
// (launch_stream_advance_packed) over the same entry block.  The flush's second launch is: ss_nstream_zero_rows below.
#include "ss_nemo_body.h"

namespace ss {

namespace {

constexpr int kWaves = 12;

size_t nemo_lds(const NemoArgs &a)
{
    return (static_cast<size_t>(kWaves) * kWaveFloats + L::kMelW + 16 * static_cast<size_t>(a.mel_wpitch) + 4) * sizeof(float);
}

// SPT = FrameStreamPackedArgs (float chunks), FrameStreamPackedPcmArgs (16-bit PCM) or NemoFlushArgs; total: its rows
template <typename SPT>
hipError_t launch_pool(const NemoArgs &a, const SPT &sp, unsigned long long total, hipStream_t stream, int num_cus, LaunchInfo *info)
{
    const size_t lds = nemo_lds(a);
    GroupPlan plan;
    const PlanStatus ps = plan_groups(total, 0u, 4, false, lds, kWaves, num_cus, plan);
    if (ps == PlanStatus::Invalid) return hipErrorInvalidValue;
    if (ps == PlanStatus::Empty) plan.grid = 1u;  // an empty output block still gets one workgroup: the entry pass runs
    auto go = [&](auto kern, const char *name) { return launch_kernel(kern, name, plan.grid, kWaves, lds, stream, info, a, NemoVarlenArgs{}, sp); };
    constexpr int k = std::is_same_v<SPT, NemoFlushArgs> ? 2 : std::is_same_v<SPT, FrameStreamPackedPcmArgs> ? 1 : 0;
    static const char *const names[3][3] = {{"ss_nemo_c256<10,sp>", "ss_nemo_c256<10,spi>", "ss_nemo_c256<10,fl>"},
                                            {"ss_nemo_c256<13,sp>", "ss_nemo_c256<13,spi>", "ss_nemo_c256<13,fl>"},
                                            {"ss_nemo_c256<16,sp>", "ss_nemo_c256<16,spi>", "ss_nemo_c256<16,fl>"}};
    if (a.win_len <= 320) return go(ss_nemo_c256<10, false, kWaves, SPT>, names[0][k]);
    if (a.win_len <= 416) return go(ss_nemo_c256<13, false, kWaves, SPT>, names[1][k]);
    return go(ss_nemo_c256<16, false, kWaves, SPT>, names[2][k]);
}

bool nemo_shape_ok(const NemoArgs &a)
{
    return a.win_len >= 258 && a.win_len <= 512 && (a.win_len & 1u) == 0u && a.n_mels != 0 && a.n_mels <= kNemoMaxMels;
}

// The flush's second launch: pool row slots[i] := 0 for every entry whose slot names a pool row; any other entry raises the error
// word (a vector store to the pinned word).  A workgroup per entry, grid-stride.
__global__ __launch_bounds__(256) void ss_nstream_zero_rows(const NemoFlushArgs s)
{
    for (unsigned e = blockIdx.x; e < s.n_active; e += gridDim.x) {
        const int slot = s.slots[e];
        if (slot < 0 || static_cast<unsigned>(slot) >= s.pool_streams) {
            if (threadIdx.x == 0 && s.err) __hip_atomic_store(s.err, kVarlenError, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            continue;
        }
        float *st = s.pool + static_cast<unsigned long long>(slot) * s.state_len;
        for (unsigned i = threadIdx.x; i < s.state_len; i += 256) st[i] = 0.f;
    }
}

}  // namespace

hipError_t launch_nemo_c256_stream_packed(const NemoArgs &a, const FrameStreamPackedPcmArgs &sp, bool pcm, hipStream_t stream, int num_cus,
                                          LaunchInfo *info)
{
    const FrameStreamPackedArgs &s = sp.e;
    if (!nemo_shape_ok(a)) return hipErrorInvalidValue;
    if (!s.so || !s.ro || !s.slots || !s.pool || s.n_active == 0 || s.step != kNemoHop) return hipErrorInvalidValue;
    // S = 160 L + W / 2 + 1 and lead = S - 1 with W / 2 <= 160 (L + 1): a row's frame and its predecessor start inside the pool row,
    // and the frame ends inside its chunk
    if (s.lead < 0 || s.state_len != static_cast<uint32_t>(s.lead) + 1u || (static_cast<uint32_t>(s.lead) - a.win_len / 2) % kNemoHop != 0 ||
        a.win_len / 2 > static_cast<uint32_t>(s.lead) || a.win_len > static_cast<uint32_t>(s.lead) + kNemoHop)
        return hipErrorInvalidValue;
    if (static_cast<unsigned long long>(s.total_rows) + 4 >= (1ull << 31)) return hipErrorInvalidValue;
    if (pcm ? (!sp.x || (reinterpret_cast<uintptr_t>(sp.x) & 1u)) : !a.x) return hipErrorInvalidValue;
    return pcm ? launch_pool(a, sp, s.total_rows, stream, num_cus, info) : launch_pool(a, s, s.total_rows, stream, num_cus, info);
}

hipError_t launch_nemo_c256_flush(const NemoArgs &a, const NemoFlushArgs &s, hipStream_t stream, int num_cus, LaunchInfo *info)
{
    if (!nemo_shape_ok(a)) return hipErrorInvalidValue;
    if (!s.slots || !s.pool || s.n_active == 0) return hipErrorInvalidValue;
    // every position a row reads, its predecessor included, lies inside the pool row: 160 L + W / 2 + 1 <= S
    if (static_cast<unsigned long long>(s.delay) * kNemoHop + a.win_len / 2 + 1 > s.state_len) return hipErrorInvalidValue;
    const unsigned long long total = static_cast<unsigned long long>(s.n_active) * s.delay;
    if (total + 4 >= (1ull << 31)) return hipErrorInvalidValue;
    if (total > 0) {
        if (!a.out) return hipErrorInvalidValue;
        const hipError_t e = launch_pool(a, s, total, stream, num_cus, info);
        if (e != hipSuccess) return e;
    }
    const unsigned grid = s.n_active < 4096u ? s.n_active : 4096u;
    if (total == 0 && info) *info = LaunchInfo{"ss_nstream_zero_rows", grid, 256u, 0};
    hipLaunchKernelGGL(ss_nstream_zero_rows, dim3(grid), dim3(256), 0, stream, s);
    return hipGetLastError();
}

}  // namespace ss
