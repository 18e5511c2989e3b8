// The stream-pool builds of ss_kaldi_c256 (ss_kstream_*_packed_device): the Kaldi-compatible fbank / MFCC front end over a pool of
// stream states, fed ragged float or 16-bit PCM chunks.  The kernel is ss_kaldi_body.h's one template -- the same conditioning stage,
// FFT, untangle, mel, ln and DCT as the dense and packed builds of ss_kaldi512.hip, which is what makes a stream's rows bit for bit
// the dense call's on zeros(S) ++ stream -- with the pool's row lookup and loader (load_quad_pool) in front.  A translation unit of
// its own: 24 more builds, {NE 10, 13, 16} x {pow2, magnitude} x {fbank, mfcc} x {float, PCM}, next to the 48 of ss_kaldi512.hip.
// The state advance is not here: it is the frame pool's second launch (launch_stream_advance_packed) over the same entry block.
#include "ss_kaldi_body.h"

namespace ss {

namespace {

// SPT = FrameStreamPackedArgs (float chunks) or FrameStreamPackedPcmArgs (16-bit PCM); s = its entry block
template <typename SPT>
hipError_t launch_pool(const KaldiArgs &a, const SPT &sp, const FrameStreamPackedArgs &s, hipStream_t stream, int num_cus, LaunchInfo *info)
{
    constexpr int WAVES = 12;
    constexpr bool PCM = std::is_same_v<SPT, FrameStreamPackedPcmArgs>;
    const size_t lds = (static_cast<size_t>(WAVES) * kWaveFloats + L::kMelW + 16 * static_cast<size_t>(a.mel_wpitch) + 512 + 4) * sizeof(float);
    GroupPlan plan;
    const PlanStatus ps = plan_groups(s.total_rows, 0u, 4, false, lds, WAVES, num_cus, plan);
    if (ps == PlanStatus::Invalid) return hipErrorInvalidValue;
    if (ps == PlanStatus::Empty) plan.grid = 1u;  // an empty output block still gets one workgroup: the entry pass runs
    auto go = [&](auto kern, const char *name) { return launch_kernel(kern, name, plan.grid, WAVES, lds, stream, info, a, KaldiVarlenArgs{}, sp); };
    const bool pow2 = a.use_power != 0, mfcc = a.out_mfcc != 0;
#define SS_K(NE, P, C, NAME) go(ss_kaldi_c256<NE, P, C, false, WAVES, SPT>, PCM ? NAME ",spi>" : NAME ",sp>")
#define SS_KN(NE, TAG)                                                                                                     \
    if (pow2) return mfcc ? SS_K(NE, true, true, "ss_kaldi_c256<" TAG ",pow2,mfcc") : SS_K(NE, true, false, "ss_kaldi_c256<" TAG ",pow2,fbank"); \
    return mfcc ? SS_K(NE, false, true, "ss_kaldi_c256<" TAG ",mfcc") : SS_K(NE, false, false, "ss_kaldi_c256<" TAG ",fbank");
    if (a.flen <= 320) { SS_KN(10, "10") }
    if (a.flen <= 416) { SS_KN(13, "13") }
    SS_KN(16, "16")
#undef SS_KN
#undef SS_K
}

}  // namespace

hipError_t launch_kaldi_c256_stream_packed(const KaldiArgs &a, const FrameStreamPackedPcmArgs &sp, bool pcm, hipStream_t stream, int num_cus,
                                           LaunchInfo *info)
{
    const FrameStreamPackedArgs &s = sp.e;
    if (a.flen <= 256 || a.flen > 512 || a.step == 0 || a.n_filters > 80 || a.n_ceps > 32) return hipErrorInvalidValue;
    if (!s.so || !s.ro || !s.slots || s.n_active == 0 || s.step != a.step || (s.state_len > 0 && !s.pool)) return hipErrorInvalidValue;
    // S = D * step with flen <= (D + 1) * step: a row's frame starts inside the pool row and ends inside its chunk
    if (s.state_len % a.step != 0 || static_cast<unsigned long long>(s.state_len) + a.step < a.flen) return hipErrorInvalidValue;
    if (static_cast<unsigned long long>(s.total_rows) + 4 >= (1ull << 31)) return hipErrorInvalidValue;
    if (pcm ? (!sp.x || (reinterpret_cast<uintptr_t>(sp.x) & 1u)) : !a.x) return hipErrorInvalidValue;
    return pcm ? launch_pool(a, sp, s, stream, num_cus, info) : launch_pool(a, s, s, stream, num_cus, info);
}

}  // namespace ss
