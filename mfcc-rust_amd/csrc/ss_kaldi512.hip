// ss_kaldi_c256: the Kaldi-compatible fbank / MFCC front end (compute-fbank-feats / compute-mfcc-feats as
// torchaudio.compliance.kaldi restates them) for frames that pad to 512 points, on gfx950.  The specification is the ss_kaldi_*
// comment of include/speechsauce_amd.h; the reference crate has no such path, so this file restates nothing of it.
//
// The quad skeleton (a QUAD of 4 consecutive frames of the flat frame list per wave, 16 lanes per frame, persistent 12-wave
// workgroups, the two radix-16 passes and the untangle) is ss_quad256.h; the table block is ss::KaldiTables (mfcc512w_layout + the
// window).  Zero padding is compile-time (template NE).  What is this file's own:
//   * between the load and the first butterfly, on the input registers: the per-frame conditioning stage -- input scale, DC
//     removal (frame sum by row16_sum, a true division, the pad kept at zero), raw energy, per-frame pre-emphasis (the predecessor
//     of s[2n] is the neighbouring lane's .y: one row_ror:1 DPP move per pair and a select for lane 0, whose predecessor sits one
//     register earlier in lane 15), window, windowed energy.
//   * The P row holds the unscaled |2X|^2 or |2X|; the 1/4 or 1/2 rides on the mel sums (exact: a power of two).  No 1/N, no
//     T-dependent scale; the Nyquist bin has no weight in the bank.
//   * banded mel, five filters per lane, max(., eps) and v_log_f32 (eps is a normal f32: no pre-scale), then either the [T x M]
//     row (+ the log energy) or the DCT against the lane's liftered table row, c[0] replaced by the log energy under use_energy.
//   * VARLEN: the flat frame index is the output row of a packed launch; clip and frame come from fo / so by offset_seek /
//     offset_find, every T_b is recomputed from so, an inconsistent clip is skipped (no load, no store) and raises the error word.
//   * Frame starts: a quad whose four frame starts are all 8-byte aligned loads sample pairs as float2; any other quad (odd
//     shift, odd ld, odd clip offset, an unaligned base) loads single floats.  The choice is per quad and wave-uniform.
//   * 16-bit PCM (ss_kpcm_*; a KaldiPcmArgs / KaldiVarlenPcmArgs behind the kernel's two arguments): a sample pair is one dword at
//     2-byte alignment, so every frame start takes the one path; the dword stays raw until the conditioning stage converts it
//     (exact: a power-of-two scale), which is what makes the rows bit for bit the float build's on the converted samples.
//     Reported as ss_kaldi_c256<..,i> (dense) and <..,vi> (packed).
// The kernel template itself is ss_kaldi_body.h, shared with the stream-pool builds of ss_kaldi512_pool.hip; this file holds the
// launchers of the dense and packed builds.
#include "ss_kaldi_body.h"

namespace ss {

namespace {

// PCM: nothing (float samples at a.x; v: the packed call's tables), or the call's PCM pack (v: the tables it carries)
template <bool VARLEN, typename... PCM>
hipError_t launch_k(const KaldiArgs &a_in, const KaldiVarlenArgs &v, hipStream_t stream, int num_cus, LaunchInfo *info, const PCM &...pcm)
{
    constexpr int WAVES = 12;
    constexpr bool I16 = sizeof...(PCM) > 0;
    KaldiArgs a = a_in;
    const unsigned long long total = VARLEN ? v.total_frames : static_cast<unsigned long long>(a.batch) * a.n_frames;
    if (a.flen <= 256 || a.flen > 512 || a.step == 0 || a.n_filters > 80 || a.n_ceps > 32) return hipErrorInvalidValue;
    const size_t lds = (static_cast<size_t>(WAVES) * kWaveFloats + L::kMelW + 16 * static_cast<size_t>(a.mel_wpitch) + 512 + 4) * sizeof(float);
    GroupPlan plan;
    const PlanStatus ps = plan_groups(total, a.n_frames, 4, !VARLEN, lds, WAVES, num_cus, plan);
    if (ps != PlanStatus::Launch) return ps == PlanStatus::Empty ? hipSuccess : hipErrorInvalidValue;
    a.nf_magic = plan.nf_magic;
    a.nf_shift = plan.nf_shift;
    // (a PCM pack's tables ride in the pack: the kernel's own table argument stays empty)
    auto go = [&](auto kern, const char *name) { return launch_kernel(kern, name, plan.grid, WAVES, lds, stream, info, a, I16 ? KaldiVarlenArgs{} : v, pcm...); };
    const bool pow2 = a.use_power != 0, mfcc = a.out_mfcc != 0;
#define SS_K(NE, P, C, NAME) go(ss_kaldi_c256<NE, P, C, VARLEN, WAVES, PCM...>, I16 ? (VARLEN ? NAME ",vi>" : NAME ",i>") : (VARLEN ? NAME ",v>" : NAME ">"))
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

hipError_t launch_kaldi_c256(const KaldiArgs &a, hipStream_t stream, int num_cus, LaunchInfo *info)
{
    return launch_k<false>(a, KaldiVarlenArgs{}, stream, num_cus, info);
}

hipError_t launch_kaldi_c256_varlen(const KaldiArgs &a, const KaldiVarlenArgs &v, hipStream_t stream, int num_cus, LaunchInfo *info)
{
    if (!v.so || !v.fo || v.n_clips == 0) return hipErrorInvalidValue;
    return launch_k<true>(a, v, stream, num_cus, info);
}

hipError_t launch_kaldi_c256(const KaldiArgs &a, const KaldiPcmArgs &p, hipStream_t stream, int num_cus, LaunchInfo *info)
{
    if (!p.x || (reinterpret_cast<uintptr_t>(p.x) & 1u)) return hipErrorInvalidValue;
    return launch_k<false>(a, KaldiVarlenArgs{}, stream, num_cus, info, p);
}

hipError_t launch_kaldi_c256_varlen(const KaldiArgs &a, const KaldiVarlenPcmArgs &v, hipStream_t stream, int num_cus, LaunchInfo *info)
{
    if (!v.v.so || !v.v.fo || v.v.n_clips == 0 || !v.x || (reinterpret_cast<uintptr_t>(v.x) & 1u)) return hipErrorInvalidValue;
    return launch_k<true>(a, v.v, stream, num_cus, info, v);
}

}  // namespace ss
