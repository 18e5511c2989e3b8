// ss_nemo_c256 and ss_nemo_norm_kernel: the NeMo / Parakeet log-mel front end (NeMo's FilterbankFeatures as
// transformers.ParakeetFeatureExtractor restates it) for 512-point frames at a 160-sample hop, on gfx950.  The specification is the
// ss_nemo_* comment of include/speechsauce_amd.h; the reference crate has no such path, so this file restates nothing of it.
//
// The quad skeleton (a QUAD of 4 consecutive rows of the flat row list per wave, 16 lanes per frame, persistent 12-wave
// workgroups, the two radix-16 passes and the untangle) is ss_quad256.h; the table block is ss::NemoTables (nemo512_layout).  Zero
// padding behind the window is compile-time (template NE, as in ss_kaldi_c256).  The kernel itself is ss_nemo_body.h's one template;
// this file holds its dense and packed builds.  What is the front end's own:
//   * The loader.  Frame t of a clip starts at clip sample 160 t - W / 2: before the clip for the first frames, and it runs past
//     the clip's end for the last ones; a clip shorter than W has only such frames.  Samples outside [0, len) are zero and are
//     NOT fetched -- in a packed block they are the neighbour's, at the block's edge they are nobody's.  A quad whose four frames
//     lie wholly inside their clips takes the path without per-sample tests (float2 where the four starts are 8-byte aligned);
//     any other quad tests every sample.  The choice is per quad and wave-uniform and changes no bit: both fetch the same samples.
//   * Whole-clip pre-emphasis on the input registers: the predecessor of s[2n] is the neighbouring lane's .y (one row_ror:1 DPP
//     move per pair and a select for lane 0, whose predecessor sits one register earlier in lane 15); the predecessor of the
//     frame's first live sample is the clip's real x[start - 1] -- one more load in lane 0 -- or 0 at the clip's start.  Positions
//     at or beyond len are cleared afterwards (the extractor's masked_fill): only an edge quad has any.
//   * Banded mel over EIGHT filter slots per lane (128 bands over 16 lanes), ln(0.25 sum + guard) by v_log_f32 (the guard is a
//     normal f32: no pre-scale), the row gathered in band order in the slot behind the P row and stored coalesced.
//   * VARLEN: the flat row index is the output row of a packed launch; clip and frame come from fo / so (row_owner), every T_b is
//     recomputed from so, an inconsistent clip is skipped (no load, no store) and raises the error word.  A clip without rows
//     (fewer than 160 samples) is consistent.
//   * ss_nemo_norm_kernel: per clip and band the two f64 sums of step 8 in row order, then the apply, in place; one thread per
//     (clip, band), neighbouring threads neighbouring bands, so a clip's bits depend on its own rows alone.
#include "ss_nemo_body.h"

namespace ss {

namespace {

// Step 8 in place: thread id = clip * n_mels + band, so neighbouring lanes read neighbouring bands of one row.  The loads of a pass
// are independent of its sums: the unrolled loops keep eight rows in flight while the additions stay in row order.  (Batches of 32
// rows loaded up front and then consumed ran this kernel at half the rate on an MI355X, 2026-10-21: the plain loops overlap
// the next rows' loads with the f64 arithmetic of the current ones.)
__global__ __launch_bounds__(256) void ss_nemo_norm_kernel(const NemoArgs a, const NemoVarlenArgs v, const int varlen)
{
#pragma clang fp contract(off)
    const unsigned M = a.n_mels;
    const unsigned long long id = blockIdx.x * 256ull + threadIdx.x;
    const unsigned long long n = static_cast<unsigned long long>(varlen ? v.n_clips : a.batch) * M;
    if (id >= n) return;
    const unsigned b = static_cast<unsigned>(id / M), m = static_cast<unsigned>(id - static_cast<unsigned long long>(b) * M);
    unsigned long long r0 = static_cast<unsigned long long>(b) * a.n_frames;
    unsigned T = a.n_frames;
    if (varlen) {
        const NClip c = nemo_clip(v, b);
        if (!c.ok) return;  // skipped by every launch
        r0 = static_cast<unsigned long long>(c.f0);
        T = c.T;
    }
    if (T == 0) return;
    float *p = a.out + r0 * M + m;
    double sum = 0.0;
#pragma unroll 8
    for (unsigned t = 0; t < T; ++t) sum += static_cast<double>(p[static_cast<size_t>(t) * M]);
    const double mean = sum / static_cast<double>(T);
    double sq = 0.0;
#pragma unroll 8
    for (unsigned t = 0; t < T; ++t) {
        const double d = static_cast<double>(p[static_cast<size_t>(t) * M]) - mean;
        sq += d * d;
    }
    const double den = (T > 1 ? sqrt(sq / static_cast<double>(T - 1)) : 0.0) + static_cast<double>(a.norm_eps);
#pragma unroll 4
    for (unsigned t = 0; t < T; ++t) {
        float *q = p + static_cast<size_t>(t) * M;
        *q = static_cast<float>((static_cast<double>(*q) - mean) / den);
    }
}

template <bool VARLEN>
hipError_t launch_n(const NemoArgs &a_in, const NemoVarlenArgs &v, hipStream_t stream, int num_cus, LaunchInfo *info)
{
    constexpr int WAVES = 12;
    NemoArgs a = a_in;
    const unsigned long long total = VARLEN ? v.total_frames : static_cast<unsigned long long>(a.batch) * a.n_frames;
    if (a.win_len < 258 || a.win_len > 512 || (a.win_len & 1u) || a.n_mels == 0 || a.n_mels > kNemoMaxMels) return hipErrorInvalidValue;
    const size_t lds = (static_cast<size_t>(WAVES) * kWaveFloats + L::kMelW + 16 * static_cast<size_t>(a.mel_wpitch) + 4) * sizeof(float);
    GroupPlan plan;
    const PlanStatus ps = plan_groups(total, a.n_frames, 4, !VARLEN, lds, WAVES, num_cus, plan);
    if (ps != PlanStatus::Launch) return ps == PlanStatus::Empty ? hipSuccess : hipErrorInvalidValue;
    a.nf_magic = plan.nf_magic;
    a.nf_shift = plan.nf_shift;
    auto go = [&](auto kern, const char *name) { return launch_kernel(kern, name, plan.grid, WAVES, lds, stream, info, a, v); };
#define SS_N(NE, TAG) go(ss_nemo_c256<NE, VARLEN, WAVES>, VARLEN ? "ss_nemo_c256<" TAG ",v>" : "ss_nemo_c256<" TAG ">")
    if (a.win_len <= 320) return SS_N(10, "10");
    if (a.win_len <= 416) return SS_N(13, "13");
    return SS_N(16, "16");
#undef SS_N
}

}  // namespace

hipError_t launch_nemo_c256(const NemoArgs &a, hipStream_t stream, int num_cus, LaunchInfo *info)
{
    return launch_n<false>(a, NemoVarlenArgs{}, stream, num_cus, info);
}

hipError_t launch_nemo_c256_varlen(const NemoArgs &a, const NemoVarlenArgs &v, hipStream_t stream, int num_cus, LaunchInfo *info)
{
    if (!v.so || !v.fo || v.n_clips == 0) return hipErrorInvalidValue;
    return launch_n<true>(a, v, stream, num_cus, info);
}

hipError_t launch_nemo_norm(const NemoArgs &a, const NemoVarlenArgs *v, hipStream_t stream)
{
    const unsigned long long n = static_cast<unsigned long long>(v ? v->n_clips : a.batch) * a.n_mels;
    if (n == 0) return hipSuccess;
    if ((n + 255) / 256 > 0x7fffffffull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(ss_nemo_norm_kernel, dim3(static_cast<unsigned>((n + 255) / 256)), dim3(256), 0, stream, a, v ? *v : NemoVarlenArgs{}, v ? 1 : 0);
    return hipGetLastError();
}

}  // namespace ss
