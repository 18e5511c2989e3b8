// ss_nemo_c256 and ss_nemo_norm_kernel: the NeMo / Parakeet log-mel front end (NeMo's FilterbankFeatures as
// transformers.ParakeetFeatureExtractor restates it) for 512-point frames at a 160-sample hop, on gfx950.  The specification is the
// ss_nemo_* comment of include/speechsauce_amd.h; the reference crate has no such path, so this file restates nothing of it.
//
// The quad skeleton (a QUAD of 4 consecutive rows of the flat row list per wave, 16 lanes per frame, persistent 12-wave
// workgroups, the two radix-16 passes and the untangle) is ss_quad256.h; the table block is ss::NemoTables (nemo512_layout).  Zero
// padding behind the window is compile-time (template NE, as in ss_kaldi_c256).  What is this file's own:
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
#include "ss_device.h"
#include "ss_fft_reg.h"
#include "ss_internal.h"
#include "ss_quad256.h"
#include "ss_wave.h"

namespace ss {

namespace {

using namespace wv;
using namespace q256;  // the slot holds, after the exchange, P row [260] | ln(mel) row [128]

namespace L = nemo512_layout;
constexpr int kPRowX = 260;  // bins 0..256 + three zero pad bins
constexpr int kHop = static_cast<int>(kNemoHop);
constexpr float kLn2 = 0.69314718055994530942f;

struct NClip {
    long long s0, f0;
    int len;
    unsigned T;
    bool ok;
};
// clip b of a packed launch: ok = rows fo[b] .. fo[b+1] are exactly the T_b = len / 160 frames `so` implies, inside the output block
__device__ __forceinline__ NClip nemo_clip(const NemoVarlenArgs &v, unsigned b)
{
    NClip c;
    c.s0 = v.so[b];
    c.f0 = v.fo[b];
    const long long len = v.so[b + 1] - c.s0, f1 = v.fo[b + 1];
    const bool len_ok = len >= 0 && len <= 0x7fffffffll;
    c.len = len_ok ? static_cast<int>(len) : 0;
    c.T = static_cast<unsigned>(c.len) / kHop;
    c.ok = len_ok && c.s0 >= 0 && c.f0 >= 0 && f1 - c.f0 == static_cast<long long>(c.T) && static_cast<unsigned long long>(f1) <= v.total_frames;
    return c;
}

// A lane group's frame: the clip's first sample, where in the clip the frame's first live sample lies (negative for the first
// frames), the clip's length, and whether the row exists.
struct Frame {
    const float *base;
    int s0, len;
    bool ok;
};
// Dense: lanes past the last row redo it.  VARLEN: `cursor` is the wave's clip of its last quad's first row (claims only increase).
template <bool VARLEN>
__device__ __forceinline__ Frame frame_of(const NemoArgs &a, const NemoVarlenArgs &v, unsigned quad, unsigned total, int f, unsigned &cursor)
{
    const unsigned q4 = quad * 4;                                           // uniform
    const unsigned g = q4 + min(static_cast<unsigned>(f), total - 1 - q4);  // lanes past the last row redo it
    const int half = static_cast<int>(a.win_len >> 1);
    Frame fr;
    if constexpr (VARLEN) {
        const unsigned c = row_owner(v.fo, v.n_clips, q4, g, cursor);
        const NClip cl = nemo_clip(v, c);
        const long long tl = static_cast<long long>(g) - cl.f0;
        fr.ok = cl.ok && tl >= 0 && tl < static_cast<long long>(cl.T);
        fr.base = a.x + (fr.ok ? cl.s0 : 0ll);
        fr.len = fr.ok ? cl.len : 0;
        fr.s0 = fr.ok ? static_cast<int>(tl) * kHop - half : 0;  // (t * 160 < len < 2^31)
    } else {
        unsigned clip, t;
        locate_frame(q4, g - q4, a.n_frames, a.nf_magic, a.nf_shift, clip, t);
        fr.ok = true;
        fr.base = a.x + static_cast<unsigned long long>(clip) * a.ld;
        fr.len = static_cast<int>(a.n_samples);
        fr.s0 = static_cast<int>(t) * kHop - half;
    }
    return fr;
}

// Issues the loads of one quad: vin[e] = (x[s0 + 2n], x[s0 + 2n + 1]), n = j + 16 e, of this lane group's frame; zero outside the
// clip, beyond the window (W is even: no half pair) and for a row that does not exist.  W > 32 * (NE - 3): the pairs e < NE - 3 of
// every lane lie inside the window, only the last three are tested against it.
// pred: the clip's sample in front of the frame's first live one (lane 0; 0 at or before the clip's start).
// lim: position p of the frame lies in front of the clip's end iff p < lim (any value >= 512 says "all of them"); 0 for a row that
// does not exist, at least 1 for one that does (160 t < len).
// edge (uniform): some frame of the quad does not lie wholly inside its clip -- the per-sample path ran, the consumer clears.
template <int NE>
__device__ __forceinline__ void load_quad_n(const Frame &fr, int W, int j, float2 (&vin)[NE], float &pred, int &lim, bool &edge)
{
#pragma unroll
    for (int e = 0; e < NE; ++e) vin[e] = make_float2(0.f, 0.f);
    pred = 0.f;
    lim = fr.ok ? static_cast<int>(min(static_cast<long long>(fr.len) - fr.s0, 1024ll)) : 0;
    const bool interior = __all(fr.ok && fr.s0 >= 0 && lim >= W);  // uniform
    edge = !interior;
    if (fr.ok && j == 0 && fr.s0 >= 1) pred = fr.base[fr.s0 - 1];
    if (interior) {
        const float *src = fr.base + fr.s0;
        const bool pairs = __all((reinterpret_cast<uintptr_t>(src) & 7u) == 0u);  // uniform: the four frame starts are all 8-byte aligned
        if (pairs) {
            const float2 *p = reinterpret_cast<const float2 *>(src) + j;
#pragma unroll
            for (int e = 0; e < NE; ++e)
                if (e < NE - 3 || 2 * (j + 16 * e) < W) vin[e] = p[16 * e];
        } else {
            const float *p = src + 2 * j;
#pragma unroll
            for (int e = 0; e < NE; ++e)
                if (e < NE - 3 || 2 * (j + 16 * e) < W) vin[e] = make_float2(p[32 * e], p[32 * e + 1]);
        }
    } else if (fr.ok) {
#pragma unroll
        for (int e = 0; e < NE; ++e) {
            const int n2 = 2 * (j + 16 * e), q = fr.s0 + n2;  // the pair's position in the frame and in the clip
            const bool live = e < NE - 3 || n2 < W;
            if (live && q >= 0 && n2 < lim) vin[e].x = fr.base[q];
            if (live && q + 1 >= 0 && n2 + 1 < lim) vin[e].y = fr.base[q + 1];
        }
    }
}

template <int NE, bool VARLEN, int WAVES>
__global__ __launch_bounds__(WAVES * 64) void ss_nemo_c256(const NemoArgs a, const NemoVarlenArgs vl)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x;
    const int wave = tid >> 6;
    const int lane = tid & 63;
    const int f = lane >> 4;  // frame within the quad
    const int j = lane & 15;  // lane within the frame (DPP row)

    float *slot = reinterpret_cast<float *>(smem) + wave * kWaveFloats + f * kSlotFloats;
    float2 *zh = reinterpret_cast<float2 *>(slot);
    float *s_tab = reinterpret_cast<float *>(smem) + WAVES * kWaveFloats;
    const float4 *s_tw2 = reinterpret_cast<const float4 *>(s_tab + L::kTw2);
    const float2 *s_twn = reinterpret_cast<const float2 *>(s_tab + L::kTwn);
    const float2 *s_win = reinterpret_cast<const float2 *>(s_tab + L::kWin);  // 256 window sample pairs (zero beyond W)
    const int *s_start = reinterpret_cast<const int *>(s_tab + L::kStart);
    const int *s_filt = reinterpret_cast<const int *>(s_tab + L::kFilt);
    const float *s_melw = s_tab + L::kMelW;
    unsigned *s_next = reinterpret_cast<unsigned *>(s_tab + L::kMelW + 16 * a.mel_wpitch);

    const unsigned total = VARLEN ? static_cast<unsigned>(vl.total_frames) : a.batch * a.n_frames;
    const unsigned quads = (total + 3) / 4;
    const unsigned q_lo = static_cast<unsigned>(static_cast<unsigned long long>(quads) * blockIdx.x / gridDim.x);
    const unsigned q_hi = static_cast<unsigned>(static_cast<unsigned long long>(quads) * (blockIdx.x + 1) / gridDim.x);
    stage_tables(s_tab, a.tab, (L::kMelW + 16 * a.mel_wpitch) / 4, tid, WAVES * 64);
    if (tid == 0) *s_next = q_lo + WAVES;
    if constexpr (VARLEN) {
        // one pass over the clips, spread over the grid: an inconsistent clip raises the error word (a vector store to the pinned word)
        bool bad = false;
        for (unsigned b = blockIdx.x * (WAVES * 64) + tid; b < vl.n_clips; b += gridDim.x * (WAVES * 64)) bad |= !nemo_clip(vl, b).ok;
        if (bad && vl.err) __hip_atomic_store(vl.err, kVarlenError, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    unsigned quad = __builtin_amdgcn_readfirstlane(q_lo + wave);  // uniform: kept scalar
    unsigned cursor = 0;
    if constexpr (VARLEN) {
        if (quad < q_hi) cursor = offset_find(vl.fo, vl.n_clips, static_cast<long long>(quad) * 4);
    }
    const int W = static_cast<int>(a.win_len);
    float2 vin[NE];
    float pred_next = 0.f;
    int lim_next = 0;
    bool edge_next = false;
    if (quad < q_hi) {
        const Frame fr = frame_of<VARLEN>(a, vl, quad, total, f, cursor);
        load_quad_n<NE>(fr, W, j, vin, pred_next, lim_next, edge_next);
    }

    const int paddr = partner_addr(lane, j), wbase1 = exchange_write_base(j);
    const int M = static_cast<int>(a.n_mels);
    __syncthreads();
    const float4 *w4 = reinterpret_cast<const float4 *>(s_melw + j * a.mel_wpitch);

    while (quad < q_hi) {
        const unsigned next = claim_next(s_next, lane);
        const bool edge_cur = edge_next;
        const float pred_cur = pred_next;
        const int lim_cur = lim_next;

        // ---- steps 2 and 3 of the specification on the input registers ----
        float2 v[16];
        {
            // every product and sum of this stage is rounded on its own (the fused ones are written as fmaf): the bits do not
            // depend on what the compiler finds next to them in a particular build
#pragma clang fp contract(off)
            float2 s[NE];
#pragma unroll
            for (int e = 0; e < NE; ++e) s[e] = vin[e];
            if (a.preemph != 0.f) {
                const float nc = -a.preemph;
                float left = pred_cur;  // lane 0: the clip's own sample in front of the frame, then lane 15's pair e - 1
#pragma unroll
                for (int e = 0; e < NE; ++e) {
                    // x[2n - 1] is the .y of the lane to the left, same register (row_ror:1; lane 0 gets lane 15's: its pair e + 1)
                    const float up = dpp<0x121>(s[e].y);
                    const float prev = j == 0 ? left : up;
                    left = up;
                    s[e] = make_float2(fmaf(nc, prev, s[e].x), fmaf(nc, s[e].x, s[e].y));
                }
                if (edge_cur) {
                    // y is zero at and beyond the clip's end: the pre-emphasis left -c x[len - 1] at position len
#pragma unroll
                    for (int e = 0; e < NE; ++e) {
                        const int n2 = 2 * (j + 16 * e);
                        s[e] = make_float2(n2 < lim_cur ? s[e].x : 0.f, n2 + 1 < lim_cur ? s[e].y : 0.f);
                    }
                }
            }
            // window (zero beyond W: also clears what the pre-emphasis left in the first pad sample)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                if (e < NE) {
                    const float2 w = s_win[j + 16 * e];
                    v[e] = make_float2(__fmul_rn(s[e].x, w.x), __fmul_rn(s[e].y, w.y));
                } else {
                    v[e] = make_float2(0.f, 0.f);
                }
            }
        }
        // ---- 256-point complex FFT of the packed frame; the next quad's samples go into the dead input registers ----
        pass1(v, zh, wbase1);
        if (next < q_hi) {
            const Frame fr = frame_of<VARLEN>(a, vl, next, total, f, cursor);
            load_quad_n<NE>(fr, W, j, vin, pred_next, lim_next, edge_next);
        }
        float2 u[16];
        pass2(u, zh, j, s_tw2);

        // ---- untangle Z -> 2X; |2X|^2 into the P row ----
        // (the untangle twiddles and the slots' first bins are fetched where they are used: next to the prefetched quad and its
        // clip bookkeeping the 168 registers of a 12-wave workgroup do not hold them across the loop)
        float2 zcs[8];
        fetch_partners(u, paddr, zcs);
        float *prow = slot;
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const Bin b = untangle(u, zcs, s_twn[r * 16 + j], j, r);  // exp(-2 pi i (j + 16 r) / 512)
            const float xb_r = fmaf(2.f, b.s.x, -b.xr), xb_i = fmaf(2.f, b.s.y, -b.xi);  // 2 conj X[256-k]
            prow[j + 16 * r] = fmaf(b.xr, b.xr, b.xi * b.xi);
            prow[256 - j - 16 * r] = fmaf(xb_r, xb_r, xb_i * xb_i);  // (bin 256, the Nyquist bin, has weight 0 in the bank)
        }
        if (j == 0) {
            // lane 0's pair k = 0 produced X[0] and X[256]; X[128] = conj Z[128] is the one extra bin
            const float2 z = u[8];
            prow[128] = 4.f * fmaf(z.x, z.x, z.y * z.y);
        }
        if (j < 3) prow[257 + j] = 0.f;  // pad bins read (with zero weight) by the mel stage
        wave_order();

        // ---- banded mel (step 5), guard and ln (step 6): the 1/4 of |2X|^2 rides on the sum ----
        {
            float *frow = slot + kPRowX;
            float m[L::kSlots];
            int st[L::kSlots];
#pragma unroll
            for (int k = 0; k < L::kSlots; ++k) st[k] = s_start[k * 16 + j];
            mel_raw_sums(w4, prow, st, a.mel_q4, m);
#pragma unroll
            for (int k = 0; k < L::kSlots; ++k) {
                const int col = s_filt[k * 16 + j];  // (fetched again: eight registers the loader needs more than this does)
                if (col >= 0) frow[col] = __builtin_amdgcn_logf(fmaf(0.25f, m[k], a.log_guard)) * kLn2;
            }
            wave_order();
            const unsigned gf = quad * 4 + f;
            if (gf < total && lim_cur > 0) {  // (a row that exists has lim >= 1: its frame starts in front of the clip's end)
                float *row = a.out + static_cast<unsigned long long>(gf) * M;
                for (int c = j; c < M; c += 16) row[c] = frow[c];  // 64 consecutive bytes per frame and store
            }
        }
        wave_order();
        quad = next;
    }
}

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
