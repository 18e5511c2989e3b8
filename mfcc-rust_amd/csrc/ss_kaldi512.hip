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
#include "ss_device.h"
#include "ss_fft_reg.h"
#include "ss_internal.h"
#include "ss_quad256.h"
#include "ss_wave.h"

namespace ss {

namespace {

using namespace wv;
using namespace q256;  // the slot holds, after the exchange, P row [260] | ln(mel) row [80]

namespace L = mfcc512w_layout;
constexpr int kPRowX = 260;            // bins 0..256 + three zero pad bins
constexpr float kLn2 = 0.69314718055994530942f;

// ln(max(v, eps)): eps = 2^-23 is a normal number, v_log_f32 needs no denormal care
__device__ __forceinline__ float ln_floored(float v) { return __builtin_amdgcn_logf(fmaxf(v, kEps)) * kLn2; }

__device__ __forceinline__ unsigned kaldi_frames_dev(uint32_t flen, uint32_t step, long long len)
{
    if (len < static_cast<long long>(flen) || len > 0x7fffffffll) return 0u;
    return 1u + (static_cast<unsigned>(len) - flen) / step;
}

struct KClip {
    long long s0, f0;
    unsigned T;
    bool ok;
};
// clip b of a packed launch: ok = rows fo[b] .. fo[b+1] are exactly the T_b frames `so` implies, inside the output block
__device__ __forceinline__ KClip kaldi_clip(const KaldiVarlenArgs &v, uint32_t flen, uint32_t step, unsigned b)
{
    KClip c;
    c.s0 = v.so[b];
    c.f0 = v.fo[b];
    const long long s1 = v.so[b + 1], f1 = v.fo[b + 1];
    c.T = kaldi_frames_dev(flen, step, s1 - c.s0);
    c.ok = c.T > 0u && c.s0 >= 0 && c.f0 >= 0 && f1 - c.f0 == static_cast<long long>(c.T) && static_cast<unsigned long long>(f1) <= v.total_frames;
    return c;
}

// Where this lane group's frame starts and whether it exists.  Dense: lanes past the last frame redo it.  VARLEN: `cursor` is the
// wave's clip of its last quad's first row (claims only increase); a lane's frame lies at most three clips WITH rows further on.
template <bool VARLEN>
__device__ __forceinline__ const float *frame_src(const KaldiArgs &a, const KaldiVarlenArgs &v, unsigned quad, unsigned total, int f, unsigned &cursor, bool &ok)
{
    const unsigned q4 = quad * 4;                                           // uniform
    const unsigned g = q4 + min(static_cast<unsigned>(f), total - 1 - q4);  // lanes past the last row redo it
    if constexpr (VARLEN) {
        unsigned c = offset_seek(v.fo, v.n_clips, cursor, q4);
        cursor = c;
        bool step = true;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            step = c + 1 < v.n_clips && v.fo[c + 1] <= static_cast<long long>(g);
            c += step ? 1u : 0u;
        }
        // entries without rows inside the quad (fo[b] == fo[b + 1]) take steps of their own: a lane that took all three looks once
        // more, and searches where they did not get there
        if (step && c + 1 < v.n_clips && v.fo[c + 1] <= static_cast<long long>(g)) c = offset_find(v.fo, v.n_clips, static_cast<long long>(g));
        const KClip cl = kaldi_clip(v, a.flen, a.step, c);
        const long long tl = static_cast<long long>(g) - cl.f0;
        ok = cl.ok && tl >= 0 && tl < static_cast<long long>(cl.T);
        return a.x + (ok ? cl.s0 + tl * static_cast<long long>(a.step) : 0ll);
    } else {
        unsigned clip, t;
        locate_frame(q4, g - q4, a.n_frames, a.nf_magic, a.nf_shift, clip, t);
        ok = true;
        return a.x + static_cast<unsigned long long>(clip) * a.ld + static_cast<unsigned long long>(t) * a.step;
    }
}

// Issues the loads of one quad: vin[e] = (x[2n], x[2n+1]), n = j + 16 e, of this lane group's frame; zero beyond flen (an odd frame
// length ends in a half pair) and for a frame that does not exist.
// flen > 32 * (NE - 3): the pairs e < NE - 3 of every lane lie inside the frame, only the last three are tested.
template <int NE, bool VARLEN>
__device__ __forceinline__ void load_quad_k(const float *src, bool ok, uint32_t flen, int j, float2 (&vin)[NE])
{
    const bool pair_ok = (reinterpret_cast<uintptr_t>(src) & 7u) == 0u;
    const bool pairs = __all(pair_ok);  // uniform: the quad's four frame starts are all 8-byte aligned
#pragma unroll
    for (int e = 0; e < NE; ++e) vin[e] = make_float2(0.f, 0.f);
    if (VARLEN && !ok) return;
    if (pairs) {
        const float2 *p = reinterpret_cast<const float2 *>(src) + j;
#pragma unroll
        for (int e = 0; e < NE; ++e) {
            if (e < NE - 3) {
                vin[e] = p[16 * e];
            } else {
                const int rem = static_cast<int>(flen) - 2 * (j + 16 * e);
                if (rem >= 2) vin[e] = p[16 * e];
                else if (rem == 1) vin[e].x = reinterpret_cast<const float *>(p)[32 * e];
            }
        }
    } else {
        const float *p = src + 2 * j;
#pragma unroll
        for (int e = 0; e < NE; ++e) {
            if (e < NE - 3) {
                vin[e] = make_float2(p[32 * e], p[32 * e + 1]);
            } else {
                const int rem = static_cast<int>(flen) - 2 * (j + 16 * e);
                if (rem >= 1) vin[e].x = p[32 * e];
                if (rem >= 2) vin[e].y = p[32 * e + 1];
            }
        }
    }
}

template <int NE, bool POW2, bool MFCC, bool VARLEN, int WAVES>
__global__ __launch_bounds__(WAVES * 64) void ss_kaldi_c256(const KaldiArgs a, const KaldiVarlenArgs vl)
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
    const float *s_cos = s_tab + L::kCos;
    const int *s_start = reinterpret_cast<const int *>(s_tab + L::kStart);
    const int *s_filt = reinterpret_cast<const int *>(s_tab + L::kFilt);
    const float *s_melw = s_tab + L::kMelW;
    const float2 *s_win = reinterpret_cast<const float2 *>(s_tab + L::kMelW + 16 * a.mel_wpitch);  // 256 window sample pairs (zero beyond flen)
    unsigned *s_next = reinterpret_cast<unsigned *>(s_tab + L::kMelW + 16 * a.mel_wpitch + 512);

    const unsigned total = VARLEN ? static_cast<unsigned>(vl.total_frames) : a.batch * a.n_frames;
    const unsigned quads = (total + 3) / 4;
    const unsigned q_lo = static_cast<unsigned>(static_cast<unsigned long long>(quads) * blockIdx.x / gridDim.x);
    const unsigned q_hi = static_cast<unsigned>(static_cast<unsigned long long>(quads) * (blockIdx.x + 1) / gridDim.x);
    stage_tables(s_tab, a.tab, (L::kMelW + 16 * a.mel_wpitch + 512) / 4, tid, WAVES * 64);
    if (tid == 0) *s_next = q_lo + WAVES;
    if constexpr (VARLEN) {
        // one pass over the clips, spread over the grid: an inconsistent clip raises the error word (a vector store to the pinned word)
        bool bad = false;
        for (unsigned b = blockIdx.x * (WAVES * 64) + tid; b < vl.n_clips; b += gridDim.x * (WAVES * 64)) bad |= !kaldi_clip(vl, a.flen, a.step, b).ok;
        if (bad && vl.err) __hip_atomic_store(vl.err, kVarlenError, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    unsigned quad = __builtin_amdgcn_readfirstlane(q_lo + wave);  // uniform: kept scalar
    unsigned cursor = 0;
    if (VARLEN && quad < q_hi) cursor = offset_find(vl.fo, vl.n_clips, static_cast<long long>(quad) * 4);
    float2 vin[NE];
    bool ok_next = false;
    if (quad < q_hi) {
        const float *src = frame_src<VARLEN>(a, vl, quad, total, f, cursor, ok_next);
        load_quad_k<NE, VARLEN>(src, ok_next, a.flen, j, vin);
    }

    const int paddr = partner_addr(lane, j), wbase1 = exchange_write_base(j);
    const int Cc = static_cast<int>(a.n_ceps), M = static_cast<int>(a.n_filters);
    // the P row holds |2X|^2 or |2X|: the 1/4 or 1/2 of the untangle rides on the mel sums
    const float hscale = POW2 ? 0.25f : 0.5f;
    const int flen = static_cast<int>(a.flen);
    __syncthreads();
    int st[5], fi[5];
#pragma unroll
    for (int s = 0; s < 5; ++s) {
        st[s] = s_start[s * 16 + j];
        fi[s] = s_filt[s * 16 + j];
    }
    const float4 *w4 = reinterpret_cast<const float4 *>(s_melw + j * a.mel_wpitch);
    const float4 *c4 = reinterpret_cast<const float4 *>(s_cos + j * L::kCosPitch);
    float2 twn[8];  // exp(-2 pi i (j + 16 r) / 512) stays in registers
#pragma unroll
    for (int r = 0; r < 8; ++r) twn[r] = s_twn[r * 16 + j];

    while (quad < q_hi) {
        const unsigned next = claim_next(s_next, lane);
        const bool ok_cur = ok_next;

        // ---- conditioning stage (steps 1-5 of the specification) on the input registers ----
        float2 v[16];
        float energy;
        {
            // every product and sum of this stage is rounded on its own (the fused ones are written as fmaf): the bits do not
            // depend on what the compiler finds next to them in a particular build
#pragma clang fp contract(off)
            float2 s[NE];
#pragma unroll
            for (int e = 0; e < NE; ++e) s[e] = vin[e];
            if (a.input_scale != 1.0f) {
#pragma unroll
                for (int e = 0; e < NE; ++e) s[e] = make_float2(__fmul_rn(s[e].x, a.input_scale), __fmul_rn(s[e].y, a.input_scale));
            }
            if (a.remove_dc) {
                float part = 0.f;
#pragma unroll
                for (int e = 0; e < NE; ++e) part = __fadd_rn(part, __fadd_rn(s[e].x, s[e].y));
                const float mean = __fdiv_rn(row16_sum(part), a.flen_f);
#pragma unroll
                for (int e = 0; e < NE; ++e) {
                    float2 d = make_float2(__fsub_rn(s[e].x, mean), __fsub_rn(s[e].y, mean));
                    if (e >= NE - 3) {  // only the last three pairs of a lane can lie beyond flen: the pad stays exactly zero
                        const int rem = flen - 2 * (j + 16 * e);
                        d = make_float2(rem >= 1 ? d.x : 0.f, rem >= 2 ? d.y : 0.f);
                    }
                    s[e] = d;
                }
            }
            float esum = 0.f;
            if (a.raw_energy) {
#pragma unroll
                for (int e = 0; e < NE; ++e) esum = fmaf(s[e].y, s[e].y, fmaf(s[e].x, s[e].x, esum));
            }
            if (a.preemph != 0.f) {
                const float nc = -a.preemph;
                float up[NE];  // the .y of the lane to the left (lane 0: of lane 15), same register
#pragma unroll
                for (int e = 0; e < NE; ++e) up[e] = dpp<0x121>(s[e].y);  // row_ror:1
#pragma unroll
                for (int e = 0; e < NE; ++e) {
                    // s[2n - 1]: lane j - 1's pair e; for lane 0 lane 15's pair e - 1, and the frame's own first sample for s[0]
                    const float prev = j == 0 ? (e == 0 ? s[0].x : up[e > 0 ? e - 1 : 0]) : up[e];
                    s[e] = make_float2(fmaf(nc, prev, s[e].x), fmaf(nc, s[e].x, s[e].y));
                }
            }
            // window (zero beyond flen: also clears what the pre-emphasis left in the first pad sample)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                if (e < NE) {
                    const float2 w = s_win[j + 16 * e];
                    v[e] = make_float2(__fmul_rn(s[e].x, w.x), __fmul_rn(s[e].y, w.y));
                } else {
                    v[e] = make_float2(0.f, 0.f);
                }
            }
            if (!a.raw_energy) {
#pragma unroll
                for (int e = 0; e < NE; ++e) esum = fmaf(v[e].y, v[e].y, fmaf(v[e].x, v[e].x, esum));
            }
            energy = fmaxf(ln_floored(row16_sum(esum)), a.log_floor);  // steps 3 / 5 and 9
        }
        // ---- 256-point complex FFT of the packed frame; the next quad's samples go into the dead input registers ----
        pass1(v, zh, wbase1);
        if (next < q_hi) {
            const float *src = frame_src<VARLEN>(a, vl, next, total, f, cursor, ok_next);
            load_quad_k<NE, VARLEN>(src, ok_next, a.flen, j, vin);
        }
        float2 u[16];
        pass2(u, zh, j, s_tw2);

        // ---- untangle Z -> 2X; |2X|^2 or |2X| into the P row ----
        float2 zcs[8];
        fetch_partners(u, paddr, zcs);
        float *prow = slot;
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const Bin b = untangle(u, zcs, twn[r], j, r);
            const float xb_r = fmaf(2.f, b.s.x, -b.xr), xb_i = fmaf(2.f, b.s.y, -b.xi);  // 2 conj X[256-k]
            const float na = fmaf(b.xr, b.xr, b.xi * b.xi), nb = fmaf(xb_r, xb_r, xb_i * xb_i);
            prow[j + 16 * r] = POW2 ? na : __builtin_amdgcn_sqrtf(na);
            prow[256 - j - 16 * r] = POW2 ? nb : __builtin_amdgcn_sqrtf(nb);  // (bin 256, the Nyquist bin, has no weight in the bank)
        }
        if (j == 0) {
            // lane 0's pair k = 0 produced X[0] and X[256]; X[128] = conj Z[128] is the one extra bin
            const float2 z = u[8];
            const float n = 4.f * fmaf(z.x, z.x, z.y * z.y);
            prow[128] = POW2 ? n : __builtin_amdgcn_sqrtf(n);
        }
        if (j < 3) prow[257 + j] = 0.f;  // pad bins read (with zero weight) by the mel stage
        wave_order();

        // ---- banded mel reduction (step 7), floor and ln (step 8) ----
        {
            float *frow = slot + kPRowX;
            float m[5];
            mel_raw_sums(w4, prow, st, a.mel_q4, m);
#pragma unroll
            for (int k = 0; k < 5; ++k) m[k] = ln_floored(hscale * m[k]);
            const unsigned gf = quad * 4 + f;
            const bool store = gf < total && ok_cur;
            if (!MFCC) {
                if (store) {
                    float *row = a.out + static_cast<unsigned long long>(gf) * M;
#pragma unroll
                    for (int k = 0; k < 5; ++k)
                        if (fi[k] >= 0) row[fi[k]] = m[k];
                    if (j == 0 && a.out_energy) a.out_energy[gf] = energy;
                }
            } else {
#pragma unroll
                for (int k = 0; k < 5; ++k) frow[16 * k + j] = m[k];
                wave_order();
                // ---- DCT with the lifter folded in (step 10): lane c against the 80-entry row; beyond 16 cepstra the lane also
                // forms coefficient 16 + j from the same row fetches.  Five rounds of four float4 pairs: this stage runs next to the prefetch
                // registers (the fully unrolled form spills).
                const float4 *d4 = c4 + 16 * (L::kCosPitch / 4);
                const bool two = Cc > 16;  // uniform
                float acc = 0.f, acc2 = 0.f;
#pragma unroll 2
                for (int h = 0; h < 10; ++h) {
                    float4 lq[2], cq[2], dq[2];
#pragma unroll
                    for (int i = 0; i < 2; ++i) {
                        lq[i] = *reinterpret_cast<const float4 *>(&frow[4 * (2 * h + i)]);
                        cq[i] = c4[2 * h + i];
                        dq[i] = two ? d4[2 * h + i] : make_float4(0.f, 0.f, 0.f, 0.f);
                    }
#pragma unroll
                    for (int i = 0; i < 2; ++i) {
                        acc = fmaf(lq[i].x, cq[i].x, acc);
                        acc = fmaf(lq[i].y, cq[i].y, acc);
                        acc = fmaf(lq[i].z, cq[i].z, acc);
                        acc = fmaf(lq[i].w, cq[i].w, acc);
                        if (two) {
                            acc2 = fmaf(lq[i].x, dq[i].x, acc2);
                            acc2 = fmaf(lq[i].y, dq[i].y, acc2);
                            acc2 = fmaf(lq[i].z, dq[i].z, acc2);
                            acc2 = fmaf(lq[i].w, dq[i].w, acc2);
                        }
                    }
                }
                const float o = (j == 0 && a.use_energy) ? energy : acc;
                if (store) {
                    if (j < Cc) a.out[static_cast<unsigned long long>(gf) * Cc + j] = o;
                    if (16 + j < Cc) a.out[static_cast<unsigned long long>(gf) * Cc + 16 + j] = acc2;
                }
            }
        }
        wave_order();
        quad = next;
    }
}

template <bool VARLEN>
hipError_t launch_k(const KaldiArgs &a_in, const KaldiVarlenArgs &v, hipStream_t stream, int num_cus, LaunchInfo *info)
{
    constexpr int WAVES = 12;
    KaldiArgs a = a_in;
    const unsigned long long total = VARLEN ? v.total_frames : static_cast<unsigned long long>(a.batch) * a.n_frames;
    if (a.flen <= 256 || a.flen > 512 || a.step == 0 || a.n_filters > 80 || a.n_ceps > 32) return hipErrorInvalidValue;
    const size_t lds = (static_cast<size_t>(WAVES) * kWaveFloats + L::kMelW + 16 * static_cast<size_t>(a.mel_wpitch) + 512 + 4) * sizeof(float);
    GroupPlan plan;
    const PlanStatus ps = plan_groups(total, a.n_frames, 4, !VARLEN, lds, WAVES, num_cus, plan);
    if (ps != PlanStatus::Launch) return ps == PlanStatus::Empty ? hipSuccess : hipErrorInvalidValue;
    a.nf_magic = plan.nf_magic;
    a.nf_shift = plan.nf_shift;
    auto go = [&](auto kern, const char *name) { return launch_kernel(kern, name, plan.grid, WAVES, lds, stream, info, a, v); };
    const bool pow2 = a.use_power != 0, mfcc = a.out_mfcc != 0;
#define SS_K(NE, P, C, NAME) go(ss_kaldi_c256<NE, P, C, VARLEN, WAVES>, VARLEN ? NAME ",v>" : NAME ">")
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

}  // namespace ss
