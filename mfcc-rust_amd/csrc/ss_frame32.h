// The frame stages shared by ss_mfcc_c512 and ss_mel_c512 (ss_mfcc1024.hip), ss_mfcc_c1024 (ss_mfcc2048.hip) and ss_mel_c2048
// (ss_mfcc4096.hip); load_window also serves ss_mel_c256 (ss_mel512.hip).  One iteration of a kernel's persistent loop is
//     claim_next | load_frame or load_window | apply_window | the kernel's FFT | untangle_bin (ss_wave.h) per register |
//     mel_ln_rows | store_mfe_energy, or the kernel's sum / difference rows + dct_dot
// after split_and_stage.  Deliberately not here: ss_mfcc512.hip, ss_mel2048.hip and ss_mfcc_c2048 (the benchmark kernels) with
// the 1024- and 2048-point FFTs that ss_mfcc_c1024 and ss_mel_c2048 share with them by text; the DCT's sum / difference rows (as
// a function their ds_write2st64_b32 pairs split: 6 paired stores become 8 single ones); the 512-point FFT, twice in
// ss_mfcc1024.hip (as one function its complex multiplies contract the other way round: a third of the outputs move by one ulp).
#pragma once

#include "ss_wave.h"

namespace ss {
namespace fr32 {
using namespace wv;

// The workgroup's balanced share [lo, hi) of the launch's units (frame pairs, row pairs or rows), the table block (n4 float4s) into
// LDS and the work counter behind the share's first round; ends in the workgroup barrier.
struct UnitRange { unsigned lo, hi; };
__device__ __forceinline__ UnitRange split_and_stage(unsigned long long units, float *s_tab, const float *tab, int n4, unsigned *s_next, int tid, int waves)
{
    const UnitRange u{static_cast<unsigned>(units * blockIdx.x / gridDim.x), static_cast<unsigned>(units * (blockIdx.x + 1) / gridDim.x)};
    stage_tables(s_tab, tab, n4, tid, waves * 64);
    if (tid == 0) *s_next = u.lo + waves;
    __syncthreads();
    return u;
}

// The MFCC frame that starts at sample s0 of clip xc, zero-padded to 64 NE samples: lane jj of the frame's 32 takes the sample pairs
// n = jj + 32 e.  Contract frames (stack_frames, processing.rs:65-129) and the centred frames inside the clip load whole pairs from
// their (even) start; LIB builds (librosa center=True) mirror (np.pad 'reflect') or zero the missing samples of the few frames at the
// clip edges, per sample.  pre: fused pre-emphasis (processing.rs:31-53) of the samples that exist, tap shift psh -- a run-time flag
// (a uniform branch) or a build's constant, as the kernel has it.
template <int NE, bool LIB, class Args>
__device__ __forceinline__ void load_frame(float2 (&v)[NE], const Args &a, const float *xc, int s0, int jj, bool pre, unsigned psh)
{
    const int flen = static_cast<int>(a.flen), ns = static_cast<int>(a.n_samples);
    // valid sample pairs of this lane: 2 n < flen (zero pad to fft_points, processing.rs:147-156)
    const int half_pairs = flen / 2;
    const int e_hi = min(NE, max(0, (half_pairs - jj + 31) >> 5));
    const bool odd_tail = (a.flen & 1) != 0;
    if (!LIB || __all(s0 >= 0 && s0 + flen <= ns)) {
        const float2 *src = reinterpret_cast<const float2 *>(xc + s0) + jj;
#pragma unroll
        for (int e = 0; e < NE; ++e) {
            float2 s = make_float2(0.f, 0.f);
            if (e < e_hi) s = src[32 * e];
            // odd frame length: the last sample is the first half of a pair (its partner is zero padding)
            if (odd_tail && jj + 32 * e == half_pairs) s = make_float2(xc[s0 + 2 * half_pairs], 0.f);
            if (pre) {
                const int pos = s0 + 2 * (jj + 32 * e), rem = flen - 2 * (jj + 32 * e);
                if (rem >= 1) s.x = fmaf(-a.preemph, preemph_tap(xc, pos, psh, a.n_samples), s.x);
                if (rem >= 2) s.y = fmaf(-a.preemph, preemph_tap(xc, pos + 1, psh, a.n_samples), s.y);
            }
            v[e] = s;
        }
    } else {
#pragma unroll
        for (int e = 0; e < NE; ++e) {
            float sv[2] = {0.f, 0.f};
#pragma unroll
            for (int hh = 0; hh < 2; ++hh) {
                int pos = s0 + 2 * (jj + 32 * e) + hh;
                bool ok = 2 * (jj + 32 * e) + hh < flen;  // zero pad; an odd frame length ends in a half pair
                if (pos < 0 || pos >= ns) {
                    if (a.pad_reflect) pos = pos < 0 ? -pos : 2 * (ns - 1) - pos;
                    else ok = false;
                }
                if (ok) sv[hh] = pre ? fmaf(-a.preemph, preemph_tap(xc, pos, psh, a.n_samples), xc[pos]) : xc[pos];
            }
            v[e] = make_float2(sv[0], sv[1]);
        }
    }
}

// v *= the window pairs of lane jl of LANES (the table's [NE][LANES] float2)
template <int NE, int LANES = 32>
__device__ __forceinline__ void apply_window(float2 (&v)[NE], const float2 *s_win, int jl)
{
#pragma unroll
    for (int e = 0; e < NE; ++e) {
        const float2 w = s_win[jl + LANES * e];
        v[e] = make_float2(v[e].x * w.x, v[e].y * w.y);
    }
}

// The mel / STFT window of 2 NE LANES samples that starts at sample `start` (may be negative) of clip xc, n samples long: lane jl
// of LANES takes the pairs jl + LANES e.  whole (uniform): the window lies inside the clip, constant offsets.  Otherwise zero
// initial state, zero tail and inactive rows (all zero, D3): with start and n even a pair is inside or outside as a whole and the
// valid pairs form one range [e_lo, e_hi) per lane (the address of a masked load may lie outside the clip; it is never
// dereferenced); with an odd hop or clip length a pair may straddle the clip edge, bounds per sample.
template <int NE, int LANES>
__device__ __forceinline__ void load_window(float2 (&v)[NE], const float *xc, int start, int n, int jl, bool active, bool whole)
{
    constexpr int SH = LANES == 16 ? 5 : LANES == 32 ? 6 : 7;  // a lane's pairs lie 2 LANES = 2^SH samples apart
    static_assert(2 * LANES == 1 << SH, "16, 32 or 64 lanes per window");
    const float2 *src = reinterpret_cast<const float2 *>(xc + start) + jl;
    if (whole) {
#pragma unroll
        for (int e = 0; e < NE; ++e) v[e] = src[LANES * e];
        return;
    }
    const int base = start + 2 * jl;
    if (((start | n) & 1) == 0) {
        const int e_lo = base >= 0 ? 0 : ((1 << SH) - 1 - base) >> SH;
        int e_hi = base >= n ? 0 : min(NE, (n - base + (1 << SH) - 1) >> SH);
        if (!active) e_hi = 0;
#pragma unroll
        for (int e = 0; e < NE; ++e) {
            float2 s = make_float2(0.f, 0.f);
            if (e >= e_lo && e < e_hi) s = src[LANES * e];
            v[e] = s;
        }
    } else {
#pragma unroll
        for (int e = 0; e < NE; ++e) {
            const int p0 = base + (e << SH);
            v[e] = make_float2(active && p0 >= 0 && p0 < n ? xc[p0] : 0.f, active && p0 + 1 >= 0 && p0 + 1 < n ? xc[p0 + 1] : 0.f);
        }
    }
}

// Banded mel reduction of a lane's four slots over the P row (feature.rs:229), scale (hscale32 carries 2^32, see ln_scaled), zero
// handling (:230); then either the mfe store into the frame's output row (MFE; nothing for a dead frame) or ln (:105) into the
// filter-order row frow.
template <bool MFE>
__device__ __forceinline__ void mel_ln_rows(const float4 *w4, const float *prow, const int (&st)[4], const int (&fi)[4], const int32_t *q4, float hscale32,
                                            float *frow, float *out_row, bool live)
{
    int off = 0;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        float m = hscale32 * mel_slot4(w4 + off, reinterpret_cast<const float4 *>(prow + st[s]), q4[s]);
        m = m == 0.f ? kEps * kTwo32 : m;
        if (fi[s] >= 0) {
            if (MFE) {
                if (live) out_row[fi[s]] = m * (1.0f / kTwo32);  // exact: power of two
            } else {
                frow[fi[s]] = ln_scaled(m);
            }
        }
        off += q4[s];
    }
}

// the mfe epilogue: the frame energy (handed over times 2^32), by the frame's first lane
__device__ __forceinline__ void store_mfe_energy(float *out_energy, unsigned gf, float energy32, int jj, bool live)
{
    if (jj == 0 && live) out_energy[gf] = energy32 * (1.0f / kTwo32);
}

// DCT-II (feature.rs:120-123) with the m <-> M-1-m symmetry of the cosine, cos(pi c (2(M-1-m)+1) / 2M) = (-1)^c cos(pi c (2m+1) / 2M):
// the kernels form the sum and difference rows of ln(mel) once per frame (their own text, see above); even coefficients then take
// a (M+1)/2-term product with the sum row, odd ones with the difference row.  One coefficient: nq float4s of its row against its
// cosine row.
__device__ __forceinline__ float dct_dot(const float4 *r4, const float4 *c4, int nq)
{
    float acc = 0.f;
    for (int i = 0; i < nq; ++i) {
        const float4 r = r4[i], cw = c4[i];
        acc = fmaf(r.x, cw.x, acc);
        acc = fmaf(r.y, cw.y, acc);
        acc = fmaf(r.z, cw.z, acc);
        acc = fmaf(r.w, cw.w, acc);
    }
    return acc;
}

}  // namespace fr32
}  // namespace ss
