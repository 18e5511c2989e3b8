// ss_mfcc_c512: fused MFCC / mfe for fft_points = 1024 (C = 512 packed complex points) on gfx950 -- the structure of the
// 4096-point kernel (ss_mfcc4096.hip) at a quarter of the size, two frames per wave.
//
//   * 32 lanes own a frame, 16 complex points per lane.  512-point FFT = 16 x 32: a radix-16 register butterfly over n2
//     (n = n1 + 32 n2, n1 = lane), ONE transposing exchange through wave-private LDS, then the 32-point transform over n1
//     split as n1 = a + 2b: lane (k1, a) does a radix-16 butterfly over b, and the last radix-2 over a pairs lanes L and
//     L + 16 with v_permlane16_swap (odd DPP rows of one register trade places with even rows of another: one swap of
//     registers (i, 8 + i) gives the even-row lane both halves' column i and the odd-row lane both halves' column 8 + i).
//     ss_mel_c512 below repeats the transform (one function for both moves output bits: see ss_frame32.h).
//   * real-FFT untangle: lane (k1, h) register r0[i] holds bin k = k1 + 16 i + 128 h (< 256); its partner 512 - k is
//     r1[7 - i] of lane (16 - k1, 1 - h) (r1[8 - i] for the k1 = 0 lanes), fetched with ds_bpermute_b32; untangle_bin (ss_wave.h).
//   * |X|/N: bins 0..256 go to the P row (the mel bank ends at (F+1)/2, feature.rs:69-70), all 513 feed the frame energy.
//   * the stages around the transform are the frame stages of ss_frame32.h, shared with ss_mfcc_c1024 (ss_mfcc2048.hip):
//     load_frame (contract / centred / pre-emphasised frames), apply_window, mel_ln_rows (banded mel, 4 filters per lane,
//     aligned float4 taps; zero handling; ln), store_mfe_energy (mfe build), dct_dot (symmetric DCT-II); the sum /
//     difference rows, reference scaling and column-0 replacement stay here.
//   * 12 waves per CU, frame pairs from an LDS counter; no workgroup barrier in the main loop.
// Reference semantics: feature.rs:99-148 (mfcc), :200-233 (mfe), processing.rs:65-181.  Tables: ss::mfcc1024_layout.
#include "ss_device.h"
#include "ss_fft_reg.h"
#include "ss_frame32.h"
#include "ss_internal.h"
#include "ss_wave.h"

namespace ss {

namespace {

using namespace wv;
using namespace fr32;

namespace L = mfcc1024_layout;
constexpr int kClsK = 8 * 34 + 8;        // float2 per class slice (+8: the two classes of a write group sit 16 banks apart)
constexpr int kFrameF2 = 560;            // float2 per frame region (4480 B = 128 mod 256: the two frames of a wave use different banks)
constexpr int kFrameFloats = 2 * kFrameF2;  // after the exchange: P row [260] | ln(mel) row [128] | s [64] | d [64]
constexpr int kWaveFloatsK = 2 * kFrameFloats;

template <bool POW2, bool MFE, bool WIN, int WAVES, bool LIB = false>
__global__ __launch_bounds__(WAVES * 64) void ss_mfcc_c512(const Mfcc1024Args a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x;
    const int wave = tid >> 6;
    const int lane = tid & 63;
    const int fr = lane >> 5;                 // frame within the wave
    const int jj = lane & 31;                 // lane within the frame
    const int k1 = jj & 15, h = jj >> 4;      // reader view: column k1, half a = h
    const int cls = jj & 1, bw = jj >> 1;     // writer view: n1 = jj = cls + 2 bw

    float *fbase = reinterpret_cast<float *>(smem) + wave * kWaveFloatsK + fr * kFrameFloats;
    float2 *exf = reinterpret_cast<float2 *>(fbase);
    // LIB builds (librosa-compatible switches) keep all 513 bins of the P row: [516] | ln(mel) [128] | s [64] | d [64]
    float *prow = fbase, *frow = fbase + (LIB ? 516 : 260), *srow = frow + 128, *drow = srow + 64;
    float *s_tab = reinterpret_cast<float *>(smem) + WAVES * kWaveFloatsK;
    const float4 *s_t1 = reinterpret_cast<const float4 *>(s_tab + L::kT1);
    const float2 *s_t2 = reinterpret_cast<const float2 *>(s_tab + L::kT2);
    const float2 *s_twn = reinterpret_cast<const float2 *>(s_tab + L::kTwn);
    const float2 *s_win = reinterpret_cast<const float2 *>(s_tab + L::kWin);
    const int *s_start = reinterpret_cast<const int *>(s_tab + L::kStart);
    const int *s_filt = reinterpret_cast<const int *>(s_tab + L::kFilt);
    const float *s_cos = s_tab + L::kCos;
    const float *s_melw = s_tab + L::kMelW;
    unsigned *s_next = reinterpret_cast<unsigned *>(s_tab + L::kMelW + 32 * a.mel_wpitch);

    const unsigned total = a.batch * a.n_frames;
    const UnitRange ur = split_and_stage((total + 1) / 2, s_tab, a.tab, (L::kMelW + 32 * a.mel_wpitch) / 4, s_next, tid, WAVES);
    int st[4], fi[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        st[s] = s_start[s * 32 + jj];
        fi[s] = s_filt[s * 32 + jj];
    }
    const float4 *w4 = reinterpret_cast<const float4 *>(s_melw + jj * a.mel_wpitch);
    const int paddr = ((lane & 32) | ((16 - k1) & 15) | ((1 - h) << 4)) << 2;  // lane holding Z[512 - k]
    float2 *exw = exf + cls * kClsK + 34 * (bw >> 1) + (bw & 1);  // writer base (float2 units)
    const float2 *exr = exf + h * kClsK + 2 * k1;                  // reader base
    const float hscale32 = (POW2 ? 0.25f * a.scale : 0.5f * a.scale) * kTwo32;
    const bool k1z = k1 == 0;
    const int M = static_cast<int>(a.n_filters), Cc = static_cast<int>(a.n_ceps), Mh = M / 2, Mc = (M + 1) / 2, nq = (Mc + 3) / 4;
    const bool pre = a.preemph != 0.f;  // fused pre-emphasis (run-time: a uniform branch in the loader)
    const unsigned psh = a.preemph_shift % a.n_samples;

    unsigned unit = __builtin_amdgcn_readfirstlane(ur.lo + wave);  // uniform: kept scalar
    while (unit < ur.hi) {
        const unsigned next = claim_next(s_next, lane);

        const unsigned gf_raw = 2 * unit + fr;
        const bool live = gf_raw < total;
        const unsigned gf = live ? gf_raw : total - 1;
        const unsigned clip = gf / a.n_frames;
        const unsigned t = gf - clip * a.n_frames;
        // stack_frames (processing.rs:65-129, contract framing): frame t starts at sample t*step; librosa center=True (LIB
        // builds): it is centred on sample t*step
        const float *xc = a.x + static_cast<unsigned long long>(clip) * a.ld;
        const int s0 = static_cast<int>(t * a.step) - (LIB && a.center ? static_cast<int>(a.flen / 2) : 0);
        float2 v[16];
        load_frame<16, LIB>(v, a, xc, s0, jj, pre, psh);
        if (WIN) apply_window<16>(v, s_win, jj);
        // ---- pass 1: radix-16 over n2; transpose (two 16 x 16 problems: even and odd n1) ----
        fft_reg<16>(v);
#pragma unroll
        for (int k = 0; k < 16; ++k) exw[2 * k] = v[k];
        wave_order();
        float2 u[16];
#pragma unroll
        for (int p = 0; p < 8; ++p) {
            const float4 t4 = *reinterpret_cast<const float4 *>(&exr[34 * p]);
            u[2 * p] = make_float2(t4.x, t4.y);
            u[2 * p + 1] = make_float2(t4.z, t4.w);
        }
        wave_order();
        // ---- twiddle W256^(b k1), radix-16 over b ----
#pragma unroll
        for (int p = 0; p < 8; ++p) {
            const float4 w2 = s_t1[p * 16 + k1];
            u[2 * p + 1] = cmul(u[2 * p + 1], make_float2(w2.x, w2.y));
            if (p < 7) u[2 * p + 2] = cmul(u[2 * p + 2], make_float2(w2.z, w2.w));
        }
        fft_reg<16>(u);  // u[c] = G_a[c], a = h
        // ---- radix-2 over a with one row swap per register pair: r0[i] (d = 0) and r1[i] (d = 1) hold
        //      Z[k1 + 16 c + 256 d] = G0[c] + (-1)^d W512^(k1 + 16 c) G1[c],  c = i + 8 h ----
        float2 r0[8], r1[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            float px = u[i].x, qx = u[8 + i].x, py = u[i].y, qy = u[8 + i].y;
            swap_rows(px, qx);
            swap_rows(py, qy);
            const float2 wq = cmul(make_float2(qx, qy), s_t2[i * 32 + jj]);
            r0[i] = make_float2(px + wq.x, py + wq.y);
            r1[i] = make_float2(px - wq.x, py - wq.y);
        }

        // ---- untangle Z -> X; |X| (processing.rs:168) * 1/N (:180); row sum (feature.rs:216) ----
        // the i = 0 pairs of the k1 = 0 lanes are in-lane: (k1, h) = (0, 0) has k = 0 (X[0] and X[512] come from Z[0] alone),
        // (0, 1) has (128, 384) = (r0[0], r1[0]).  Z[256] = r1[0] of (0, 0).
        float esum = 0.f;
        float2 zcs[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const float2 sv = k1z ? r1[(8 - i) & 7] : r1[7 - i];
            zcs[i] = make_float2(bperm(paddr, sv.x), bperm(paddr, sv.y));
        }
        float *pdst = prow + k1 + 128 * h;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const float2 zk = r0[i];
            float2 zc = zcs[i];
            if (i == 0) zc = k1z ? (h ? r1[0] : zk) : zc;
            const Bin b = untangle_bin(zk, zc, s_twn[i * 32 + jj]);
            const float xb_r = fmaf(2.f, b.s.x, -b.xr), xb_i = fmaf(2.f, b.s.y, -b.xi);  // 2 conj X[512-k] = 2 s - 2 X[k]
            const float na = b.xr * b.xr + b.xi * b.xi, nb = xb_r * xb_r + xb_i * xb_i;
            const float pa = POW2 ? na : __builtin_amdgcn_sqrtf(na);
            const float pb = POW2 ? nb : __builtin_amdgcn_sqrtf(nb);
            pdst[16 * i] = pa;  // bins 0..255 (the bank ends at (F+1)/2, feature.rs:69-70); 256 below
            if (LIB) prow[512 - (k1 + 128 * h + 16 * i)] = pb;  // bins 257..512 for banks over the whole spectrum
            esum += pa + pb;
        }
        if (jj == 0) {
            const float2 z = r1[0];  // X[256] = conj Z[256]
            const float n = 4.f * (z.x * z.x + z.y * z.y);
            const float p256 = POW2 ? n : __builtin_amdgcn_sqrtf(n);
            prow[256] = p256;
            esum += p256;
        }
        if (jj < 3) prow[(LIB ? 513 : 257) + jj] = 0.f;  // pad bins read (with zero weight) by the mel stage
        float energy = hscale32 * half_sum(esum);            // E * 2^32
        energy = energy == 0.f ? kEps * kTwo32 : energy;     // zero_handling, feature.rs:219
        wave_order();

        mel_ln_rows<MFE>(w4, prow, st, fi, a.mel_q4, hscale32, frow, a.out + static_cast<unsigned long long>(gf) * M, live);
        if (MFE) {
            store_mfe_energy(a.out_energy, gf, energy, jj, live);
            wave_order();
            unit = next;
            continue;
        }
        wave_order();
        // ---- DCT-II (feature.rs:120-123) with the m <-> M-1-m symmetry of the cosine: sum and difference rows once per frame
        // (the text of ss_mfcc_c1024's: see ss_frame32.h), then a (M+1)/2-term product per coefficient ----
#pragma unroll
        for (int h2 = 0; h2 < 2; ++h2) {
            const int m = jj + 32 * h2;
            if (m < Mh) {
                const float lo = frow[m], hi = frow[M - 1 - m];
                srow[m] = lo + hi;
                drow[m] = lo - hi;
            } else if (m < Mc) {  // odd filter count: the middle filter pairs with itself (its odd-coefficient cosines are zero)
                srow[m] = frow[m];
                drow[m] = 0.f;
            } else if (m < ((Mc + 3) & ~3)) {  // dct_dot runs over whole float4s
                srow[m] = 0.f;
                drow[m] = 0.f;
            }
        }
        wave_order();
        const float4 *r4 = reinterpret_cast<const float4 *>((jj & 1) ? drow : srow);  // coefficients jj and jj + 32: same parity, same row
        if (jj < Cc) {
            const float acc = dct_dot(r4, reinterpret_cast<const float4 *>(s_cos + jj * L::kCosPitch), nq);
            // scaling + column-0 replacement (feature.rs:126-146)
            float o = acc * a.dct_scale_k;
            if (jj == 0) o = a.dc_elimination ? ln_scaled(energy) : acc * (t == 0 ? a.dct_scale_00 : a.dct_scale_0);
            if (live) a.out[static_cast<unsigned long long>(gf) * Cc + jj] = o;
        }
        if (Cc > 32) {  // 33..64 cepstra: the lane also forms coefficient jj + 32
            wave_order();
            if (jj + 32 < Cc) {
                const float acc = dct_dot(r4, reinterpret_cast<const float4 *>(s_cos + (jj + 32) * L::kCosPitch), nq);
                if (live) a.out[static_cast<unsigned long long>(gf) * Cc + jj + 32] = acc * a.dct_scale_k;
            }
        }
        wave_order();
        unit = next;
    }
}

// ss_mel_c512: the mel-spectrogram path (frame_analysis + |X wnorm|^2 + mel einsum, functions.rs:125-170, feature.rs:151-174)
// at fft_points = 1024 on the same FFT mapping: 32 lanes own a 1024-sample window, a wave carries two consecutive rows of
// one clip, the work unit is a (clip, row pair).  Row r covers the 1024 samples that end at chunk r + n_pad: zero initial
// state, zero tail, rows past the real ones all zero (D3) -- load_window of ss_frame32.h.  The table block is
// mfcc1024_layout with the Vorbis window in kWin (kCos unused).
template <int WAVES, bool STFT>
__global__ __launch_bounds__(WAVES * 64) void ss_mel_c512(const Mel2048Args a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x;
    const int wave = tid >> 6;
    const int lane = tid & 63;
    const int fr = lane >> 5;                 // row within the pair
    const int jj = lane & 31;                 // lane within the row
    const int k1 = jj & 15, h = jj >> 4;      // reader view: column k1, half a = h
    const int cls = jj & 1, bw = jj >> 1;     // writer view: n1 = jj = cls + 2 bw

    float *fbase = reinterpret_cast<float *>(smem) + wave * kWaveFloatsK + fr * kFrameFloats;
    float2 *exf = reinterpret_cast<float2 *>(fbase);
    float *prow = fbase;  // [516] after the exchange
    float *s_tab = reinterpret_cast<float *>(smem) + WAVES * kWaveFloatsK;
    const float4 *s_t1 = reinterpret_cast<const float4 *>(s_tab + L::kT1);
    const float2 *s_t2 = reinterpret_cast<const float2 *>(s_tab + L::kT2);
    const float2 *s_twn = reinterpret_cast<const float2 *>(s_tab + L::kTwn);
    const float2 *s_win = reinterpret_cast<const float2 *>(s_tab + L::kWin);
    const int *s_start = reinterpret_cast<const int *>(s_tab + L::kStart);
    const int *s_filt = reinterpret_cast<const int *>(s_tab + L::kFilt);
    const float *s_melw = s_tab + L::kMelW;
    unsigned *s_next = reinterpret_cast<unsigned *>(s_tab + L::kMelW + 32 * a.mel_wpitch);

    const int R = static_cast<int>(a.rows), Rreal = static_cast<int>(a.real_rows), M = static_cast<int>(a.n_filters);
    const unsigned pairs = (a.rows + 1) / 2;
    const unsigned long long units = static_cast<unsigned long long>(a.batch) * pairs;
    const UnitRange ur = split_and_stage(units, s_tab, a.tab, (L::kMelW + 32 * a.mel_wpitch) / 4, s_next, tid, WAVES);
    int st[4], fi[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        st[s] = s_start[s * 32 + jj];
        fi[s] = s_filt[s * 32 + jj];
    }
    const float4 *w4 = reinterpret_cast<const float4 *>(s_melw + jj * a.mel_wpitch);
    const int paddr = ((lane & 32) | ((16 - k1) & 15) | ((1 - h) << 4)) << 2;  // lane holding Z[512 - k]
    float2 *exw = exf + cls * kClsK + 34 * (bw >> 1) + (bw & 1);  // writer base (float2 units)
    const float2 *exr = exf + h * kClsK + 2 * k1;                  // reader base
    const float hs = 0.25f * a.scale * a.scale;                    // |X wnorm|^2 = (wnorm^2 / 4) |2X|^2
    const bool k1z = k1 == 0;

    unsigned unit = __builtin_amdgcn_readfirstlane(ur.lo + wave);  // uniform: kept scalar
    while (unit < ur.hi) {
        const unsigned next = claim_next(s_next, lane);

        const unsigned clip = unit / pairs;
        const int r = static_cast<int>(unit - clip * pairs) * 2 + fr;
        const float *xc = a.x + static_cast<unsigned long long>(clip) * a.ld;
        const bool active = r < Rreal;
        // functions.rs:137-151: the window covers the last 1024 samples ending at chunk r + n_pad
        const int start = static_cast<int>(r + a.n_pad + 1) * static_cast<int>(a.hop) - 1024;
        const bool inside = active && start >= 0 && start + 1024 <= static_cast<int>(a.n_samples);
        float2 v[16];
        load_window<16, 32>(v, xc, start, static_cast<int>(a.n_samples), jj, active, __all(inside));
        apply_window<16>(v, s_win, jj);
        // ---- 512-point complex FFT as in ss_mfcc_c512 ----
        fft_reg<16>(v);
#pragma unroll
        for (int k = 0; k < 16; ++k) exw[2 * k] = v[k];
        wave_order();
        float2 u[16];
#pragma unroll
        for (int p = 0; p < 8; ++p) {
            const float4 t4 = *reinterpret_cast<const float4 *>(&exr[34 * p]);
            u[2 * p] = make_float2(t4.x, t4.y);
            u[2 * p + 1] = make_float2(t4.z, t4.w);
        }
        wave_order();
#pragma unroll
        for (int p = 0; p < 8; ++p) {
            const float4 w2 = s_t1[p * 16 + k1];
            u[2 * p + 1] = cmul(u[2 * p + 1], make_float2(w2.x, w2.y));
            if (p < 7) u[2 * p + 2] = cmul(u[2 * p + 2], make_float2(w2.z, w2.w));
        }
        fft_reg<16>(u);
        float2 r0[8], r1[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            float px = u[i].x, qx = u[8 + i].x, py = u[i].y, qy = u[8 + i].y;
            swap_rows(px, qx);
            swap_rows(py, qy);
            const float2 wq = cmul(make_float2(qx, qy), s_t2[i * 32 + jj]);
            r0[i] = make_float2(px + wq.x, py + wq.y);
            r1[i] = make_float2(px - wq.x, py - wq.y);
        }
        // ---- untangle Z -> X; (|X| wnorm)^2 (functions.rs:166-169 + feature.rs:164) ----
        float2 zcs[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const float2 sv = k1z ? r1[(8 - i) & 7] : r1[7 - i];
            zcs[i] = make_float2(bperm(paddr, sv.x), bperm(paddr, sv.y));
        }
        const int kb = k1 + 128 * h;
        // stft build (functions.rs:86-123, :166-169): X[k] * wnorm for all 513 bins of the row, interleaved re / im
        float2 *srow = nullptr;
        if (STFT && r < R) srow = reinterpret_cast<float2 *>(a.out) + (static_cast<unsigned long long>(clip) * R + r) * 513ull;
        const float cs = 0.5f * a.scale;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const float2 zk = r0[i];
            float2 zc = zcs[i];
            if (i == 0) zc = k1z ? (h ? r1[0] : zk) : zc;
            const Bin b = untangle_bin(zk, zc, s_twn[i * 32 + jj]);  // the mirrored bin, 2 conj X[512-k] = 2 s - 2 X[k], only where it is wanted
            const float xr = b.xr, xi = b.xi;
            const float2 s = b.s;
            if (STFT) {
                if (srow) {
                    srow[kb + 16 * i] = make_float2(cs * xr, cs * xi);
                    srow[512 - (kb + 16 * i)] = make_float2(cs * fmaf(2.f, s.x, -xr), -cs * fmaf(2.f, s.y, -xi));
                }
                continue;
            }
            prow[kb + 16 * i] = hs * fmaf(xr, xr, xi * xi);
            if (a.fullp) {  // the bank reaches past (F+1)/2: bins 257..512 as well
                const float yr = fmaf(2.f, s.x, -xr), yi = fmaf(2.f, s.y, -xi);
                prow[512 - (kb + 16 * i)] = hs * fmaf(yr, yr, yi * yi);
            }
        }
        if (jj == 0) {
            const float2 z = r1[0];  // X[256] = conj Z[256]
            if (STFT) {
                if (srow) srow[256] = make_float2(a.scale * z.x, -a.scale * z.y);
            } else {
                prow[256] = hs * 4.f * fmaf(z.x, z.x, z.y * z.y);
            }
        }
        if (STFT) {
            wave_order();
            unit = next;
            continue;
        }
        if (jj < 3) prow[(a.fullp ? 513 : 257) + jj] = 0.f;  // pad bins read (with zero weight) by the mel stage
        wave_order();
        // ---- banded mel reduction (feature.rs:173); the two rows of the wave are adjacent words of out[clip][m][.] ----
        if (r < R) {
            float *dst = a.out + static_cast<unsigned long long>(clip) * M * R + r;
            int off = 0;
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const float m = mel_slot4(w4 + off, reinterpret_cast<const float4 *>(prow + st[s]), a.mel_q4[s]);
                if (fi[s] >= 0) dst[static_cast<unsigned long long>(fi[s]) * R] = m;
                off += a.mel_q4[s];
            }
        }
        wave_order();
        unit = next;
    }
}

template <int WAVES>
hipError_t launch_k(const Mfcc1024Args &a, hipStream_t stream, int num_cus, LaunchInfo *info)
{
    const size_t lds = (static_cast<size_t>(WAVES) * kWaveFloatsK + L::kMelW + 32 * static_cast<size_t>(a.mel_wpitch) + 4) * sizeof(float);
    if (lds > 160 * 1024) return hipErrorInvalidValue;
    const unsigned long long total = static_cast<unsigned long long>(a.batch) * a.n_frames;
    if (total == 0) return hipSuccess;
    if (total >= 0xffffffffull) return hipErrorInvalidValue;
    const unsigned long long units = (total + 1) / 2;
    const unsigned grid = cu_capped_grid(units, WAVES, num_cus);
    auto go = [&](auto kern, const char *name) { return launch_kernel(kern, name, grid, WAVES, lds, stream, info, a); };
    const bool pow2 = a.spectrum_exponent == 2, win = a.windowed != 0, lib = a.center != 0 || a.fullp != 0;
#define SS_K(P, M, W, LB, NAME) go(ss_mfcc_c512<P, M, W, WAVES, LB>, NAME)
// the eight builds of one layout; END closes a tag list (">" / ",lib>"), BARE is the list of the build without switches
#define SS_KN(LB, END, BARE)                                                                                                                        \
    if (a.out_mfe) {                                                                                                                                \
        if (pow2) return win ? SS_K(true, true, true, LB, "ss_mfcc_c512<pow2,mfe,win" END) : SS_K(true, true, false, LB, "ss_mfcc_c512<pow2,mfe" END); \
        return win ? SS_K(false, true, true, LB, "ss_mfcc_c512<mfe,win" END) : SS_K(false, true, false, LB, "ss_mfcc_c512<mfe" END);                \
    }                                                                                                                                               \
    if (pow2) return win ? SS_K(true, false, true, LB, "ss_mfcc_c512<pow2,win" END) : SS_K(true, false, false, LB, "ss_mfcc_c512<pow2" END);        \
    return win ? SS_K(false, false, true, LB, "ss_mfcc_c512<win" END) : SS_K(false, false, false, LB, "ss_mfcc_c512" BARE);
    if (lib) { SS_KN(true, ",lib>", "<lib>") }
    SS_KN(false, ">", "")
#undef SS_KN
#undef SS_K
}

}  // namespace

hipError_t launch_mfcc_c512(const Mfcc1024Args &a, hipStream_t stream, int num_cus, LaunchInfo *info)
{
    return launch_k<12>(a, stream, num_cus, info);
}

hipError_t launch_mel_c512(const Mel2048Args &a, hipStream_t stream, int num_cus, LaunchInfo *info)
{
    constexpr int WAVES = 12;
    const size_t lds = (static_cast<size_t>(WAVES) * kWaveFloatsK + L::kMelW + 32 * static_cast<size_t>(a.mel_wpitch) + 4) * sizeof(float);
    if (lds > 160 * 1024) return hipErrorInvalidValue;
    if (a.batch == 0 || a.rows == 0) return hipSuccess;
    const unsigned long long units = static_cast<unsigned long long>(a.batch) * ((a.rows + 1) / 2);
    if (units >= 0xffffffffull) return hipErrorInvalidValue;
    const unsigned grid = cu_capped_grid(units, WAVES, num_cus);
    return a.out_stft ? launch_kernel(ss_mel_c512<WAVES, true>, "ss_mel_c512<stft>", grid, WAVES, lds, stream, info, a)
                      : launch_kernel(ss_mel_c512<WAVES, false>, "ss_mel_c512", grid, WAVES, lds, stream, info, a);
}

}  // namespace ss
