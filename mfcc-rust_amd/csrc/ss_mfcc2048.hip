// ss_mfcc_c1024: fused MFCC / mfe for fft_points = 2048 (C = 1024 packed complex points) on gfx950 -- the frame path
// (feature.rs:99-148, :200-233; processing.rs:65-181) one size up from ss_mfcc512.hip and one down from ss_mfcc4096.hip.
//
//   * 32 lanes own a frame, 32 complex points per lane; a wave carries two consecutive frames of the flat frame list.  One
//     persistent 8-wave workgroup per CU; waves pull frame pairs from an LDS counter.
//   * FFT exactly as in ss_mel2048.hip (a local copy: that file holds a benchmark kernel): radix-32, ONE transposing exchange
//     through wave-private LDS in two register halves (ds_write_b64 scatter to 34*(n1>>1) + 2*k1' + (n1&1), ds_read_b128
//     back), twiddle, radix-32.  No workgroup barrier in the main loop.
//   * untangle with ds_bpermute_b32 (partner = lane 32-j, register 31-r; untangle_bin of ss_wave.h): bins 0..512 go to the P
//     row (the mel bank ends at (F+1)/2, feature.rs:69-70), all 1025 feed the frame energy (feature.rs:216-219), summed over
//     the half-wave.
//   * every other stage is a frame stage of ss_frame32.h, shared with ss_mfcc_c512 (ss_mfcc1024.hip): load_frame, apply_window
//     (optional frame window, mfcc_window switch, from the table block), mel_ln_rows (banded mel, 4 filters per lane, aligned
//     float4 taps; zero handling; ln -> row in filter order), store_mfe_energy (the mfe build stops there), dct_dot (DCT-II
//     with the m <-> M-1-m symmetry of the cosine, half the table); the sum / difference rows, reference scaling and
//     column-0 replacement stay here.
//   * LIB builds (librosa-compatible switches): centred frames with reflect / zero padding at the clip edges, and P rows of
//     all 1025 bins for banks over the whole spectrum; the rows then outgrow the exchange region (10304 B per wave).  The
//     pre-emphasis builds (PRE, a template parameter handed to load_frame) use the LIB layout.
// Reference semantics as in ss_mfcc512.hip; tables: ss::mfcc2048_layout (ss_internal.h).
#include "ss_device.h"
#include "ss_fft_reg.h"
#include "ss_frame32.h"
#include "ss_internal.h"
#include "ss_wave.h"

namespace ss {

namespace {

using namespace wv;
using namespace fr32;

namespace L = mfcc2048_layout;
constexpr int kExSlotsG = 2 * 16 * 34;      // float2 in the wave's exchange region: two frames x half the columns (8704 B)
constexpr int kWaveFloatsG = kExSlotsG * 2;
constexpr int kHalfFloats = kWaveFloatsG / 2;  // per frame after the exchange: P row [520] | ln(mel) row [128] | s [64] | d [64]
constexpr int kHalfFloatsLib = 1288;           // LIB: P row [1028] | ln(mel) row [128] | s [64] | d [64]
template <bool LIB> constexpr int wave_floats() { return LIB ? 2 * kHalfFloatsLib : kWaveFloatsG; }


template <bool POW2, bool MFE, bool WIN, int WAVES, bool LIB = false, bool PRE = false>
__global__ __launch_bounds__(WAVES * 64) void ss_mfcc_c1024(const Mfcc2048Args a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x;
    const int wave = tid >> 6;
    const int lane = tid & 63;
    const int half = lane >> 5;  // frame within the wave
    const int j = lane & 31;     // lane within the frame

    constexpr int kWF = wave_floats<LIB>();
    float *wbase = reinterpret_cast<float *>(smem) + wave * kWF;
    float2 *ex = reinterpret_cast<float2 *>(wbase);
    float *hb = wbase + half * (LIB ? kHalfFloatsLib : kHalfFloats);  // this frame's rows after the exchange
    float *prow = hb, *frow = hb + (LIB ? 1028 : 520), *srow = frow + 128, *drow = srow + 64;
    float *s_tab = reinterpret_cast<float *>(smem) + WAVES * kWF;
    const float4 *s_tw2 = reinterpret_cast<const float4 *>(s_tab + L::kTw2);
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
        st[s] = s_start[s * 32 + j];
        fi[s] = s_filt[s * 32 + j];
    }
    const float4 *w4 = reinterpret_cast<const float4 *>(s_melw + j * a.mel_wpitch);
    const int paddr = ((lane & 32) | ((32 - j) & 31)) << 2;  // lane holding Z[1024 - k]
    const float hscale32 = (POW2 ? 0.25f * a.scale : 0.5f * a.scale) * kTwo32;
    const int M = static_cast<int>(a.n_filters), Cc = static_cast<int>(a.n_ceps), Mh = M / 2, Mc = (M + 1) / 2, nq = (Mc + 3) / 4;
    // fused pre-emphasis: builds of their own (LIB layout: they also serve centred frames)
    const unsigned psh = PRE ? a.preemph_shift % a.n_samples : 0u;

    unsigned unit = __builtin_amdgcn_readfirstlane(ur.lo + wave);  // uniform: kept scalar
    while (unit < ur.hi) {
        const unsigned next = claim_next(s_next, lane);

        const unsigned gf_raw = 2 * unit + half;
        const bool live = gf_raw < total;
        const unsigned gf = live ? gf_raw : total - 1;
        const unsigned clip = gf / a.n_frames;
        const unsigned t = gf - clip * a.n_frames;
        // stack_frames (processing.rs:65-129, contract framing): frame t starts at sample t*step; librosa center=True (LIB
        // builds): it is centred on sample t*step
        const float *xc = a.x + static_cast<unsigned long long>(clip) * a.ld;
        const int s0 = static_cast<int>(t * a.step) - (LIB && a.center ? static_cast<int>(a.flen / 2) : 0);
        float2 v[32];
        load_frame<32, LIB>(v, a, xc, s0, j, PRE, psh);
        if (WIN) apply_window<32>(v, s_win, j);
        // ---- 1024-point complex FFT: radix-32, transpose through LDS (two register halves), twiddle, radix-32 ----
        fft_reg<32>(v);
        float2 u[32];
        float2 *exf = ex + half * (16 * 34);
        const int wbh = 34 * (j >> 1) + (j & 1);
        const int jl = j & 15;
#pragma unroll
        for (int k = 0; k < 16; ++k) exf[wbh + 2 * k] = v[k];
        wave_order();
        if (j < 16) {
#pragma unroll
            for (int p = 0; p < 16; ++p) {
                const float4 t4 = *reinterpret_cast<const float4 *>(&exf[34 * p + 2 * jl]);
                u[2 * p] = make_float2(t4.x, t4.y);
                u[2 * p + 1] = make_float2(t4.z, t4.w);
            }
        }
        wave_order();
#pragma unroll
        for (int k = 0; k < 16; ++k) exf[wbh + 2 * k] = v[16 + k];
        wave_order();
        if (j >= 16) {
#pragma unroll
            for (int p = 0; p < 16; ++p) {
                const float4 t4 = *reinterpret_cast<const float4 *>(&exf[34 * p + 2 * jl]);
                u[2 * p] = make_float2(t4.x, t4.y);
                u[2 * p + 1] = make_float2(t4.z, t4.w);
            }
        }
        wave_order();
#pragma unroll
        for (int p = 0; p < 16; ++p) {
            const float4 w2 = s_tw2[p * 32 + j];
            u[2 * p + 1] = cmul(u[2 * p + 1], make_float2(w2.x, w2.y));
            if (p < 15) u[2 * p + 2] = cmul(u[2 * p + 2], make_float2(w2.z, w2.w));
        }
        fft_reg<32>(u);  // u[r] = Z[j + 32 r]

        // ---- untangle Z -> X; |X| (processing.rs:168) * 1/N (:180); row sum (feature.rs:216) ----
        float esum = 0.f;
#pragma unroll
        for (int hb2 = 0; hb2 < 2; ++hb2) {
            float2 zcs[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) zcs[q] = make_float2(bperm(paddr, u[31 - (8 * hb2 + q)].x), bperm(paddr, u[31 - (8 * hb2 + q)].y));
#pragma unroll
            for (int qq = 0; qq < 8; ++qq) {
                const int q = 8 * hb2 + qq;
                const float2 zk = u[q];
                // lane 0 pairs with itself: Z[1024 - 32 q] = own register (32 - q) & 31
                const float2 zc = j == 0 ? u[(32 - q) & 31] : zcs[qq];
                const Bin b = untangle_bin(zk, zc, s_twn[q * 32 + j]);
                const float xb_r = fmaf(2.f, b.s.x, -b.xr), xb_i = fmaf(2.f, b.s.y, -b.xi);  // 2 conj X[1024-k] = 2 s - 2 X[k]
                const float na = b.xr * b.xr + b.xi * b.xi, nb = xb_r * xb_r + xb_i * xb_i;
                const float pa = POW2 ? na : __builtin_amdgcn_sqrtf(na);
                const float pb = POW2 ? nb : __builtin_amdgcn_sqrtf(nb);
                prow[j + 32 * q] = pa;  // bins 0..511 (the bank ends at (F+1)/2, feature.rs:69-70); 512 below
                if (LIB) prow[1024 - (j + 32 * q)] = pb;  // bins 513..1024 for banks over the whole spectrum
                esum += pa + pb;        // X[0] and X[1024] come from lane 0's self pair (q = 0)
            }
        }
        if (j == 0) {
            const float2 z = u[16];  // X[512] = conj Z[512]
            const float n = 4.f * (z.x * z.x + z.y * z.y);
            const float p512 = POW2 ? n : __builtin_amdgcn_sqrtf(n);
            prow[512] = p512;
            esum += p512;
        }
        if (j < 3) prow[(LIB ? 1025 : 513) + j] = 0.f;  // pad bins read (with zero weight) by the mel stage
        float energy = hscale32 * half_sum(esum);              // E * 2^32
        energy = energy == 0.f ? kEps * kTwo32 : energy;     // zero_handling, feature.rs:219
        wave_order();

        mel_ln_rows<MFE>(w4, prow, st, fi, a.mel_q4, hscale32, frow, a.out + static_cast<unsigned long long>(gf) * M, live);
        if (MFE) {
            store_mfe_energy(a.out_energy, gf, energy, j, live);
            wave_order();
            unit = next;
            continue;
        }
        wave_order();
        // ---- DCT-II (feature.rs:120-123), cos(pi c (2(M-1-m)+1) / 2M) = (-1)^c cos(pi c (2m+1) / 2M): sum and difference rows
        // once per frame (the text of ss_mfcc_c512's: see ss_frame32.h), then a (M+1)/2-term product per coefficient ----
#pragma unroll
        for (int h2 = 0; h2 < 2; ++h2) {
            const int m = j + 32 * h2;
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
        const float4 *r4 = reinterpret_cast<const float4 *>((j & 1) ? drow : srow);  // coefficients j and j + 32: same parity, same row
        if (j < Cc) {
            const float acc = dct_dot(r4, reinterpret_cast<const float4 *>(s_cos + j * L::kCosPitch), nq);
            // scaling + column-0 replacement (feature.rs:126-146)
            float o = acc * a.dct_scale_k;
            if (j == 0) o = a.dc_elimination ? ln_scaled(energy) : acc * (t == 0 ? a.dct_scale_00 : a.dct_scale_0);
            if (live) a.out[static_cast<unsigned long long>(gf) * Cc + j] = o;
        }
        if (Cc > 32) {  // 33..64 cepstra: the lane also forms coefficient j + 32
            wave_order();
            if (j + 32 < Cc) {
                const float acc = dct_dot(r4, reinterpret_cast<const float4 *>(s_cos + (j + 32) * L::kCosPitch), nq);
                if (live) a.out[static_cast<unsigned long long>(gf) * Cc + j + 32] = acc * a.dct_scale_k;
            }
        }
        wave_order();
        unit = next;
    }
}

template <int WAVES>
hipError_t launch_g(const Mfcc2048Args &a, hipStream_t stream, int num_cus, LaunchInfo *info)
{
    const bool lib = a.center != 0 || a.fullp != 0 || a.preemph != 0.f;  // the pre-emphasis builds use the LIB layout
    const size_t lds = (static_cast<size_t>(WAVES) * (lib ? wave_floats<true>() : wave_floats<false>()) + L::kMelW + 32 * static_cast<size_t>(a.mel_wpitch) + 4) * sizeof(float);
    if (lds > 160 * 1024) return hipErrorInvalidValue;
    const unsigned long long total = static_cast<unsigned long long>(a.batch) * a.n_frames;
    if (total == 0) return hipSuccess;
    if (total >= 0xffffffffull) return hipErrorInvalidValue;
    const unsigned long long units = (total + 1) / 2;
    const unsigned grid = cu_capped_grid(units, WAVES, num_cus);
    auto go = [&](auto kern, const char *name) { return launch_kernel(kern, name, grid, WAVES, lds, stream, info, a); };
    const bool pow2 = a.spectrum_exponent == 2, win = a.windowed != 0;
#define SS_G(P, M, W, LB, PR, NAME) go(ss_mfcc_c1024<P, M, W, WAVES, LB, PR>, NAME)
// the eight builds of one layout; END closes a tag list (">" / ",lib>" / ",lib,pre>"), BARE is the list of the build without switches
#define SS_GN(LB, PR, END, BARE)                                                                                                                            \
    if (a.out_mfe) {                                                                                                                                        \
        if (pow2) return win ? SS_G(true, true, true, LB, PR, "ss_mfcc_c1024<pow2,mfe,win" END) : SS_G(true, true, false, LB, PR, "ss_mfcc_c1024<pow2,mfe" END); \
        return win ? SS_G(false, true, true, LB, PR, "ss_mfcc_c1024<mfe,win" END) : SS_G(false, true, false, LB, PR, "ss_mfcc_c1024<mfe" END);              \
    }                                                                                                                                                       \
    if (pow2) return win ? SS_G(true, false, true, LB, PR, "ss_mfcc_c1024<pow2,win" END) : SS_G(true, false, false, LB, PR, "ss_mfcc_c1024<pow2" END);      \
    return win ? SS_G(false, false, true, LB, PR, "ss_mfcc_c1024<win" END) : SS_G(false, false, false, LB, PR, "ss_mfcc_c1024" BARE);
    if (a.preemph != 0.f) { SS_GN(true, true, ",lib,pre>", "<lib,pre>") }
    if (lib) { SS_GN(true, false, ",lib>", "<lib>") }
    SS_GN(false, false, ">", "")
#undef SS_GN
#undef SS_G
}

}  // namespace

hipError_t launch_mfcc_c1024(const Mfcc2048Args &a, hipStream_t stream, int num_cus, LaunchInfo *info)
{
    return launch_g<8>(a, stream, num_cus, info);
}

}  // namespace ss
