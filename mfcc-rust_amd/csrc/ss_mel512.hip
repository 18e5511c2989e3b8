// ss_mel_c256: fused mel-spectrogram for fft_points = 512 on gfx950 -- frame_analysis + |X wnorm|^2 + the mel einsum
// (functions.rs:125-170, feature.rs:151-174) in one launch; the STFT-path sibling of ss_mfcc512.hip, one size down from
// ss_mel2048.hip.
//
//   * 16 lanes (one DPP row) own a 512-sample window = 256 packed complex points, 16 per lane; a wave carries four
//     consecutive rows of one clip, the work unit pulled from the LDS counter is a (clip, row quad).  One persistent
//     12-wave workgroup per CU; the next unit's samples are prefetched into the dead window registers.
//   * Row r of a clip covers the 512 samples that end at chunk r + n_pad (functions.rs:137-151): zero initial state,
//     zero tail, rows past the real ones are all zero (D3).  Windows inside the clip load as 8-byte pairs at constant
//     offsets; at the clip edges one masked range per lane (load_window of ss_frame32.h, shared with ss_mel_c512 and
//     ss_mel_c2048).  Vorbis window pairs come from the table block in LDS.
//   * FFT / untangle: the shared quad skeleton of ss_quad256.h.  |X|^2 wnorm^2 of bins 0..128 -- or all 257 when the
//     bank reaches past (F+1)/2 -- goes to a P row inside the slot.
//   * banded mel, up to 5 filters per lane (80 filters), host-sorted by tap count; the four rows of a wave are adjacent
//     words of out[clip][m][.].  No zero handling, no log (feature.rs:164-173).
//   * stft build (ss_stft_device): skips the mel stage and writes X[k] wnorm for all 257 bins of a row.
// Tables: ss::mel512_layout (ss_internal.h).
#include "ss_device.h"
#include "ss_fft_reg.h"
#include "ss_frame32.h"
#include "ss_internal.h"
#include "ss_quad256.h"
#include "ss_wave.h"

namespace ss {

namespace {

using namespace wv;
using namespace q256;  // the slot holds, after the exchange, the P row [260]

namespace L = mel512_layout;

template <int WAVES, bool STFT>
__global__ __launch_bounds__(WAVES * 64) void ss_mel_c256(const Mel512Args a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x;
    const int wave = tid >> 6;
    const int lane = tid & 63;
    const int f = lane >> 4;  // row within the quad
    const int j = lane & 15;  // lane within the row (DPP row)

    float *slot = reinterpret_cast<float *>(smem) + wave * kWaveFloats + f * kSlotFloats;
    float2 *zh = reinterpret_cast<float2 *>(slot);
    float *prow = slot;
    float *s_tab = reinterpret_cast<float *>(smem) + WAVES * kWaveFloats;
    const float4 *s_tw2 = reinterpret_cast<const float4 *>(s_tab + L::kTw2);
    const float2 *s_twn = reinterpret_cast<const float2 *>(s_tab + L::kTwn);
    const float2 *s_win = reinterpret_cast<const float2 *>(s_tab + L::kWin);
    const int *s_start = reinterpret_cast<const int *>(s_tab + L::kStart);
    const int *s_filt = reinterpret_cast<const int *>(s_tab + L::kFilt);
    const float *s_melw = s_tab + L::kMelW;
    unsigned *s_next = reinterpret_cast<unsigned *>(s_tab + L::kMelW + 16 * a.mel_wpitch);

    const int R = static_cast<int>(a.rows), Rreal = static_cast<int>(a.real_rows), M = static_cast<int>(a.n_filters);
    // work unit: four consecutive rows of one clip; the workgroup owns a contiguous range of units
    const unsigned qpc = (a.rows + 3) / 4;
    const unsigned long long units = static_cast<unsigned long long>(a.batch) * qpc;
    const unsigned u_lo = static_cast<unsigned>(units * blockIdx.x / gridDim.x);
    const unsigned u_hi = static_cast<unsigned>(units * (blockIdx.x + 1) / gridDim.x);
    stage_tables(s_tab, a.tab, (L::kMelW + 16 * a.mel_wpitch) / 4, tid, WAVES * 64);
    if (tid == 0) *s_next = u_lo + WAVES;
    // (clip, row) of this lane group within a unit, and the loads of its window: functions.rs:137-151, the window covers
    // the last 512 samples ending at chunk r + n_pad
    auto load_unit = [&](unsigned un, float2 (&vv)[16]) {
        const unsigned clip = un / qpc;
        const int r = static_cast<int>(un - clip * qpc) * 4 + f;
        const float *xc = a.x + static_cast<unsigned long long>(clip) * a.ld;
        const bool active = r < Rreal;
        const int start = static_cast<int>(r + a.n_pad + 1) * static_cast<int>(a.hop) - 512;
        const bool inside = active && start >= 0 && start + 512 <= static_cast<int>(a.n_samples);
        // clip edges (zero initial state, zero padding of the last chunk, D3) and inactive rows: load_window's masked paths
        fr32::load_window<16, 16>(vv, xc, start, static_cast<int>(a.n_samples), j, active, __all(inside));
    };
    unsigned unit = __builtin_amdgcn_readfirstlane(u_lo + wave);  // uniform: kept scalar
    float2 vin[16];
    if (unit < u_hi) load_unit(unit, vin);

    const int paddr = partner_addr(lane, j), wbase1 = exchange_write_base(j);
    const float hs = 0.25f * a.scale * a.scale;              // |X wnorm|^2 = (wnorm^2 / 4) |2X|^2
    __syncthreads();
    int st[5], fi[5];
#pragma unroll
    for (int s = 0; s < 5; ++s) {
        st[s] = s_start[s * 16 + j];
        fi[s] = s_filt[s * 16 + j];
    }
    const float4 *w4 = reinterpret_cast<const float4 *>(s_melw + j * a.mel_wpitch);
    float2 twn[8];  // the untangle twiddles stay in registers; the pass-2 ones would spill next to the 32 prefetch registers
#pragma unroll
    for (int r = 0; r < 8; ++r) twn[r] = s_twn[r * 16 + j];

    while (unit < u_hi) {
        const unsigned next = claim_next(s_next, lane);
        const unsigned clip = unit / qpc;
        const int r = static_cast<int>(unit - clip * qpc) * 4 + f;

        float2 v[16];
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const float2 w = s_win[j + 16 * e];
            v[e] = make_float2(vin[e].x * w.x, vin[e].y * w.y);
        }
        // ---- 256-point complex FFT; the next unit's samples go into the dead window registers ----
        pass1(v, zh, wbase1);
        if (next < u_hi) load_unit(next, vin);
        float2 u[16];
        pass2(u, zh, j, s_tw2);

        // ---- untangle Z -> X; (|X| wnorm)^2 (functions.rs:166-169 + feature.rs:164) ----
        // stft build (functions.rs:86-123, :166-169): X[k] * wnorm for all 257 bins of the row, interleaved re / im
        float2 *srow = nullptr;
        if (STFT && r < R) srow = reinterpret_cast<float2 *>(a.out) + (static_cast<unsigned long long>(clip) * R + r) * 257ull;
        const float cs = 0.5f * a.scale;
        float2 zcs[8];
        fetch_partners(u, paddr, zcs);
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const Bin b = untangle(u, zcs, twn[q], j, q);  // the mirrored bin, 2 conj X[256-k] = 2 s - 2 X[k], only where it is wanted
            const float xr = b.xr, xi = b.xi;
            const float2 s = b.s;
            if (STFT) {
                if (srow) {
                    srow[j + 16 * q] = make_float2(cs * xr, cs * xi);
                    srow[256 - j - 16 * q] = make_float2(cs * fmaf(2.f, s.x, -xr), -cs * fmaf(2.f, s.y, -xi));
                }
                continue;
            }
            prow[j + 16 * q] = hs * fmaf(xr, xr, xi * xi);
            if (a.fullp) {  // the bank reaches past (F+1)/2: bins 129..256 as well
                const float yr = fmaf(2.f, s.x, -xr), yi = fmaf(2.f, s.y, -xi);
                prow[256 - j - 16 * q] = hs * fmaf(yr, yr, yi * yi);
            }
        }
        if (j == 0) {
            const float2 z = u[8];  // X[128] = conj Z[128]
            if (STFT) {
                if (srow) srow[128] = make_float2(a.scale * z.x, -a.scale * z.y);
            } else {
                prow[128] = hs * 4.f * fmaf(z.x, z.x, z.y * z.y);
            }
        }
        if (STFT) {
            wave_order();
            unit = next;
            continue;
        }
        if (j < 3) prow[(a.fullp ? 257 : 129) + j] = 0.f;  // pad bins read (with zero weight) by the mel stage
        wave_order();

        // ---- banded mel reduction (feature.rs:173); the four rows of the wave are adjacent words of out[clip][m][.] ----
        if (r < R) {
            float *dst = a.out + static_cast<unsigned long long>(clip) * M * R + r;
            int off = 0;
#pragma unroll
            for (int s = 0; s < 5; ++s) {
                if (a.mel_q4[s] == 0) break;
                const float m = mel_slot1(w4 + off, prow + st[s], a.mel_q4[s]);
                if (fi[s] >= 0) dst[static_cast<unsigned long long>(fi[s]) * R] = m;
                off += a.mel_q4[s];
            }
        }
        wave_order();
        unit = next;
    }
}

}  // namespace

hipError_t launch_mel_c256(const Mel512Args &a, hipStream_t stream, int num_cus, LaunchInfo *info)
{
    constexpr int WAVES = 12;
    const size_t lds = (static_cast<size_t>(WAVES) * kWaveFloats + L::kMelW + 4 + 16 * static_cast<size_t>(a.mel_wpitch)) * sizeof(float);
    if (lds > kLdsLimit) return hipErrorInvalidValue;
    if (a.batch == 0 || a.rows == 0) return hipSuccess;
    const unsigned long long units = static_cast<unsigned long long>(a.batch) * ((a.rows + 3) / 4);
    if (units >= 0xffffffffull) return hipErrorInvalidValue;
    const unsigned grid = cu_capped_grid(units, WAVES, num_cus);
    return a.out_stft ? launch_kernel(ss_mel_c256<WAVES, true>, "ss_mel_c256<stft>", grid, WAVES, lds, stream, info, a)
                      : launch_kernel(ss_mel_c256<WAVES, false>, "ss_mel_c256", grid, WAVES, lds, stream, info, a);
}

}  // namespace ss
