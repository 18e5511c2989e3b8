// Whisper log-mel front end: ss_whisper_* of include/speechsauce_amd.h, whose comment is the definition; the reference crate has no
// such stage, so this file restates nothing of it.  400-point frames are not a power of two: ss_params configurations with
// fft_points = 400 run the chirp-z build of the generic kernel (two 1024-point complex transforms per frame).  This family has a
// kernel of its own instead: ONE 200-point complex transform per frame, z[n] = x[2n] + i x[2n+1], and the real-FFT untangle.
//
// ss_whisper_c200 (gfx950, wave64).  200 = 25 x 8: eight lanes own a frame, lane j holds the points n = j + 8 m, m < 25, in
// registers.  Radix 5 x 5 over m in registers, the twiddles exp(-2 pi i j k1 / 200), then radix 8 over the eight lanes as three
// radix-2 steps whose partner values arrive by DPP (quad_perm for lane ^ 1 and lane ^ 2, row_half_mirror + quad_perm for lane ^ 4):
// no LDS round trip.  Lane j ends with the bins k = 25 bitrev3(j) + k1.  The untangle partner Z[200 - k] of k1 >= 1 is register
// 25 - k1 of lane j ^ 7 (the complement of a bit-reversed index is the bit-reversed complement): one row_half_mirror per value;
// the k1 = 0 bins pair through one ds_bpermute_b32.  A wave carries 8 frames per pass and two passes per unit, so a unit is 16
// consecutive frames of one clip; persistent workgroups of 8 waves, one per CU, take their units (every grid-th unit, so that clips of
// different lengths balance) from an LDS counter.
//
// Per pass: the power row of 201 bins per frame goes to a wave-private LDS row; lane (f = lane & 7, g = lane >> 3) forms the mel
// sums of frame f for the filters m = g + 8 i from the host-sparsified Slaney bank (taps in ascending k, one fmaf each), then
// l = sum > 1e-10 ? log10(sum) : -10 into the wave's [M][16] tile.  Behind the second pass the tile goes out along t: a lane stores
// four consecutive frames of one mel row (16 bytes where the row is so aligned), four lanes a run of 16 floats.  The clip's maximum
// is gathered by integer atomicMax on float_key; the keys are set by ss_whisper_keys_kernel in front, so a captured call holds no
// memset node.
//
// Silent frames (ss_whisper.h: first_silent) are neither loaded nor transformed nor stored here: a unit that begins with one is
// dropped when it is claimed, and so is a second pass.  ss_whisper_floor_kernel writes them: for every element of out it takes the
// stored l, or -10 for a silent frame, and stores conv(fmaf(max(l, mx - 8), 0.25f, 1.0f)) with 16-byte stores.
//
// 16-bit PCM (ss_whisper_log_mel*_i16*): ss_whisper_c200<int16_t>, reported as ss_whisper_c200i.  Sample k is (float)x[k] * scale,
// scale a power of two (the product is exact).  An interior pass fetches every pair as ONE dword at 2-byte alignment (pcm_raw_pair)
// and converts it on the spot -- this kernel does not prefetch across iterations -- so one path serves either parity of the clip's
// first sample; an edge pass reads single 16-bit samples through the same reflect / live tests.  Everything behind the load is the
// float build's text, so the bits are the float call's on the converted samples.  The keys and floor kernels never read x.
//
// The whole file is compiled with fp contract(off): every fused operation is an explicit fmaf, and the dense and the packed call
// are the SAME kernel (a null table selects the dense addressing), so they cannot round differently.
#include "ss_device.h"
#include "ss_hip_staging.h"
#include "ss_host_checks.h"
#include "ss_internal.h"
#include "ss_wave.h"
#include "ss_whisper.h"

#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#pragma clang fp contract(off)

namespace ss {

namespace {

using namespace whisper;

constexpr unsigned kWhisperError = 4u;  // the handle's error word after a bad table entry

template <typename T>  // T: float, or int16_t (16-bit PCM times `scale`)
struct WhisperArgs {
    const T *x;
    const long long *so;  // [n_clips + 1] sample offsets of the packed call; null: dense rows
    unsigned long long ld;  // dense: row stride
    uint32_t n_samples;     // dense: min(n_samples, N)
    uint32_t n_clips, n_frames, n_mels;
    const float *tab;
    float *inter;  // [n_clips x M x n_frames] f32: out itself (SS_PAD_F32) or the caller's scratch
    int *keys;     // [n_clips]
    uint32_t q_base, q_rem;  // split_units of n_clips * units_per_clip(n_frames) over the grid
    float scale;             // PCM build: the power-of-two sample scale (float build: unused)
};

// live samples L = min(len, N) of clip c and its first sample; a bad table entry is an empty clip (ok = false)
template <typename T>
struct Clip {
    const T *x;
    uint32_t L;
    bool ok;
};
template <typename T>
__device__ __forceinline__ Clip<T> clip_of(const T *x, const long long *so, unsigned long long ld, uint32_t n_samples, uint32_t n_frames, uint32_t c)
{
    const uint32_t N = n_frames * kHop;
    if (!so) return Clip<T>{x + static_cast<size_t>(c) * ld, n_samples < N ? n_samples : N, true};
    const long long lo = so[c], hi = so[c + 1];
    if (lo < 0 || hi < lo) return Clip<T>{x, 0u, false};
    const unsigned long long len = static_cast<unsigned long long>(hi - lo);
    return Clip<T>{x + lo, len < N ? static_cast<uint32_t>(len) : N, true};
}

__device__ __forceinline__ float2 cmul(float2 a, float2 b) { return make_float2(fmaf(-a.y, b.y, a.x * b.x), fmaf(a.y, b.x, a.x * b.y)); }

// 5-point DFT, forward: y[k] = sum_n x[n] exp(-2 pi i n k / 5)
__device__ __forceinline__ void dft5(float2 &x0, float2 &x1, float2 &x2, float2 &x3, float2 &x4)
{
    constexpr float c1 = 0.309017f, c2 = -0.809017f, s1 = 0.95105654f, s2 = 0.58778524f;
    const float2 t1 = make_float2(x1.x + x4.x, x1.y + x4.y), t2 = make_float2(x2.x + x3.x, x2.y + x3.y);
    const float2 t3 = make_float2(x1.x - x4.x, x1.y - x4.y), t4 = make_float2(x2.x - x3.x, x2.y - x3.y);
    const float2 m1 = make_float2(fmaf(c2, t2.x, fmaf(c1, t1.x, x0.x)), fmaf(c2, t2.y, fmaf(c1, t1.y, x0.y)));
    const float2 m2 = make_float2(fmaf(c1, t2.x, fmaf(c2, t1.x, x0.x)), fmaf(c1, t2.y, fmaf(c2, t1.y, x0.y)));
    const float2 n1 = make_float2(fmaf(s2, t4.x, s1 * t3.x), fmaf(s2, t4.y, s1 * t3.y));
    const float2 n2 = make_float2(fmaf(-s1, t4.x, s2 * t3.x), fmaf(-s1, t4.y, s2 * t3.y));
    x0 = make_float2(x0.x + t1.x + t2.x, x0.y + t1.y + t2.y);
    x1 = make_float2(m1.x + n1.y, m1.y - n1.x);  // m1 - i n1
    x4 = make_float2(m1.x - n1.y, m1.y + n1.x);
    x2 = make_float2(m2.x + n2.y, m2.y - n2.x);
    x3 = make_float2(m2.x - n2.y, m2.y + n2.x);
}

// cos, sin of 2 pi k / 25
__device__ constexpr float kC25[25] = {1.f,           0.968583167f,  0.876306653f,  0.72896862f,   0.535826802f,  0.309017003f,  0.0627905205f,
                                       -0.187381312f, -0.425779283f, -0.637423992f, -0.809017003f, -0.92977649f,  -0.992114723f, -0.992114723f,
                                       -0.92977649f,  -0.809017003f, -0.637423992f, -0.425779283f, -0.187381312f, 0.0627905205f, 0.309017003f,
                                       0.535826802f,  0.72896862f,   0.876306653f,  0.968583167f};
__device__ constexpr float kS25[25] = {0.f,           0.24868989f,   0.481753677f,  0.684547126f,  0.844327927f,  0.95105654f,   0.998026729f,
                                       0.982287228f,  0.904827058f,  0.770513237f,  0.587785244f,  0.368124545f,  0.125333235f,  -0.125333235f,
                                       -0.368124545f, -0.587785244f, -0.770513237f, -0.904827058f, -0.982287228f, -0.998026729f, -0.95105654f,
                                       -0.844327927f, -0.684547126f, -0.481753677f, -0.24868989f};

// 25-point DFT in registers: in v[m], out v[c + 5 d] = Y[c + 5 d] -- m = 5 a + b: five DFTs over a, the twiddles exp(-2 pi i b c / 25),
// five DFTs over b
__device__ __forceinline__ void dft25(float2 (&v)[25])
{
#pragma unroll
    for (int b = 0; b < 5; ++b) dft5(v[b], v[5 + b], v[10 + b], v[15 + b], v[20 + b]);  // v[5 c + b] = T_b[c]
#pragma unroll
    for (int c = 1; c < 5; ++c)
#pragma unroll
        for (int b = 1; b < 5; ++b) v[5 * c + b] = cmul(v[5 * c + b], make_float2(kC25[b * c], -kS25[b * c]));
#pragma unroll
    for (int c = 0; c < 5; ++c) dft5(v[5 * c], v[5 * c + 1], v[5 * c + 2], v[5 * c + 3], v[5 * c + 4]);  // v[5 c + d] = Y[c + 5 d]
}

constexpr int kDppXor1 = 0xB1, kDppXor2 = 0x4E, kDppXor3 = 0x1B, kDppHalfMirror = 0x141;  // quad_perm [1,0,3,2], [2,3,0,1], [3,2,1,0]; row_half_mirror

template <int H>
__device__ __forceinline__ float lane_xor(float v)
{
    if constexpr (H == 1) return wv::dpp<kDppXor1>(v);
    else if constexpr (H == 2) return wv::dpp<kDppXor2>(v);
    else return wv::dpp<kDppXor3>(wv::dpp<kDppHalfMirror>(v));  // (l ^ 7) ^ 3 = l ^ 4
}

// one radix-2 step of the decimation-in-frequency radix 8 over the lanes: the lane without bit H gets a + p, the lane with it
// (p - a) tw; sgn = +1 / -1, tw = 1 on the lanes without the bit
template <int H>
__device__ __forceinline__ float2 lane_step(float2 a, float sgn, float2 tw)
{
    const float2 p = make_float2(lane_xor<H>(a.x), lane_xor<H>(a.y));
    const float2 r = make_float2(fmaf(sgn, a.x, p.x), fmaf(sgn, a.y, p.y));
    if constexpr (H == 1) return r;
    else return cmul(r, tw);
}

__device__ __forceinline__ float wave_max(float v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}

__global__ __launch_bounds__(256) void ss_whisper_keys_kernel(const long long *__restrict__ so, uint32_t n_clips, uint32_t n_frames, int *__restrict__ keys,
                                                             int *__restrict__ lengths, uint32_t dense_len, unsigned *err)
{
    const uint32_t c = blockIdx.x * 256u + threadIdx.x;
    if (c >= n_clips) return;
    keys[c] = float_key(kLogFloor);
    int len = static_cast<int>(dense_len);
    if (so) {
        const long long lo = so[c], hi = so[c + 1];
        const bool bad = lo < 0 || hi < lo;
        const unsigned long long fr = bad ? 0ull : static_cast<unsigned long long>(hi - lo) / kHop;
        len = bad ? -1 : static_cast<int>(fr < n_frames ? fr : n_frames);
        if (bad && err) __hip_atomic_store(err, kWhisperError, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    if (lengths) lengths[c] = len;
}

template <typename T>
__global__ __launch_bounds__(kWaves * 64) void ss_whisper_c200(WhisperArgs<T> a)
{
    constexpr bool PCM = std::is_same_v<T, int16_t>;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float *s_tab = reinterpret_cast<float *>(smem);
    unsigned *s_next = reinterpret_cast<unsigned *>(s_tab + layout::kFloats);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float *s_wave = s_tab + layout::kFloats + 4 + static_cast<size_t>(wave) * kWaveFloats;
    float *s_prow = s_wave;                             // [8][kPRowPitch]
    float *s_tile = s_wave + kPassFrames * kPRowPitch;  // [M][kTilePitch]

    for (int i = tid; i < layout::kFloats / 4; i += kWaves * 64) reinterpret_cast<float4 *>(s_tab)[i] = reinterpret_cast<const float4 *>(a.tab)[i];
    if (tid == 0) *s_next = 0;
    __syncthreads();

    const float2 *s_win = reinterpret_cast<const float2 *>(s_tab + layout::kWin);
    const float2 *s_tw2 = reinterpret_cast<const float2 *>(s_tab + layout::kTw2);
    const float2 *s_twn = reinterpret_cast<const float2 *>(s_tab + layout::kTwn);
    const int *s_start = reinterpret_cast<const int *>(s_tab + layout::kStart);
    const int *s_len = reinterpret_cast<const int *>(s_tab + layout::kLen);
    const int *s_off = reinterpret_cast<const int *>(s_tab + layout::kOff);
    const float *s_melw = s_tab + layout::kMelW;

    const int j = lane & 7, f = lane >> 3;  // transform: lane j of frame f
    // the radix-8 steps' signs and twiddles: exp(-2 pi i (j & 3) / 8) on the lanes with bit 2, exp(-2 pi i (j & 1) / 4) on those with bit 1
    constexpr float r2 = 0.70710677f;
    const float sg4 = (j & 4) ? -1.f : 1.f, sg2 = (j & 2) ? -1.f : 1.f, sg1 = (j & 1) ? -1.f : 1.f;
    float2 tw4 = make_float2(1.f, 0.f), tw2 = make_float2(1.f, 0.f);
    if (j & 4) tw4 = (j & 3) == 0 ? make_float2(1.f, 0.f) : (j & 3) == 1 ? make_float2(r2, -r2) : (j & 3) == 2 ? make_float2(0.f, -1.f) : make_float2(-r2, -r2);
    if ((j & 2) && (j & 1)) tw2 = make_float2(0.f, -1.f);
    const int K2 = static_cast<int>(bitrev3(static_cast<uint32_t>(j)));
    const int self_addr = ((lane & ~7) | static_cast<int>(bitrev3(static_cast<uint32_t>((8 - K2) & 7)))) << 2;  // the lane holding Z[200 - 25 K2]
    const int mf = lane & 7, mg = lane >> 3;  // mel stage: frame mf, filters mg + 8 i

    const uint32_t upc = units_per_clip(a.n_frames);
    const uint32_t b = blockIdx.x;
    // workgroup b takes the units b, b + grid, b + 2 grid, ...: a clip's units spread over the workgroups, so that clips of different
    // lengths (whose silent units cost nothing) do not leave the workgroup of the longest clip working alone
    const uint32_t count = a.q_base + (b < a.q_rem ? 1u : 0u);
    const int N = static_cast<int>(a.n_frames * kHop);

    for (;;) {
        unsigned u = 0;
        if (lane == 0) u = atomicAdd(s_next, 1u);
        u = __builtin_amdgcn_readfirstlane(u);
        if (u >= count) break;
        const uint32_t unit = b + u * gridDim.x;
        const uint32_t c = unit / upc, t0 = (unit - c * upc) * kUnitFrames;  // uniform
        const Clip<T> clip = clip_of(a.x, a.so, a.ld, a.n_samples, a.n_frames, c);
        const uint32_t L = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(clip.L)));
        const uint32_t limit = first_silent(L, a.n_frames);  // frames t >= limit are silent (or past the end)
        if (t0 >= limit) continue;                            // a silent unit: nothing is loaded, transformed or stored
        const T *xb = clip.x;
        // uniform: the clip's even samples sit on 8-byte boundaries (a PCM pair is one dword at any parity: no split)
        [[maybe_unused]] const bool pair_ok = (reinterpret_cast<uintptr_t>(xb) & 7u) == 0;
        float lmax = kLogFloor;

#pragma unroll 1
        for (uint32_t pass = 0; pass < 2; ++pass) {
            const uint32_t tp = t0 + pass * kPassFrames;
            if (tp >= limit) break;  // uniform
            float2 v[25];
            const int t = static_cast<int>(tp) + f;
            const int i0 = t * static_cast<int>(kHop) - static_cast<int>(kHalf) + 2 * j;  // the lane's first raw sample index
            // interior: every raw index of the pass's eight frames is a live sample of the clip
            const bool interior = tp * kHop >= kHalf && (tp + kPassFrames - 1) * kHop + kHalf <= L;
            if (interior && (PCM || pair_ok)) {
#pragma unroll
                for (int m = 0; m < 25; ++m) {
                    if constexpr (PCM) v[m] = pcm_pair(__float_as_int(pcm_raw_pair(xb + i0 + 16 * m)), a.scale);
                    else v[m] = *reinterpret_cast<const float2 *>(xb + i0 + 16 * m);
                }
            } else if (interior) {  // (float build only: a PCM pair is one dword at either parity)
#pragma unroll
                for (int m = 0; m < 25; ++m) v[m] = make_float2(static_cast<float>(xb[i0 + 16 * m]), static_cast<float>(xb[i0 + 16 * m + 1]));
            } else {
                const bool live = static_cast<uint32_t>(t) < a.n_frames;
#pragma unroll
                for (int m = 0; m < 25; ++m) {
                    const int ia = reflect(i0 + 16 * m, N), ib = reflect(i0 + 16 * m + 1, N);
                    const bool oka = live && static_cast<uint32_t>(ia) < L, okb = live && static_cast<uint32_t>(ib) < L;
                    float xa, xc;  // L > 0 here: sample 0 exists
                    if constexpr (PCM) xa = pcm_sample(xb, oka ? ia : 0, a.scale), xc = pcm_sample(xb, okb ? ib : 0, a.scale);
                    else xa = xb[oka ? ia : 0], xc = xb[okb ? ib : 0];
                    v[m] = make_float2(oka ? xa : 0.f, okb ? xc : 0.f);
                }
            }
#pragma unroll
            for (int m = 0; m < 25; ++m) {
                const float2 w = s_win[m * 8 + j];
                v[m] = make_float2(v[m].x * w.x, v[m].y * w.y);
            }
            dft25(v);  // v[5 c + d] = Y_j[c + 5 d]
            // natural order, the twiddles exp(-2 pi i j k1 / 200), radix 8 over the lanes
            float2 z[25];
#pragma unroll
            for (int c5 = 0; c5 < 5; ++c5)
#pragma unroll
                for (int d = 0; d < 5; ++d) z[c5 + 5 * d] = v[5 * c5 + d];
#pragma unroll
            for (int k1 = 0; k1 < 25; ++k1) {
                float2 y = k1 == 0 ? z[0] : cmul(z[k1], s_tw2[k1 * 8 + j]);
                y = lane_step<4>(y, sg4, tw4);
                y = lane_step<2>(y, sg2, tw2);
                z[k1] = lane_step<1>(y, sg1, make_float2(1.f, 0.f));
            }
            // untangle: 2 X[k] = s - i w d with the partner Z[200 - k]; P = |X|^2
            float *prow = s_prow + f * kPRowPitch;
            {
                const float2 zp = make_float2(wv::bperm(self_addr, z[0].x), wv::bperm(self_addr, z[0].y));
                const float2 s = make_float2(z[0].x + zp.x, z[0].y - zp.y), d = make_float2(z[0].x - zp.x, z[0].y + zp.y);
                const float2 w = s_twn[j];
                const float xr = fmaf(w.y, d.x, fmaf(w.x, d.y, s.x)), xi = fmaf(w.y, d.y, fmaf(-w.x, d.x, s.y));
                prow[25 * K2] = 0.25f * fmaf(xr, xr, xi * xi);
                if (j == 0) {  // bin 200 pairs with Z[0] too: w = -1
                    const float yr = s.x - d.y, yi = s.y + d.x;
                    prow[200] = 0.25f * fmaf(yr, yr, yi * yi);
                }
            }
#pragma unroll
            for (int k1 = 1; k1 < 25; ++k1) {
                const float2 zk = z[k1];
                const float2 zp = make_float2(wv::dpp<kDppHalfMirror>(z[25 - k1].x), wv::dpp<kDppHalfMirror>(z[25 - k1].y));
                const float2 s = make_float2(zk.x + zp.x, zk.y - zp.y), d = make_float2(zk.x - zp.x, zk.y + zp.y);
                const float2 w = s_twn[k1 * 8 + j];
                const float xr = fmaf(w.y, d.x, fmaf(w.x, d.y, s.x)), xi = fmaf(w.y, d.y, fmaf(-w.x, d.x, s.y));
                prow[25 * K2 + k1] = 0.25f * fmaf(xr, xr, xi * xi);
            }
            wv::wave_order();
            // banded mel of frame mf, log10, into the tile; the maximum over the frames that are stored
            const float *pr = s_prow + mf * kPRowPitch;
            const bool counted = tp + static_cast<uint32_t>(mf) < limit;
            for (uint32_t m = static_cast<uint32_t>(mg); m < a.n_mels; m += 8) {
                const int st = s_start[m], n = s_len[m];
                const float *w = s_melw + s_off[m];
                float acc = 0.f;
                for (int q = 0; q < n; ++q) acc = fmaf(w[q], pr[st + q], acc);
                const float l = acc > 1e-10f ? log10f(acc) : kLogFloor;
                s_tile[m * kTilePitch + pass * kPassFrames + mf] = l;
                if (counted) lmax = fmaxf(lmax, l);
            }
            wv::wave_order();
        }

        lmax = wave_max(lmax);
        if (lane == 0) atomicMax(a.keys + c, float_key(lmax));
        // the tile along t: lane -> (mel row, four consecutive frames); frames at or past `limit` are the floor pass's
        float *dst = a.inter + static_cast<size_t>(c) * a.n_mels * a.n_frames;
        const uint32_t tq = t0 + 4u * (lane & 3);
        for (uint32_t m = static_cast<uint32_t>(lane >> 2); m < a.n_mels; m += 16) {
            const float *tr = s_tile + m * kTilePitch + 4 * (lane & 3);
            float *row = dst + static_cast<size_t>(m) * a.n_frames + tq;
            if (tq + 4 <= limit && (reinterpret_cast<uintptr_t>(row) & 15u) == 0) {
                *reinterpret_cast<float4 *>(row) = make_float4(tr[0], tr[1], tr[2], tr[3]);
            } else {
#pragma unroll
                for (uint32_t e = 0; e < 4; ++e)
                    if (tq + e < limit) row[e] = tr[e];
            }
        }
        wv::wave_order();
    }
}

// conv of ss_pad_packed (ss_pad.hip), as the low bits of a word
template <int DT>
__device__ __forceinline__ unsigned conv_bits(float v)
{
    const unsigned u = __float_as_uint(v);
    if constexpr (DT == SS_PAD_F32) {
        return u;
    } else if constexpr (DT == SS_PAD_F16) {
        // the f32 value is rounded before it is converted: without the barrier the compiler folds the caller's fmaf and this conversion
        // into one v_fma_mixlo_f16, which rounds once, and the result is no longer the converted f32 result
        asm volatile("" : "+v"(v));
        const _Float16 h = static_cast<_Float16>(v);
        unsigned short s;
        __builtin_memcpy(&s, &h, sizeof s);
        return s;
    } else {
        if ((u & 0x7fffffffu) > 0x7f800000u) return (u >> 16) | 0x40u;  // NaN stays NaN
        return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
    }
}

__device__ __forceinline__ float floor_scale(float l, float thr) { return fmaf(fmaxf(l, thr), 0.25f, 1.0f); }

// Workgroup (c, y) serves clip c = blockIdx.x with the gridDim.y - 1 others of that clip.  VEC: the clip's block is a whole number of
// 16-byte groups and out is 16-byte aligned (uniform, decided by the launcher): a lane converts and stores one group per step.
template <int DT, bool VEC>
__global__ __launch_bounds__(256) void ss_whisper_floor_kernel(const float *inter, const long long *__restrict__ so, uint32_t dense_len, uint32_t n_frames,
                                                              uint32_t n_mels, const int *__restrict__ keys, void *out)
{
    constexpr unsigned ES = DT == SS_PAD_F32 ? 4 : 2, VE = 16 / ES;
    const uint32_t c = blockIdx.x;
    const Clip<float> clip = clip_of(static_cast<const float *>(nullptr), so, 0, dense_len, n_frames, c);
    const uint32_t limit = first_silent(clip.L, n_frames);
    const float thr = key_float(keys[c]) - 8.0f;
    const uint32_t block = n_mels * n_frames;  // < 2^31 (checked by the host)
    const float *src = inter + static_cast<size_t>(c) * block;
    if constexpr (VEC) {
        uint4 *dst = reinterpret_cast<uint4 *>(static_cast<unsigned char *>(out) + static_cast<size_t>(c) * block * ES);
        const uint32_t groups = block / VE;
        for (uint32_t g = blockIdx.y * 256u + threadIdx.x; g < groups; g += gridDim.y * 256u) {
            const uint32_t e0 = g * VE;
            uint32_t t = e0 % n_frames;
            float v[VE];
            if (t + VE <= limit) {  // all live, one mel row: wide loads
#pragma unroll
                for (unsigned q = 0; q < VE / 4; ++q) {
                    const float4 x4 = *reinterpret_cast<const float4 *>(src + e0 + 4 * q);
                    v[4 * q] = x4.x, v[4 * q + 1] = x4.y, v[4 * q + 2] = x4.z, v[4 * q + 3] = x4.w;
                }
            } else {
#pragma unroll
                for (unsigned q = 0; q < VE; ++q) {
                    v[q] = t < limit ? src[e0 + q] : kLogFloor;
                    if (++t == n_frames) t = 0;
                }
            }
            unsigned w[4];
#pragma unroll
            for (unsigned q = 0; q < 4; ++q) {
                if constexpr (DT == SS_PAD_F32) w[q] = conv_bits<DT>(floor_scale(v[q], thr));
                else w[q] = conv_bits<DT>(floor_scale(v[2 * q], thr)) | (conv_bits<DT>(floor_scale(v[2 * q + 1], thr)) << 16);
            }
            dst[g] = make_uint4(w[0], w[1], w[2], w[3]);
        }
    } else {
        for (uint32_t e = blockIdx.y * 256u + threadIdx.x; e < block; e += gridDim.y * 256u) {
            const uint32_t t = e % n_frames;
            const float r = floor_scale(t < limit ? src[e] : kLogFloor, thr);
            const size_t o = static_cast<size_t>(c) * block + e;
            if constexpr (DT == SS_PAD_F32) static_cast<unsigned *>(out)[o] = conv_bits<DT>(r);
            else static_cast<unsigned short *>(out)[o] = static_cast<unsigned short>(conv_bits<DT>(r));
        }
    }
}

}  // namespace

}  // namespace ss

// The handle: the validated parameters, the table block on the device it was created on, the keys block and a pinned device error word.
struct ss_whisper_config {
    ss_whisper_params params{};
    int device = -1;
    int num_cus = 256;
    float *d_tab = nullptr;
    int *d_keys = nullptr;
    unsigned *h_err = nullptr, *d_err = nullptr;
};

namespace {

using ss::fail;
using ss::hip_fail;

int whisper_pending_error(const ss_whisper_config *cfg)
{
    if (!cfg->h_err || __atomic_load_n(cfg->h_err, __ATOMIC_ACQUIRE) == 0) return SS_OK;
    const unsigned w = __atomic_exchange_n(cfg->h_err, 0u, __ATOMIC_ACQ_REL);
    if (w == 0) return SS_OK;
    return fail(SS_ERR_DEVICE, "a launch on this handle met a packed clip whose sample offsets are inconsistent (error word " + std::to_string(w) +
                                   "): that clip's block is all -1.5 and its length -1");
}

int whisper_ready(const ss_whisper_config *cfg)
{
    int dev = -1;
    const hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return hip_fail(e, "hipGetDevice");
    if (dev != cfg->device) return fail(SS_ERR_ARG, "the handle was created on a different HIP device than the current one");
    return whisper_pending_error(cfg);
}

size_t elem_bytes(int dtype) { return dtype == SS_PAD_F32 ? 4 : 2; }
// the kernels form 160 (t + 16) in 32-bit integers
constexpr size_t kMaxFrames = ((1ull << 31) - 1) / ss::whisper::kHop - 16;

// what needs no device: the sizes, the types and the pointers' alignment (T: float samples, or int16_t -- 16-bit PCM)
template <typename T>
int whisper_check(const ss_whisper_config *cfg, const T *x, size_t n_clips, size_t n_frames, int dtype, const void *work, const void *out)
{
    if (dtype != SS_PAD_F32 && dtype != SS_PAD_F16 && dtype != SS_PAD_BF16) return fail(SS_ERR_ARG, "dtype must be SS_PAD_F32, SS_PAD_F16 or SS_PAD_BF16");
    if (n_frames < 2) return fail(SS_ERR_ARG, "n_frames must be at least 2");
    if (n_frames > kMaxFrames) return fail(SS_ERR_ARG, "n_frames * 160 must stay below 2^31 (with 16 frames to spare)");
    if (n_clips > SS_WHISPER_MAX_CLIPS) return fail(SS_ERR_ARG, "more than SS_WHISPER_MAX_CLIPS clips in one call");
    if (!cfg) return fail(SS_ERR_ARG, "null handle");
    if (static_cast<unsigned long long>(cfg->params.n_mels) * n_frames >= (1ull << 31)) return fail(SS_ERR_ARG, "n_mels * n_frames must be below 2^31");
    if (static_cast<unsigned long long>(n_clips) * ss::whisper::units_per_clip(static_cast<uint32_t>(n_frames)) >= 0xffffffffull)
        return fail(SS_ERR_ARG, "n_clips * ceil(n_frames / 16) must fit the 32-bit unit counter");
    if (!x || !out || (dtype != SS_PAD_F32 && !work)) return fail(SS_ERR_ARG, "null buffer");
    if (reinterpret_cast<uintptr_t>(x) % sizeof(T)) return fail(SS_ERR_ARG, sizeof(T) == 4 ? "x must be 4-byte aligned" : "x must be 2-byte aligned");
    if (reinterpret_cast<uintptr_t>(out) % 16 || (dtype != SS_PAD_F32 && reinterpret_cast<uintptr_t>(work) % 16))
        return fail(SS_ERR_ARG, "out and work must be 16-byte aligned");
    return SS_OK;
}

template <int DT>
hipError_t launch_floor(const float *inter, const long long *so, uint32_t dense_len, uint32_t n_clips, uint32_t n_frames, uint32_t n_mels, const int *keys, void *out,
                        hipStream_t stream)
{
    constexpr unsigned VE = DT == SS_PAD_F32 ? 4 : 8;
    const unsigned long long block = static_cast<unsigned long long>(n_mels) * n_frames;
    const bool vec = block % VE == 0;
    const dim3 grid(n_clips, ss::packed_split(n_clips, (block / (vec ? VE : 1) + 1023) / 1024));
    if (vec) hipLaunchKernelGGL((ss::ss_whisper_floor_kernel<DT, true>), grid, dim3(256), 0, stream, inter, so, dense_len, n_frames, n_mels, keys, out);
    else hipLaunchKernelGGL((ss::ss_whisper_floor_kernel<DT, false>), grid, dim3(256), 0, stream, inter, so, dense_len, n_frames, n_mels, keys, out);
    return hipGetLastError();
}

// the three launches; so == nullptr: dense rows of n_samples with stride ld.  T = int16_t: the PCM build of the middle one (sample k is
// (float)x[k] * scale; the keys and floor kernels never read x)
template <typename T>
int whisper_launch(const ss_whisper_config *cfg, const T *d_x, float scale, size_t n_clips, const int64_t *d_so, size_t n_samples, size_t ld, size_t n_frames,
                   int dtype, void *d_work, void *d_out, int32_t *d_lengths, hipStream_t stream)
{
    constexpr bool PCM = std::is_same_v<T, int16_t>;
    constexpr const char *kName = PCM ? "ss_whisper_c200i" : "ss_whisper_c200";
    using namespace ss::whisper;
    const uint32_t N = static_cast<uint32_t>(n_frames * kHop), nc = static_cast<uint32_t>(n_clips), nf = static_cast<uint32_t>(n_frames);
    const uint32_t dense_len = static_cast<uint32_t>(n_samples < N ? n_samples : N);
    const long long *so = reinterpret_cast<const long long *>(d_so);
    float *inter = dtype == SS_PAD_F32 ? static_cast<float *>(d_out) : static_cast<float *>(d_work);

    hipLaunchKernelGGL(ss::ss_whisper_keys_kernel, dim3((nc + 255) / 256), dim3(256), 0, stream, so, nc, nf, cfg->d_keys, reinterpret_cast<int *>(d_lengths),
                       static_cast<uint32_t>(dense_len / kHop), cfg->d_err);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "ss_whisper_keys_kernel");

    const unsigned long long units = static_cast<unsigned long long>(nc) * units_per_clip(nf);
    const unsigned grid = ss::cu_capped_grid(units, kWaves, cfg->num_cus);
    const ss::UnitSplit sp = ss::split_units(units, grid);
    ss::WhisperArgs<T> a{};
    a.x = d_x;
    a.so = so;
    a.ld = ld;
    a.n_samples = dense_len;
    a.n_clips = nc;
    a.n_frames = nf;
    a.n_mels = cfg->params.n_mels;
    a.tab = cfg->d_tab;
    a.inter = inter;
    a.keys = cfg->d_keys;
    a.q_base = sp.q_base;
    a.q_rem = sp.q_rem;
    a.scale = scale;
    e = ss::launch_kernel(ss::ss_whisper_c200<T>, kName, grid, kWaves, kLdsBytes, stream, nullptr, a);
    if (e != hipSuccess) return hip_fail(e, kName);

    if (dtype == SS_PAD_F32) e = launch_floor<SS_PAD_F32>(inter, so, dense_len, nc, nf, a.n_mels, cfg->d_keys, d_out, stream);
    else if (dtype == SS_PAD_F16) e = launch_floor<SS_PAD_F16>(inter, so, dense_len, nc, nf, a.n_mels, cfg->d_keys, d_out, stream);
    else e = launch_floor<SS_PAD_BF16>(inter, so, dense_len, nc, nf, a.n_mels, cfg->d_keys, d_out, stream);
    if (e != hipSuccess) return hip_fail(e, "ss_whisper_floor_kernel");
    ss::note_kernel(kName);
    return SS_OK;
}

// The device and host forms, once for float samples and once for 16-bit PCM (pcm: the scale; checked first among the data checks,
// every other rule in the float call's order).
template <typename T>
int whisper_dense_device(const ss_whisper_config *cfg, const T *d_x, const float *pcm, size_t batch, size_t n_samples, size_t ld, size_t n_frames, int dtype,
                         void *d_work, void *d_out, hipStream_t stream)
{
    if (pcm)
        if (int rc = ss::check_pcm_scale(*pcm)) return rc;
    if (batch == 0) return SS_OK;
    // a clip without samples reads nothing: any non-null x will do, and ld is not used
    if (int rc = whisper_check(cfg, d_x, batch, n_frames, dtype, d_work, d_out)) return rc;
    if (ld < n_samples) return fail(SS_ERR_ARG, "ld must be at least n_samples");
    if (int rc = whisper_ready(cfg)) return rc;
    return whisper_launch(cfg, d_x, pcm ? *pcm : 1.0f, batch, nullptr, n_samples, ld, n_frames, dtype, d_work, d_out, nullptr, stream);
}

template <typename T>
int whisper_packed_device(const ss_whisper_config *cfg, const T *d_x, const float *pcm, size_t n_clips, const int64_t *d_sample_offsets, size_t n_frames,
                          int dtype, void *d_work, void *d_out, int32_t *d_lengths, hipStream_t stream)
{
    if (pcm)
        if (int rc = ss::check_pcm_scale(*pcm)) return rc;
    if (n_clips == 0) return SS_OK;
    if (int rc = whisper_check(cfg, d_x, n_clips, n_frames, dtype, d_work, d_out)) return rc;
    if (!d_sample_offsets) return fail(SS_ERR_ARG, "null buffer");
    if (reinterpret_cast<uintptr_t>(d_sample_offsets) % 8 || reinterpret_cast<uintptr_t>(d_lengths) % 4)
        return fail(SS_ERR_ARG, "sample_offsets must be 8-byte and lengths 4-byte aligned");
    if (int rc = whisper_ready(cfg)) return rc;
    return whisper_launch(cfg, d_x, pcm ? *pcm : 1.0f, n_clips, d_sample_offsets, 0, 0, n_frames, dtype, d_work, d_out, d_lengths, stream);
}

// host-pointer forms (synchronous): everything on the device for the length of one call; PCM crosses the link as int16
template <typename T>
int whisper_dense_host(const ss_whisper_config *cfg, const T *x, const float *pcm, size_t batch, size_t n_samples, size_t ld, size_t n_frames, int dtype, void *out)
{
    if (pcm)
        if (int rc = ss::check_pcm_scale(*pcm)) return rc;
    if (batch == 0) return SS_OK;
    if (!cfg) return fail(SS_ERR_ARG, "null handle");
    if (dtype != SS_PAD_F32 && dtype != SS_PAD_F16 && dtype != SS_PAD_BF16) return fail(SS_ERR_ARG, "dtype must be SS_PAD_F32, SS_PAD_F16 or SS_PAD_BF16");
    if (!x || !out) return fail(SS_ERR_ARG, "null buffer");
    if (n_frames < 2 || n_frames > kMaxFrames) return fail(SS_ERR_ARG, "n_frames must be at least 2 and n_frames * 160 below 2^31");
    if (ld < n_samples) return fail(SS_ERR_ARG, "ld must be at least n_samples");
    if (!ss::have_device()) return ss::no_device("hot path");
    const size_t in_samples = (batch - 1) * ld + n_samples, block = batch * cfg->params.n_mels * n_frames;
    ss::HostStage st(pcm ? "ss_whisper_log_mel_i16" : "ss_whisper_log_mel");
    const T *d_in = st.up(x, in_samples * sizeof(T));
    void *d_out = st.room<void>(block * elem_bytes(dtype));
    void *d_work = dtype != SS_PAD_F32 ? st.room<void>(block * sizeof(float)) : nullptr;
    if (st.ok()) st.ran(whisper_dense_device(cfg, d_in, pcm, batch, n_samples, ld, n_frames, dtype, d_work, d_out, nullptr));
    st.sync();
    st.down(out, d_out, block * elem_bytes(dtype));
    return st.status();
}

template <typename T>
int whisper_packed_host(const ss_whisper_config *cfg, const T *x, const float *pcm, size_t n_clips, const int64_t *sample_offsets, size_t n_frames, int dtype,
                        void *out, int32_t *lengths)
{
    if (pcm)
        if (int rc = ss::check_pcm_scale(*pcm)) return rc;
    if (n_clips == 0) return SS_OK;
    if (!cfg) return fail(SS_ERR_ARG, "null handle");
    if (dtype != SS_PAD_F32 && dtype != SS_PAD_F16 && dtype != SS_PAD_BF16) return fail(SS_ERR_ARG, "dtype must be SS_PAD_F32, SS_PAD_F16 or SS_PAD_BF16");
    if (!x || !out || !sample_offsets) return fail(SS_ERR_ARG, "null buffer");
    if (n_frames < 2 || n_frames > kMaxFrames) return fail(SS_ERR_ARG, "n_frames must be at least 2 and n_frames * 160 below 2^31");
    // the host sees the table: the samples that come up are those of its good entries (a bad entry is contained on the device)
    int64_t top = 0;
    for (size_t b = 0; b < n_clips; ++b)
        if (sample_offsets[b] >= 0 && sample_offsets[b + 1] >= sample_offsets[b] && sample_offsets[b + 1] > top) top = sample_offsets[b + 1];
    if (!ss::have_device()) return ss::no_device("hot path");
    const size_t in_samples = static_cast<size_t>(top), block = n_clips * cfg->params.n_mels * n_frames;
    ss::HostStage st(pcm ? "ss_whisper_log_mel_packed_i16" : "ss_whisper_log_mel_packed");
    const T *d_in = st.up(x, in_samples * sizeof(T));
    void *d_out = st.room<void>(block * elem_bytes(dtype));
    void *d_work = dtype != SS_PAD_F32 ? st.room<void>(block * sizeof(float)) : nullptr;
    const int64_t *d_so = st.up(sample_offsets, (n_clips + 1) * sizeof(int64_t));
    int32_t *d_len = st.room<int32_t>(n_clips * sizeof(int32_t));
    if (st.ok()) st.ran(whisper_packed_device(cfg, d_in, pcm, n_clips, d_so, n_frames, dtype, d_work, d_out, d_len, nullptr));
    st.sync();
    st.down(out, d_out, block * elem_bytes(dtype));
    if (lengths) st.down(lengths, d_len, n_clips * sizeof(int32_t));
    return st.ok() ? whisper_pending_error(cfg) : st.status();
}

}  // namespace

extern "C" {

int ss_whisper_config_create(const ss_whisper_params *p, ss_whisper_config **out)
{
    if (!p || !out) return fail(SS_ERR_ARG, "null argument");
    *out = nullptr;
    if (int rc = ss::whisper_validate(*p)) return rc;
    std::vector<float> tab;
    ss::build_whisper_tables(*p, tab);
    if (!ss::have_device()) return ss::no_device("hot path");
    std::unique_ptr<ss_whisper_config> cfg(new ss_whisper_config());
    cfg->params = *p;
    hipError_t e = hipGetDevice(&cfg->device);
    hipDeviceProp_t prop;
    if (e == hipSuccess) e = hipGetDeviceProperties(&prop, cfg->device);
    if (e == hipSuccess) cfg->num_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&cfg->d_tab), tab.size() * sizeof(float));
    if (e == hipSuccess) e = hipMemcpy(cfg->d_tab, tab.data(), tab.size() * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&cfg->d_keys), static_cast<size_t>(SS_WHISPER_MAX_CLIPS) * sizeof(int));
    void *hp = nullptr, *dp = nullptr;
    if (e == hipSuccess) e = hipHostMalloc(&hp, 64, hipHostMallocMapped);
    if (e == hipSuccess) {
        std::memset(hp, 0, 64);
        cfg->h_err = static_cast<unsigned *>(hp);
        e = hipHostGetDevicePointer(&dp, hp, 0);
    }
    if (e != hipSuccess) {
        ss_whisper_config_destroy(cfg.release());
        return hip_fail(e, "ss_whisper_config_create");
    }
    cfg->d_err = static_cast<unsigned *>(dp);
    *out = cfg.release();
    return SS_OK;
}

void ss_whisper_config_destroy(ss_whisper_config *cfg)
{
    if (!cfg) return;
    if (cfg->d_tab) (void)hipFree(cfg->d_tab);
    if (cfg->d_keys) (void)hipFree(cfg->d_keys);
    if (cfg->h_err) (void)hipHostFree(cfg->h_err);
    delete cfg;
}

int ss_whisper_config_params(const ss_whisper_config *cfg, ss_whisper_params *out)
{
    if (!cfg || !out) return fail(SS_ERR_ARG, "null argument");
    *out = cfg->params;
    return SS_OK;
}

int ss_whisper_config_device_status(const ss_whisper_config *cfg)
{
    if (!cfg) return fail(SS_ERR_ARG, "null handle");
    return whisper_pending_error(cfg);
}

int ss_whisper_log_mel_device(const ss_whisper_config *cfg, const float *d_x, size_t batch, size_t n_samples, size_t ld, size_t n_frames, int dtype, void *d_work,
                              void *d_out, void *stream)
{
    return whisper_dense_device(cfg, d_x, nullptr, batch, n_samples, ld, n_frames, dtype, d_work, d_out, static_cast<hipStream_t>(stream));
}

int ss_whisper_log_mel_packed_device(const ss_whisper_config *cfg, const float *d_x, size_t n_clips, const int64_t *d_sample_offsets, size_t n_frames, int dtype,
                                     void *d_work, void *d_out, int32_t *d_lengths, void *stream)
{
    return whisper_packed_device(cfg, d_x, nullptr, n_clips, d_sample_offsets, n_frames, dtype, d_work, d_out, d_lengths, static_cast<hipStream_t>(stream));
}

int ss_whisper_log_mel(const ss_whisper_config *cfg, const float *x, size_t batch, size_t n_samples, size_t ld, size_t n_frames, int dtype, void *out)
{
    return whisper_dense_host(cfg, x, nullptr, batch, n_samples, ld, n_frames, dtype, out);
}

int ss_whisper_log_mel_packed(const ss_whisper_config *cfg, const float *x, size_t n_clips, const int64_t *sample_offsets, size_t n_frames, int dtype, void *out,
                              int32_t *lengths)
{
    return whisper_packed_host(cfg, x, nullptr, n_clips, sample_offsets, n_frames, dtype, out, lengths);
}

// 16-bit PCM: sample k is (float)x[k] * scale
int ss_whisper_log_mel_i16_device(const ss_whisper_config *cfg, const int16_t *d_x, size_t batch, size_t n_samples, size_t ld, float scale, size_t n_frames,
                                  int dtype, void *d_work, void *d_out, void *stream)
{
    return whisper_dense_device(cfg, d_x, &scale, batch, n_samples, ld, n_frames, dtype, d_work, d_out, static_cast<hipStream_t>(stream));
}

int ss_whisper_log_mel_packed_i16_device(const ss_whisper_config *cfg, const int16_t *d_x, size_t n_clips, const int64_t *d_sample_offsets, float scale,
                                         size_t n_frames, int dtype, void *d_work, void *d_out, int32_t *d_lengths, void *stream)
{
    return whisper_packed_device(cfg, d_x, &scale, n_clips, d_sample_offsets, n_frames, dtype, d_work, d_out, d_lengths, static_cast<hipStream_t>(stream));
}

int ss_whisper_log_mel_i16(const ss_whisper_config *cfg, const int16_t *x, size_t batch, size_t n_samples, size_t ld, float scale, size_t n_frames, int dtype,
                           void *out)
{
    return whisper_dense_host(cfg, x, &scale, batch, n_samples, ld, n_frames, dtype, out);
}

int ss_whisper_log_mel_packed_i16(const ss_whisper_config *cfg, const int16_t *x, size_t n_clips, const int64_t *sample_offsets, float scale, size_t n_frames,
                                  int dtype, void *out, int32_t *lengths)
{
    return whisper_packed_host(cfg, x, &scale, n_clips, sample_offsets, n_frames, dtype, out, lengths);
}

}  // extern "C"
