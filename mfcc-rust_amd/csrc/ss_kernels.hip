// HIP kernels for the speechsauce hot path on gfx950 (MI355X, wave64).
//
// ss_front_generic<LOG2C>: framing -> (pre-emphasis, window) -> R2C FFT -> magnitude/power ->
// sparse mel -> log -> DCT-II, one launch, any power-of-two fft_points in [32, 4096].
// ss_front_generic<LOG2C, BLU, VarlenArgs> (reported as ss_front_generic_varlen<LOG2C>): the same MFCC / mfe path over packed
// clips of different lengths (VarlenArgs, ss_device.h).
// ss_front_generic<LOG2C, BLU, StreamArgs> (reported as ss_front_generic_stream<LOG2C>): the STFT / mel path with a carried state
// per stream (StreamArgs, ss_device.h); ss_stream_advance moves the state on behind it.
// ss_front_generic<LOG2C, BLU, FrameStreamArgs> (reported as ss_front_generic_fstream<LOG2C>): the MFCC / mfe path with a carried
// state per stream (FrameStreamArgs, ss_device.h): frames and pre-emphasis taps before the chunk read the stream's state.
// ss_front_generic<LOG2C, BLU, FrameStreamPackedArgs> (reported as ss_front_generic_fstreamp<LOG2C>): the same over a pool of stream
// states -- packed chunks of different hop counts, each on the pool row its entry names (FrameStreamPackedArgs, ss_device.h);
// ss_stream_advance_packed moves the named pool rows on behind it.
// ss_front_generic<LOG2C, BLU, FrameStreamPackedPcmArgs> (reported as ss_front_generic_fstreampi<LOG2C>): that pool fed signed
// 16-bit PCM -- a chunk sample or pre-emphasis tap is (float)int16 * scale (FrameStreamPackedPcmArgs, ss_device.h), the state stays
// float; ss_stream_advance_packed_i16 moves the named pool rows on behind it.
// ss_front_generic<LOG2C, BLU, BatchPcmArgs> / <LOG2C, BLU, VarlenPcmArgs> (reported as ss_front_generic_i16<LOG2C> /
// ss_front_generic_varleni<LOG2C>): the equal-length and the packed MFCC / mfe path fed signed 16-bit PCM -- every sample or
// pre-emphasis tap is (float)int16 * scale (BatchPcmArgs / VarlenPcmArgs, ss_device.h).
// ss_front_generic<LOG2C, BLU, VarRowsArgs> (reported as ss_front_generic_varrows<LOG2C>): the STFT / mel path over packed clips of
// different lengths (VarRowsArgs, ss_device.h), handed out in tiles of packed rows.
// ss_front_generic<LOG2C, BLU, StftStreamPackedArgs> (reported as ss_front_generic_streamp<LOG2C>): the STFT / mel path over a pool
// of stream states -- the packed-rows tiles with every row on the pool row its entry names (StftStreamPackedArgs, ss_device.h);
// ss_stream_advance_packed moves the named pool rows on behind it.
// ss_front_generic<LOG2C, BLU, VarRowsArgs, BatchPcmArgs> / <LOG2C, BLU, StftStreamPackedArgs, BatchPcmArgs> (reported as
// ss_front_generic_varrowsi<LOG2C> / ss_front_generic_streampi<LOG2C>), and ss_front_generic_i16 with mel or stft output: the three
// STFT / mel layouts fed signed 16-bit PCM -- a clip or chunk sample is (float)int16 * scale, the pool rows stay float
// (ss_stream_advance_packed_i16 moves them on).
//
//   * A real frame of N = 2C samples is packed as C complex points z[n] = x[2n] + i x[2n+1]
//     and transformed by a Stockham autosort FFT whose butterflies live in registers: every
//     thread owns 16 complex points, so C/16 threads cooperate on a frame and a 256-thread
//     workgroup carries 4096/C frames per pass.  Radix plan: 16, then 16, then C/256 (or 16
//     then C/16 for C < 256): at most three LDS exchanges per frame.
//   * The LDS exchange buffer uses the padded index i + (i >> 4): the stride-16 scatter of the
//     first pass then lands on distinct banks for the 16 lanes of a ds_write_b64 group.
//   * X[k] is untangled from Z[k], Z[C-k] pairwise, magnitudes go to an LDS row, the mel bank is
//     a banded reduction over that row (CSR-like start/len/weights; no MFMA - at most two
//     filters touch a bin), and the DCT-II is a [n_ceps x n_filters] table product.
//   * HBM traffic: the clip samples once (neighbouring frames re-read them through L1/L2) and
//     the features once.
//
//   * fft_points that are not a power of two (the reference takes any length) run the chirp-z (Bluestein) build BLU of the
//     same kernel: a[n] = x[n] c[n], c[n] = exp(-i pi n^2 / N); A = FFT_L(a) with the complex L-point transform above
//     (L >= N + N/2 a power of two); A .* FFT_L(conj c) (host table); the inverse transform as conj FFT_L(conj .);
//     X[k] = c[k] (a * conj c)[k] / L for the N/2 + 1 bins.  Two L-point transforms per frame instead of one N/2-point one:
//     a completeness path, not a fast one.
//
// Reference semantics (file:line relative to the reference checkout) are cited at each stage.
#include <cstdio>

#include "ss_device.h"
#include "ss_fft_reg.h"

namespace ss {

namespace {

constexpr float kEps = 1.1920929e-7f;  // f32::EPSILON, functions.rs:70
constexpr int kBlock = 256;

__device__ __forceinline__ int phys(int i) { return i + (i >> 4); }

// ln(x) from v_log_f32 (log2) with the denormal pre-scale the library form uses; ~1 ulp of log2.
__device__ __forceinline__ float fast_ln(float x)
{
    const bool tiny = x < 1.17549435e-38f;
    const float l = __builtin_amdgcn_logf(tiny ? x * 4294967296.f : x);
    return (l - (tiny ? 32.f : 0.f)) * 0.69314718055994530942f;
}

// Hand-off between the threads of ONE frame.  A frame has C/16 threads; up to 64 of them sit in one wave, whose LDS
// operations execute in order, so only the compiler has to be kept from reordering (as in the dedicated kernels).  Frames
// that span waves (fft_points 4096) need the workgroup barrier.
template <int LOG2C>
__device__ __forceinline__ void frame_sync()
{
    if constexpr ((1 << LOG2C) / 16 <= 64) {
        asm volatile("" ::: "memory");
        __builtin_amdgcn_wave_barrier();
    } else {
        __syncthreads();
    }
}

// One Stockham pass of radix R with sub-transform length NS already done, on a frame of C points
// held 16 per thread.  `j` is the thread index within the frame (TPF = C/16 threads).
// Loads happen before the barrier-separated stores, so the pass works in place.
template <int LOG2C, int R, int NS, bool kLoad>
__device__ __forceinline__ void stockham_pass(float2 *zbuf, int j, const float2 *__restrict__ tw_c, float2 (&v)[16])
{
    constexpr int C = 1 << LOG2C;
    constexpr int TPF = C / 16 > 0 ? C / 16 : 1;
    constexpr int NB = 16 / R;  // butterflies per thread
    constexpr int STRIDE = C / R;
    if (kLoad) {
        frame_sync<LOG2C>();
#pragma unroll
        for (int q = 0; q < NB; ++q) {
            const int b = j + TPF * q;
#pragma unroll
            for (int r = 0; r < R; ++r) v[q * R + r] = zbuf[phys(b + r * STRIDE)];
        }
    }
#pragma unroll
    for (int q = 0; q < NB; ++q) {
        const int b = j + TPF * q;
        if (NS > 1) {
            const int k = b & (NS - 1);
            constexpr int TWS = C / (NS * R);  // exp(-2 pi i k r / (NS R)) = tw_c[k r TWS]
#pragma unroll
            for (int r = 1; r < R; ++r) v[q * R + r] = cmul(v[q * R + r], tw_c[k * r * TWS]);
        }
        fft_reg<R>(&v[q * R]);
    }
    frame_sync<LOG2C>();
#pragma unroll
    for (int q = 0; q < NB; ++q) {
        const int b = j + TPF * q;
        const int k = b & (NS - 1);
        const int j0 = (b - k) * R + k;
#pragma unroll
        for (int r = 0; r < R; ++r) zbuf[phys(j0 + r * NS)] = v[q * R + r];
    }
}

// Full C-point complex FFT of the frame whose pass-1 inputs are already in v
// (v[e] = z[j + e * TPF]).  Result: natural order Z[k] at zbuf[phys(k)] (after a barrier).
template <int LOG2C>
__device__ __forceinline__ void frame_fft(float2 *zbuf, int j, const float2 *__restrict__ tw_c, float2 (&v)[16])
{
    constexpr int C = 1 << LOG2C;
    stockham_pass<LOG2C, 16, 1, false>(zbuf, j, tw_c, v);
    if constexpr (LOG2C >= 8) {
        stockham_pass<LOG2C, 16, 16, true>(zbuf, j, tw_c, v);
        if constexpr (LOG2C > 8) stockham_pass<LOG2C, C / 256, 256, true>(zbuf, j, tw_c, v);
    } else if constexpr (LOG2C > 4) {
        stockham_pass<LOG2C, C / 16, 16, true>(zbuf, j, tw_c, v);
    }
    frame_sync<LOG2C>();
}

template <int LOG2C>
struct Geo {
    static constexpr int C = 1 << LOG2C;
    static constexpr int N = 2 * C;
    static constexpr int F = C + 1;
    static constexpr int TPF = C / 16;           // threads per frame
    static constexpr int FPB = kBlock / TPF;     // frames per workgroup pass
    static constexpr int ZLEN = C + C / 16;      // padded complex buffer
    static constexpr int PLEN = (F + 3) & ~3;    // magnitude row
};

// Untangle Z -> X (real-input FFT of length N from the packed C-point FFT), scale, take
// magnitude / power, store the row to LDS and return this thread's partial row sum.
//   X[k]   = 1/2 [ (Z[k] + conj Z[C-k]) - i w (Z[k] - conj Z[C-k]) ],  w = exp(-2 pi i k / N)
//   X[C-k] = conj( 1/2 [ (Z[k] + conj Z[C-k]) + i w (Z[k] - conj Z[C-k]) ] )
template <int LOG2C>
__device__ __forceinline__ float untangle_row(const float2 *zbuf, float *prow, float2 *stft_row, int j,
                                              const FrontArgs &a, bool mel_mode, bool active)
{
    using G = Geo<LOG2C>;
    float esum = 0.0f;
    for (int k = j; k <= G::C / 2; k += G::TPF) {
        const float2 zk = zbuf[phys(k)];
        const float2 zc = zbuf[phys((G::C - k) & (G::C - 1))];
        const float2 w = a.tw_n[k];
        const float2 s = make_float2(0.5f * (zk.x + zc.x), 0.5f * (zk.y - zc.y));  // E[k]
        const float2 d = make_float2(0.5f * (zk.x - zc.x), 0.5f * (zk.y + zc.y));
        // -i w d  with d = (Z[k] - conj Z[C-k])/2
        const float2 wd = cmul(w, d);
        const float2 t = make_float2(wd.y, -wd.x);
        float2 xa = cadd(s, t);           // X[k]
        float2 xb = csub(s, t);           // conj X[C-k]
        xb.y = -xb.y;
        float pa, pb;
        if (mel_mode) {
            // functions.rs:166-169 (* wnorm) then feature.rs:164 (abs().powi(2))
            xa.x *= a.scale; xa.y *= a.scale;
            xb.x *= a.scale; xb.y *= a.scale;
            pa = xa.x * xa.x + xa.y * xa.y;
            pb = xb.x * xb.x + xb.y * xb.y;
            if (stft_row && active) {
                stft_row[k] = xa;
                if (k != G::C / 2) stft_row[G::C - k] = xb;
            }
        } else {
            // processing.rs:168 sqrt(re^2 + im^2), :180 * (1/N)
            const float ma = __builtin_amdgcn_sqrtf(xa.x * xa.x + xa.y * xa.y);
            const float mb = __builtin_amdgcn_sqrtf(xb.x * xb.x + xb.y * xb.y);
            pa = a.spectrum_exponent == 2 ? a.scale * (ma * ma) : a.scale * ma;
            pb = a.spectrum_exponent == 2 ? a.scale * (mb * mb) : a.scale * mb;
        }
        prow[k] = pa;
        esum += pa;
        if (k != G::C / 2) {
            prow[G::C - k] = pb;
            esum += pb;
        }
    }
    return esum;
}

// Chirp-z epilogue: zbuf holds FFT_L(conj(A .* B)) in natural order; X[k] = c[k] conj(zbuf[k]) / L for k < F.  Same scaling,
// magnitude / power and stft output as untangle_row.
template <int LOG2C>
__device__ __forceinline__ float blu_row(const float2 *zbuf, float *prow, float2 *stft_row, int j, const FrontArgs &a, bool mel_mode,
                                         bool active, int F)
{
    using G = Geo<LOG2C>;
    const float inv_l = 1.0f / static_cast<float>(G::C);
    float esum = 0.0f;
    for (int k = j; k < F; k += G::TPF) {
        const float2 w = zbuf[phys(k)];
        const float2 c = a.blu_c[k];
        float2 xa = cmul(c, make_float2(w.x * inv_l, -w.y * inv_l));
        float pa;
        if (mel_mode) {
            xa.x *= a.scale;
            xa.y *= a.scale;
            pa = xa.x * xa.x + xa.y * xa.y;
            if (stft_row && active) stft_row[k] = xa;
        } else {
            const float ma = __builtin_amdgcn_sqrtf(xa.x * xa.x + xa.y * xa.y);
            pa = a.spectrum_exponent == 2 ? a.scale * (ma * ma) : a.scale * ma;
        }
        prow[k] = pa;
        esum += pa;
    }
    return esum;
}

// After the forward transform of the chirped frame: conj(A[k] B[k]) back into the pass-1 registers (v[e] = z[j + e TPF]) and
// the second transform.  The first pass of frame_fft stores only after a frame-wide sync, so the reads here are safe.
template <int LOG2C>
__device__ __forceinline__ void blu_convolve(float2 *zbuf, int j, const FrontArgs &a, float2 (&v)[16])
{
    using G = Geo<LOG2C>;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const int k = j + e * G::TPF;
        const float2 p = cmul(zbuf[phys(k)], a.blu_b[k]);
        v[e] = make_float2(p.x, -p.y);
    }
    frame_fft<LOG2C>(zbuf, j, a.tw_c, v);
}

// Banded mel reduction of one magnitude row (feature.rs:229 / :173 restricted to the non-zero taps).
__device__ __forceinline__ float mel_dot(const float *prow, const FrontArgs &a, int m)
{
    const int st = a.f_start[m], ln = a.f_len[m];
    const float *w = a.f_w + a.f_off[m];
    float s = 0.0f;
    for (int i = 0; i < ln; ++i) s = fmaf(w[i], prow[st + i], s);
    return s;
}

// VAR: packed variable-length clips (launch_front_generic_varlen): the flat frame index is the output row, and the clip / frame
// split, the clip's samples, its length, its literal-framing mode and its DCT scales come from the offset tables (VarlenArgs).
// STREAM: the STFT / mel path of launch_front_generic_stream -- a window sample before the chunk comes from the stream's state.
// FSTREAM: the MFCC / mfe path of launch_front_generic_frame_stream -- clip = stream, frame = row of this call; row t starts at chunk
// sample t * step - lead, and a frame sample or pre-emphasis tap before the chunk comes from the stream's state (no circular wrap).
// FSP: FSTREAM over a pool of states (launch_front_generic_frame_stream_packed) -- the flat frame index is the packed output row, and
// the row's entry (its chunk, its row within the chunk, its pool row) comes from the device tables (FrameStreamPackedArgs).
// FSPI: FSP with the chunks as 16-bit PCM (FrameStreamPackedPcmArgs: its entry block is FSP's; state reads are unchanged).
// EQI / VARI: the equal-length layout / VAR with the samples as 16-bit PCM (BatchPcmArgs / VarlenPcmArgs: VARI's tables are VAR's).
// A BatchPcmArgs behind a VarRowsArgs or a StftStreamPackedArgs: VARR / SPR with the clips / chunks as 16-bit PCM (state reads unchanged).
// VARR: the STFT / mel path of launch_front_generic_varrows -- a workgroup visit is a tile of packed rows, every row finds its own
// clip; the transposed mel flush writes each row into its clip's [M x R_b] block.
// SPR: VARR's tiles over the entries of a ragged streaming call (launch_front_generic_stream_packed) -- a row's entry (its chunk, its
// row within the chunk, its pool row) comes from the device tables (StftStreamPackedArgs), its window as in STREAM.
// (V: empty, one VarlenArgs, one StreamArgs, one FrameStreamArgs, one FrameStreamPackedArgs, one FrameStreamPackedPcmArgs, one
// BatchPcmArgs, one VarlenPcmArgs, one VarRowsArgs or one StftStreamPackedArgs, the last two also with a BatchPcmArgs behind them -- an empty pack leaves the argument block of the equal-length builds exactly as it was)
// DB (a DbArgs last in the pack: behind nothing, a BatchPcmArgs, a VarRowsArgs or a VarRowsArgs and a BatchPcmArgs): the mel output of
// the STFT / mel path in decibels -- a mel value is converted where the tile is filled (the flush is unchanged), the largest value of
// a row goes through the slot's `red` words to one atomicMax on the row's clip (ss_log_mel_spectrogram*, DbArgs in ss_device.h).
template <int LOG2C, bool BLU, typename... V>
__global__ __launch_bounds__(kBlock) void ss_front_generic(const FrontArgs a, const V... vargs)
{
    constexpr bool PCMX = (std::is_same_v<V, BatchPcmArgs> || ...);  // the layout's samples are 16-bit PCM at bpi->x
    constexpr bool VARI = (std::is_same_v<V, VarlenPcmArgs> || ...);
    constexpr bool VAR = VARI || (std::is_same_v<V, VarlenArgs> || ...);
    constexpr bool STREAM = (std::is_same_v<V, StreamArgs> || ...);
    constexpr bool FSPI = (std::is_same_v<V, FrameStreamPackedPcmArgs> || ...);
    constexpr bool FSP = FSPI || (std::is_same_v<V, FrameStreamPackedArgs> || ...);
    constexpr bool FSTREAM = FSP || (std::is_same_v<V, FrameStreamArgs> || ...);
    constexpr bool VARR = (std::is_same_v<V, VarRowsArgs> || ...);
    constexpr bool SPR = (std::is_same_v<V, StftStreamPackedArgs> || ...);
    constexpr bool EQI = PCMX && !VARR && !SPR;
    constexpr bool DB = (std::is_same_v<V, DbArgs> || ...);
    static_assert(!DB || !(VAR || STREAM || FSTREAM || SPR), "the dB builds are the equal-length and the packed-rows mel builds");
    [[maybe_unused]] const DbArgs *db = pack_arg<DbArgs>(vargs...);
    [[maybe_unused]] const StftStreamPackedArgs *sp = pack_arg<StftStreamPackedArgs>(vargs...);
    [[maybe_unused]] const VarRowsArgs *ra = pack_arg<VarRowsArgs>(vargs...);
    [[maybe_unused]] const BatchPcmArgs *bpi = pack_arg<BatchPcmArgs>(vargs...);
    [[maybe_unused]] const VarlenPcmArgs *vpi = pack_arg<VarlenPcmArgs>(vargs...);
    [[maybe_unused]] const VarlenArgs *va = pack_arg<VarlenArgs>(vargs...);
    if constexpr (VARI) va = &vpi->v;
    [[maybe_unused]] const StreamArgs *sa = pack_arg<StreamArgs>(vargs...);
    [[maybe_unused]] const FrameStreamArgs *fa = pack_arg<FrameStreamArgs>(vargs...);
    [[maybe_unused]] const FrameStreamPackedPcmArgs *fpi = pack_arg<FrameStreamPackedPcmArgs>(vargs...);
    [[maybe_unused]] const FrameStreamPackedArgs *fp = pack_arg<FrameStreamPackedArgs>(vargs...);
    if constexpr (FSPI) fp = &fpi->e;
    using G = Geo<LOG2C>;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const int tid = threadIdx.x;
    const int slot = tid / G::TPF;  // frame slot within the workgroup pass
    const int j = tid % G::TPF;     // thread within the frame

    const int M = static_cast<int>(a.n_filters);
    const int mpad = (M + 3) & ~3;
    // per-slot LDS carve: zbuf | prow | frow | red
    const size_t slot_bytes = sizeof(float2) * G::ZLEN + sizeof(float) * (G::PLEN + mpad + G::TPF + 4);
    unsigned char *sbase = smem_raw + slot_bytes * slot;
    float2 *zbuf = reinterpret_cast<float2 *>(sbase);
    float *prow = reinterpret_cast<float *>(sbase + sizeof(float2) * G::ZLEN);
    float *frow = prow + G::PLEN;
    float *red = frow + mpad;
    // MEL mode: transposed output tile [M][rows_tile + 1] after all slots
    float *tile = reinterpret_cast<float *>(smem_raw + slot_bytes * G::FPB);

    const bool mel_mode = DB || STREAM || VARR || SPR || (!VAR && !FSTREAM && (a.out_kind == OUT_MEL || a.out_kind == OUT_STFT));
    const int F = BLU ? static_cast<int>(a.blu_n / 2 + 1) : G::F;  // bins per row

    if (!mel_mode) {
        // ---------------- MFCC / MFE / power-spectrum path: flat list of B*T frames ----------------
        if constexpr (VAR) varlen_check_clips(*va, a.flen, a.step, blockIdx.x * kBlock + tid, gridDim.x * kBlock);
        if constexpr (FSP) stream_check_entries(*fp, blockIdx.x * kBlock + tid, gridDim.x * kBlock);
        unsigned long long total = static_cast<unsigned long long>(a.batch) * a.n_frames;
        if constexpr (VAR) total = va->total_frames;
        if constexpr (FSP) total = fp->total_rows;
        const unsigned long long groups = (total + G::FPB - 1) / G::FPB;
        for (unsigned long long g = blockIdx.x; g < groups; g += gridDim.x) {
            const unsigned long long gf = g * G::FPB + slot;
            bool active = gf < total;
            const float *xc;
            [[maybe_unused]] const int16_t *xi = nullptr;  // FSPI: the entry's chunk; EQI / VARI: the clip
            unsigned t;
            unsigned n_samples = a.n_samples;
            int frame_mode = a.frame_mode;
            float dct_scale_k = a.dct_scale_k, dct_scale_00 = a.dct_scale_00;
            [[maybe_unused]] const float *srow = nullptr;  // FSTREAM: the stream's state, indexed from its end (sample p < 0 is srow[p])
            if constexpr (VAR) {
                // rows past the last clip (a larger output block) are left alone; rows of an inconsistent clip are skipped
                const VarClip c = varlen_clip(*va, a.flen, a.step, active ? offset_find(va->fo, va->n_clips, static_cast<long long>(gf)) : 0u);
                active = active && c.ok && static_cast<long long>(gf) >= c.f0 && static_cast<long long>(gf) - c.f0 < static_cast<long long>(c.T);
                t = active ? static_cast<unsigned>(static_cast<long long>(gf) - c.f0) : 0u;
                if constexpr (VARI) {
                    xc = nullptr;
                    xi = vpi->x + (active ? c.s0 : 0ll);
                } else {
                    xc = a.x + (active ? c.s0 : 0ll);
                }
                n_samples = active ? c.n : 1u;
                // processing.rs:110-120 as written, with the clip's own frame count
                if (va->framing == SS_FRAMING_LITERAL) frame_mode = c.T > 2u ? FRAME_ZERO : FRAME_FIRST;
                if (!va->dct_ortho) varlen_dct_scales(*va, c.T, a.n_filters, dct_scale_k, dct_scale_00);
            } else if constexpr (FSP) {
                // rows past the last entry (a larger output block) are left alone; rows of an inconsistent entry are skipped
                const unsigned g32 = static_cast<unsigned>(gf);
                const StreamEntry en = stream_entry(*fp, active ? offset_find(fp->ro, fp->n_active, g32) : 0u);
                active = active && en.ok && static_cast<long long>(gf) >= en.r0 && static_cast<long long>(gf) - en.r0 < static_cast<long long>(en.R);
                t = active ? static_cast<unsigned>(static_cast<long long>(gf) - en.r0) : 0u;
                if constexpr (FSPI) {
                    xc = nullptr;
                    xi = fpi->x + (active ? en.s0 : 0ll);
                } else {
                    xc = a.x + (active ? en.s0 : 0ll);
                }
                if (active && fp->state_len) srow = fp->pool + static_cast<unsigned long long>(en.slot) * fp->state_len + fp->state_len;
            } else {
                const unsigned gf32 = static_cast<unsigned>(gf);  // launch_one rejects batches with >= 2^32 frames
                const unsigned clip = active ? gf32 / a.n_frames : 0u;
                t = active ? gf32 - clip * a.n_frames : 0u;
                if constexpr (EQI) {
                    xc = nullptr;
                    xi = bpi->x + static_cast<unsigned long long>(clip) * a.ld;
                } else {
                    xc = a.x + static_cast<unsigned long long>(clip) * a.ld;
                }
                if constexpr (FSTREAM) srow = fa->state + static_cast<unsigned long long>(clip) * fa->state_len + fa->state_len;
            }
            // stack_frames (processing.rs:65-129, contract framing) + zero pad to N (:147-156)
            const unsigned base = (frame_mode == FRAME_NORMAL || frame_mode == FRAME_PADDED) ? t * a.step : 0u;
            const unsigned lim = frame_mode == FRAME_ZERO ? 0u : (frame_mode == FRAME_FIRST ? (a.flen & ~1u) : a.flen);
            // sample i of the frame after framing, fused pre-emphasis and the optional window (zero beyond the frame)
            auto sample = [&](unsigned i) -> float {
                float val = 0.0f;
                if constexpr (FSTREAM) {
                    // the stream's samples s[p], p = t * step - lead + i, with zeros before its start (the zeroed state);
                    // pre-emphasis y[p] = s[p] - c s[p - sh] reaches back into the state, never round the chunk
                    if (active && i < a.flen) {
                        int lead;
                        if constexpr (FSP) lead = fp->lead;
                        else lead = fa->lead;
                        const long long p = static_cast<long long>(t) * a.step - lead + i;
                        // the chunk's sample k (FSPI: int16 times the power-of-two scale, exact)
                        auto chunk = [&](long long k) -> float {
                            if constexpr (FSPI) return pcm_sample(xi, k, fpi->scale);
                            else return xc[k];
                        };
                        val = p < 0 ? srow[p] : chunk(p);
                        if (a.preemph != 0.0f) {
                            const long long q = p - static_cast<long long>(a.preemph_shift);
                            val -= a.preemph * (q < 0 ? srow[q] : chunk(q));
                        }
                        if (a.window) val *= a.window[i];
                    }
                    return val;
                }
                if (active && i < lim) {
                    unsigned idx = base + i;
                    // FRAME_PADDED (stack_frames zero_padding = true, processing.rs:85-97): zeros past the signal
                    bool inside = frame_mode != FRAME_PADDED || idx < n_samples;
                    if (frame_mode == FRAME_CENTER) {
                        // librosa center=True: the frame is centred on t*step; outside the clip np.pad 'reflect'
                        // (mirror without repeating the edge sample) or zeros
                        long long pos = static_cast<long long>(t) * a.step + i - a.flen / 2;
                        const long long ns = n_samples;
                        if (pos < 0 || pos >= ns) {
                            if (a.pad_reflect) pos = pos < 0 ? -pos : 2 * (ns - 1) - pos;
                            else inside = false;
                        }
                        idx = static_cast<unsigned>(pos);
                    }
                    // the clip's sample k (EQI / VARI: int16 times the power-of-two scale, exact)
                    auto clip_sample = [&](unsigned k) -> float {
                        if constexpr (EQI) return pcm_sample(xi, k, bpi->scale);
                        else if constexpr (VARI) return pcm_sample(xi, k, vpi->scale);
                        else return xc[k];
                    };
                    if (inside) {
                        val = clip_sample(idx);
                        if (a.preemph != 0.0f) {  // processing.rs:31-53 fused
                            const unsigned sh = a.preemph_shift % n_samples;
                            const unsigned jdx = idx >= sh ? idx - sh : idx + n_samples - sh;
                            val -= a.preemph * clip_sample(jdx);
                        }
                    }
                    if (a.window) val *= a.window[i];
                }
                return val;
            };
            float2 v[16];
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const unsigned n = static_cast<unsigned>(j + e * G::TPF);
                if (BLU) {  // chirp-z: one real sample per complex point, times the chirp
                    const float xv = sample(n);
                    const float2 c = n < a.blu_n ? a.blu_c[n] : make_float2(0.f, 0.f);
                    v[e] = make_float2(xv * c.x, xv * c.y);
                } else {
                    v[e] = make_float2(sample(2 * n), sample(2 * n + 1));
                }
            }
            frame_fft<LOG2C>(zbuf, j, a.tw_c, v);
            float part;
            if (BLU) {
                blu_convolve<LOG2C>(zbuf, j, a, v);
                part = blu_row<LOG2C>(zbuf, prow, nullptr, j, a, false, active, F);
            } else {
                part = untangle_row<LOG2C>(zbuf, prow, nullptr, j, a, false, active);
            }
            red[j] = part;
            frame_sync<LOG2C>();  // zbuf / prow / frow / red are private to the frame's slot

            if (a.out_kind == OUT_POWER) {
                if (active) {
                    float *dst = a.out0 + gf * F;
                    for (int k = j; k < F; k += G::TPF) dst[k] = prow[k];
                }
            } else {
                // feature.rs:216-219: frame energy + zero handling (deterministic serial sum)
                float energy = 0.0f;
                if (j == 0) {  // only the thread that owns coefficient 0 / the energy output needs it
                    for (int i = 0; i < G::TPF; ++i) energy += red[i];
                    energy = energy == 0.0f ? kEps : energy;
                }
                // feature.rs:229-230 banded; zero handling
                for (int m = j; m < M; m += G::TPF) {
                    float s = mel_dot(prow, a, m);
                    s = s == 0.0f ? kEps : s;
                    if (a.out_kind == OUT_MFE) {
                        if (active) a.out0[gf * M + m] = s;
                    } else {
                        frow[m] = fast_ln(s);  // feature.rs:105
                    }
                }
                if (a.out_kind == OUT_MFE) {
                    if (active && j == 0) a.out1[gf] = energy;
                } else {
                    frame_sync<LOG2C>();  // zbuf / prow / frow / red are private to the frame's slot
                    // feature.rs:120-146: DCT-II (first n_ceps outputs), scaling, column-0 replacement
                    const int Cc = static_cast<int>(a.n_ceps);
                    const int parts = G::TPF / Cc;  // threads per coefficient (uniform)
                    if (parts >= 2) {
                        // wide frames (many threads, long filter rows): split every coefficient's sum over `parts`
                        // threads, then combine the partials in fixed order (deterministic)
                        const int c = j % Cc, part = j / Cc;
                        const int ms = (M + parts - 1) / parts;
                        float s = 0.0f;
                        if (part < parts) {
                            const float *row = a.dct + c * M;
                            const int m1 = min(M, (part + 1) * ms);
                            for (int m = part * ms; m < m1; ++m) s = fmaf(frow[m], row[m], s);
                            red[j] = s;
                        }
                        frame_sync<LOG2C>();  // zbuf / prow / frow / red are private to the frame's slot
                        if (j < Cc) {
                            float tot = 0.0f;
                            for (int p = 0; p < parts; ++p) tot += red[p * Cc + j];
                            float o;
                            if (j == 0) o = a.dc_elimination ? fast_ln(energy) : tot * (t == 0 ? dct_scale_00 : a.dct_scale_0);
                            else o = tot * dct_scale_k;
                            if (active) a.out0[gf * Cc + j] = o;
                        }
                    } else {
                        for (int c = j; c < Cc; c += G::TPF) {
                            const float *row = a.dct + c * M;
                            float s = 0.0f;
                            for (int m = 0; m < M; ++m) s = fmaf(frow[m], row[m], s);
                            float o;
                            if (c == 0) o = a.dc_elimination ? fast_ln(energy) : s * (t == 0 ? dct_scale_00 : a.dct_scale_0);
                            else o = s * dct_scale_k;
                            if (active) a.out0[gf * Cc + c] = o;
                        }
                    }
                }
            }
            frame_sync<LOG2C>();  // zbuf / prow / frow / red are private to the frame's slot
        }
    } else if constexpr (VARR || SPR) {
        // ---------------- STFT / mel-spectrogram path over packed clips: tiles of TILE packed rows -------
        // (the rows of one tile may belong to several clips: a long clip among short ones is spread over the grid like the rest)
        // SPR: the "clips" are the entries of a ragged streaming call -- whole hops, no padding rows, and a window sample before the
        // chunk comes from the entry's pool row
        if constexpr (SPR) stream_check_entries(sp->e, blockIdx.x * kBlock + tid, gridDim.x * kBlock);
        else varrows_check_clips(*ra, blockIdx.x * kBlock + tid, gridDim.x * kBlock);
        const int W = BLU ? static_cast<int>(a.blu_n) : G::N;
        constexpr int TILE = 32;  // rows buffered before a transposed flush
        // per tile row, behind the mel tile: the output word of its (m = 0, r) element (-1: the row is not written) and its clip's R_b
        size_t rtab = slot_bytes * G::FPB + (a.out_kind == OUT_MEL ? sizeof(float) * M * (TILE + 1) : 0);
        rtab = (rtab + 7) & ~static_cast<size_t>(7);
        long long *t_base = reinterpret_cast<long long *>(smem_raw + rtab);
        unsigned *t_rows = reinterpret_cast<unsigned *>(t_base + TILE);
        unsigned long long total;
        if constexpr (SPR) total = sp->e.total_rows;
        else total = ra->total_rows;
        const unsigned long long tiles = (total + TILE - 1) / TILE;
        for (unsigned long long tg = blockIdx.x; tg < tiles; tg += gridDim.x) {
            const unsigned long long g0 = tg * TILE;
            const int rt = static_cast<int>(min(static_cast<unsigned long long>(TILE), total - g0));
            for (int rp = 0; rp < rt; rp += G::FPB) {
                const int rl = rp + slot;  // row within the tile
                const unsigned long long g = g0 + rl;
                // rows past the last clip (a larger output block) are left alone; rows of an inconsistent clip are skipped
                VarRowClip c;
                [[maybe_unused]] unsigned cb = 0;  // VARR: the row's clip
                [[maybe_unused]] const float *srow = nullptr;  // SPR: the entry's pool row, indexed from its end (sample p < 0 is srow[p])
                if constexpr (SPR) {
                    const StreamEntry en = stream_entry(sp->e, rl < rt ? offset_find(sp->e.ro, sp->e.n_active, static_cast<unsigned>(g)) : 0u);
                    c = VarRowClip{en.s0, en.r0, en.n, en.R, en.ok};
                    if (en.ok) srow = sp->e.pool + static_cast<unsigned long long>(en.slot) * sp->e.state_len + sp->e.state_len;
                } else {
                    cb = rl < rt ? offset_find(ra->ro, ra->n_clips, static_cast<long long>(g)) : 0u;
                    c = varrows_clip(*ra, cb);
                }
                const long long r = static_cast<long long>(g) - c.r0;  // row within the clip
                const bool valid = rl < rt && c.ok && r >= 0 && r < static_cast<long long>(c.R);
                const long long Rreal = c.R > a.n_pad ? static_cast<long long>(c.R - a.n_pad) : 0ll;
                const bool active = valid && r < Rreal;
                const float *xc = PCMX ? nullptr : a.x + (valid ? c.s0 : 0ll);
                [[maybe_unused]] const int16_t *xi = nullptr;  // a trailing BatchPcmArgs: the clip / chunk as PCM
                if constexpr (PCMX) xi = bpi->x + (valid ? c.s0 : 0ll);
                const long long ns = valid ? static_cast<long long>(c.n) : 0ll;
                // functions.rs:137-151: window over the last W samples ending at chunk r + n_pad of the clip
                const long long start = (r + a.n_pad + 1) * static_cast<long long>(a.hop) - W;
                auto wsample = [&](int i) -> float {
                    const long long idx = start + i;
                    if constexpr (SPR) {  // (idx >= -S: a row's window ends at least one hop into the chunk)
                        if (!active || i >= W || idx >= ns) return 0.0f;
                        // (PCM: int16 times the power-of-two scale, exact -- the float the float build reads; the pool row is float)
                        if constexpr (PCMX) return (idx < 0 ? srow[idx] : pcm_sample(xi, idx, bpi->scale)) * a.window[i];
                        else return (idx < 0 ? srow[idx] : xc[idx]) * a.window[i];
                    }
                    if constexpr (PCMX) return active && i < W && idx >= 0 && idx < ns ? pcm_sample(xi, idx, bpi->scale) * a.window[i] : 0.0f;
                    else return active && i < W && idx >= 0 && idx < ns ? xc[idx] * a.window[i] : 0.0f;
                };
                float2 v[16];
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const int n = j + e * G::TPF;
                    if (BLU) {
                        const float xv = wsample(n);
                        const float2 cc = n < W ? a.blu_c[n] : make_float2(0.f, 0.f);
                        v[e] = make_float2(xv * cc.x, xv * cc.y);
                    } else {
                        v[e] = make_float2(wsample(2 * n), wsample(2 * n + 1));
                    }
                }
                frame_fft<LOG2C>(zbuf, j, a.tw_c, v);
                float2 *stft_row = nullptr;
                if (a.out_kind == OUT_STFT && valid) stft_row = reinterpret_cast<float2 *>(a.out0) + g * F;
                if (BLU) {
                    blu_convolve<LOG2C>(zbuf, j, a, v);
                    blu_row<LOG2C>(zbuf, prow, stft_row, j, a, true, active, F);
                } else {
                    untangle_row<LOG2C>(zbuf, prow, stft_row, j, a, true, active);
                }
                frame_sync<LOG2C>();  // prow is private to the frame; the shared tile has its own barriers below
                if (a.out_kind == OUT_MEL && rl < rt) {
                    // feature.rs:173: out[m, r] = sum_f P[r, f] fb[m, f]; rows >= real_rows stay zero
                    [[maybe_unused]] float mx = -INFINITY;
                    for (int m = j; m < M; m += G::TPF) {
                        float val = active ? mel_dot(prow, a, m) : 0.0f;
                        if constexpr (DB) {
                            val = power_db(val, db->amin, db->ref_db);
                            mx = fmaxf(mx, val);
                        }
                        tile[m * (TILE + 1) + rl] = val;
                    }
                    if constexpr (DB) red[j] = mx;
                    if (j == 0) {
                        t_base[rl] = valid ? c.r0 * M + r : -1ll;
                        t_rows[rl] = c.R;
                    }
                }
                if (a.out_kind == OUT_STFT && valid && !active) {
                    for (int k = j; k < F; k += G::TPF) stft_row[k] = make_float2(0.0f, 0.0f);
                }
                __syncthreads();
                if constexpr (DB) {
                    // the row's maximum into its clip's word: rows that are written only (a skipped clip's word stays as it was)
                    if (db->max_key && a.out_kind == OUT_MEL && valid && j == 0) {
                        float mx = red[0];
                        for (int i = 1; i < G::TPF; ++i) mx = fmaxf(mx, red[i]);
                        if (mx > -INFINITY) atomicMax(db->max_key + cb, float_key(mx));
                    }
                }
            }
            if (a.out_kind == OUT_MEL) {
                // clip b's block [M x R_b] starts at out + M ro[b]: element (m, r) is word M ro[b] + m R_b + r
                for (int i = tid; i < M * rt; i += kBlock) {
                    const int m = i / rt, rl = i - m * rt;
                    const long long b0 = t_base[rl];
                    if (b0 >= 0) a.out0[b0 + static_cast<long long>(m) * t_rows[rl]] = tile[m * (TILE + 1) + rl];
                }
                __syncthreads();
            }
        }
    } else if constexpr (!VAR) {
        // ---------------- STFT / mel-spectrogram path: one clip (channel) per workgroup visit -------
        const int R = static_cast<int>(a.rows);
        const int Rreal = static_cast<int>(a.real_rows);
        const int W = BLU ? static_cast<int>(a.blu_n) : G::N;
        constexpr int TILE = 32;  // rows buffered before a transposed, coalesced flush
        for (unsigned clip = blockIdx.x; clip < a.batch; clip += gridDim.x) {
            const float *xc = EQI ? nullptr : a.x + static_cast<unsigned long long>(clip) * a.ld;
            [[maybe_unused]] const int16_t *xi = nullptr;  // EQI: the clip as PCM
            if constexpr (EQI) xi = bpi->x + static_cast<unsigned long long>(clip) * a.ld;
            // STREAM: the stream's state, indexed from its end (sample p < 0 of the stream is srow[p], p >= -S)
            [[maybe_unused]] const float *srow = nullptr;
            if constexpr (STREAM) srow = sa->state + static_cast<unsigned long long>(clip) * sa->state_len + sa->state_len;
            for (int r0 = 0; r0 < R; r0 += TILE) {
                const int rt = min(TILE, R - r0);
                for (int rp = 0; rp < rt; rp += G::FPB) {
                    const int rl = rp + slot;       // row within the tile
                    const int r = r0 + rl;          // output row
                    const bool active = rl < rt && r < Rreal;
                    // functions.rs:137-151: window over the last W samples ending at chunk r + n_pad
                    const long long start = static_cast<long long>(r + a.n_pad + 1) * a.hop - W;
                    auto wsample = [&](int i) -> float {
                        const long long idx = start + i;
                        if constexpr (STREAM) {
                            if (!active || i >= W || idx >= static_cast<long long>(a.n_samples)) return 0.0f;
                            return (idx < 0 ? srow[idx] : xc[idx]) * a.window[i];
                        }
                        // (EQI: int16 times the power-of-two scale, exact -- the float the float build reads)
                        if constexpr (EQI)
                            return active && i < W && idx >= 0 && idx < static_cast<long long>(a.n_samples) ? pcm_sample(xi, idx, bpi->scale) * a.window[i] : 0.0f;
                        else return active && i < W && idx >= 0 && idx < static_cast<long long>(a.n_samples) ? xc[idx] * a.window[i] : 0.0f;
                    };
                    float2 v[16];
#pragma unroll
                    for (int e = 0; e < 16; ++e) {
                        const int n = j + e * G::TPF;
                        if (BLU) {
                            const float xv = wsample(n);
                            const float2 c = n < W ? a.blu_c[n] : make_float2(0.f, 0.f);
                            v[e] = make_float2(xv * c.x, xv * c.y);
                        } else {
                            v[e] = make_float2(wsample(2 * n), wsample(2 * n + 1));
                        }
                    }
                    frame_fft<LOG2C>(zbuf, j, a.tw_c, v);
                    float2 *stft_row = nullptr;
                    if (a.out_kind == OUT_STFT)
                        stft_row = reinterpret_cast<float2 *>(a.out0) + (static_cast<unsigned long long>(clip) * R + r) * F;
                    if (BLU) {
                        blu_convolve<LOG2C>(zbuf, j, a, v);
                        blu_row<LOG2C>(zbuf, prow, stft_row, j, a, true, active, F);
                    } else {
                        untangle_row<LOG2C>(zbuf, prow, stft_row, j, a, true, active);
                    }
                    frame_sync<LOG2C>();  // prow is private to the frame; the shared tile has its own barriers below
                    if (a.out_kind == OUT_MEL && rl < rt) {
                        // feature.rs:173: out[n,m,t] = sum_f P[n,t,f] fb[m,f]; rows >= real_rows stay zero
                        [[maybe_unused]] float mx = -INFINITY;
                        for (int m = j; m < M; m += G::TPF) {
                            float val = active ? mel_dot(prow, a, m) : 0.0f;
                            if constexpr (DB) {
                                val = power_db(val, db->amin, db->ref_db);
                                mx = fmaxf(mx, val);
                            }
                            tile[m * (TILE + 1) + rl] = val;
                        }
                        if constexpr (DB) red[j] = mx;
                    }
                    if (a.out_kind == OUT_STFT && rl < rt && r >= Rreal) {
                        for (int k = j; k < F; k += G::TPF) stft_row[k] = make_float2(0.0f, 0.0f);
                    }
                    __syncthreads();
                    if constexpr (DB) {
                        if (db->max_key && a.out_kind == OUT_MEL && rl < rt && j == 0) {
                            float mx = red[0];
                            for (int i = 1; i < G::TPF; ++i) mx = fmaxf(mx, red[i]);
                            if (mx > -INFINITY) atomicMax(db->max_key + clip, float_key(mx));
                        }
                    }
                }
                if (a.out_kind == OUT_MEL) {
                    float *dst = a.out0 + static_cast<unsigned long long>(clip) * M * R;
                    for (int i = tid; i < M * rt; i += kBlock) {
                        const int m = i / rt, rl = i - m * rt;
                        dst[static_cast<unsigned long long>(m) * R + r0 + rl] = tile[m * (TILE + 1) + rl];
                    }
                    __syncthreads();
                }
            }
        }
    }
}

template <int LOG2C>
size_t front_lds_bytes(const FrontArgs &a)
{
    using G = Geo<LOG2C>;
    const size_t mpad = (a.n_filters + 3) & ~3u;
    const size_t slot_bytes = sizeof(float2) * G::ZLEN + sizeof(float) * (G::PLEN + mpad + G::TPF + 4);
    size_t total = slot_bytes * G::FPB;
    if (a.out_kind == OUT_MEL) total += sizeof(float) * a.n_filters * 33;
    return (total + 15) & ~static_cast<size_t>(15);
}

// The parts of a launch that depend on the layout, chosen by the type of the kernel's trailing argument (none: the equal-length
// builds): the suffix of the reported name, the LDS behind the equal-length carve, and the workgroup visits of the call.
constexpr const char *layout_suffix() { return ""; }
constexpr const char *layout_suffix(const VarlenArgs &) { return "_varlen"; }
constexpr const char *layout_suffix(const BatchPcmArgs &) { return "_i16"; }
constexpr const char *layout_suffix(const VarlenPcmArgs &) { return "_varleni"; }
constexpr const char *layout_suffix(const VarRowsArgs &) { return "_varrows"; }
constexpr const char *layout_suffix(const StreamArgs &) { return "_stream"; }
constexpr const char *layout_suffix(const FrameStreamArgs &) { return "_fstream"; }
constexpr const char *layout_suffix(const FrameStreamPackedArgs &) { return "_fstreamp"; }
constexpr const char *layout_suffix(const FrameStreamPackedPcmArgs &) { return "_fstreampi"; }
constexpr const char *layout_suffix(const StftStreamPackedArgs &) { return "_streamp"; }
constexpr const char *layout_suffix(const VarRowsArgs &, const BatchPcmArgs &) { return "_varrowsi"; }
constexpr const char *layout_suffix(const StftStreamPackedArgs &, const BatchPcmArgs &) { return "_streampi"; }
// (a DbArgs last: the layout's own suffix -- the dB builds carry `db` in the template list, front_kernel_name)
constexpr const char *layout_suffix(const DbArgs &) { return ""; }
constexpr const char *layout_suffix(const BatchPcmArgs &p, const DbArgs &) { return layout_suffix(p); }
constexpr const char *layout_suffix(const VarRowsArgs &v, const DbArgs &) { return layout_suffix(v); }
constexpr const char *layout_suffix(const VarRowsArgs &v, const BatchPcmArgs &p, const DbArgs &) { return layout_suffix(v, p); }

// the packed-rows builds: the tile's row table (32 offsets + 32 row counts, 8-byte aligned)
constexpr size_t kRowTableBytes = 32 * (sizeof(long long) + sizeof(unsigned)) + 16;
template <typename... V>
constexpr size_t layout_lds(const V &...) { return 0; }
constexpr size_t layout_lds(const VarRowsArgs &) { return kRowTableBytes; }
constexpr size_t layout_lds(const StftStreamPackedArgs &) { return kRowTableBytes; }
constexpr size_t layout_lds(const FrameStreamPackedPcmArgs &) { return 0; }
constexpr size_t layout_lds(const BatchPcmArgs &) { return 0; }
constexpr size_t layout_lds(const VarlenPcmArgs &) { return 0; }
constexpr size_t layout_lds(const VarRowsArgs &, const BatchPcmArgs &) { return kRowTableBytes; }
constexpr size_t layout_lds(const StftStreamPackedArgs &, const BatchPcmArgs &) { return kRowTableBytes; }
constexpr size_t layout_lds(const DbArgs &) { return 0; }
constexpr size_t layout_lds(const BatchPcmArgs &, const DbArgs &) { return 0; }
constexpr size_t layout_lds(const VarRowsArgs &, const DbArgs &) { return kRowTableBytes; }
constexpr size_t layout_lds(const VarRowsArgs &, const BatchPcmArgs &, const DbArgs &) { return kRowTableBytes; }

// Workgroup visits of a call at `fpb` frames per visit.  0: nothing to launch; kTooManyRows: the kernel's 32-bit row index does not
// reach the last row.
constexpr unsigned long long kTooManyRows = ~0ull;
inline unsigned long long layout_work(const FrontArgs &a, unsigned long long fpb)
{
    const unsigned long long frames = static_cast<unsigned long long>(a.batch) * a.n_frames;
    const unsigned long long work = (a.out_kind == OUT_MEL || a.out_kind == OUT_STFT) ? a.batch : (frames + fpb - 1) / fpb;
    return work != 0 && frames >= 0xffffffffull ? kTooManyRows : work;
}
inline unsigned long long layout_work(const FrontArgs &a, unsigned long long, const StreamArgs &) { return a.batch; }
inline unsigned long long layout_work(const FrontArgs &a, unsigned long long fpb, const FrameStreamArgs &)
{
    const unsigned long long rows = static_cast<unsigned long long>(a.batch) * a.n_frames;
    return rows >= 0xffffffffull ? kTooManyRows : (rows + fpb - 1) / fpb;
}
// The table-driven layouts launch at least one workgroup: the pass over the clips / entries runs even where the output block has
// no rows.
constexpr unsigned long long at_least_one(unsigned long long units) { return units ? units : 1; }
inline unsigned long long layout_work(const FrontArgs &, unsigned long long fpb, const VarlenArgs &v)
{
    return at_least_one((v.total_frames + fpb - 1) / fpb);
}
inline unsigned long long layout_work(const FrontArgs &, unsigned long long fpb, const FrameStreamPackedArgs &s)
{
    return at_least_one((s.total_rows + fpb - 1) / fpb);
}
inline unsigned long long layout_work(const FrontArgs &a, unsigned long long fpb, const FrameStreamPackedPcmArgs &s)
{
    return layout_work(a, fpb, s.e);
}
inline unsigned long long layout_work(const FrontArgs &a, unsigned long long fpb, const BatchPcmArgs &) { return layout_work(a, fpb); }
inline unsigned long long layout_work(const FrontArgs &a, unsigned long long fpb, const VarlenPcmArgs &v) { return layout_work(a, fpb, v.v); }
inline unsigned long long layout_work(const FrontArgs &, unsigned long long, const VarRowsArgs &v) { return at_least_one((v.total_rows + 31) / 32); }
inline unsigned long long layout_work(const FrontArgs &, unsigned long long, const StftStreamPackedArgs &s)
{
    return at_least_one((static_cast<unsigned long long>(s.e.total_rows) + 31) / 32);
}
inline unsigned long long layout_work(const FrontArgs &a, unsigned long long fpb, const VarRowsArgs &v, const BatchPcmArgs &) { return layout_work(a, fpb, v); }
inline unsigned long long layout_work(const FrontArgs &a, unsigned long long fpb, const StftStreamPackedArgs &s, const BatchPcmArgs &)
{
    return layout_work(a, fpb, s);
}
inline unsigned long long layout_work(const FrontArgs &a, unsigned long long fpb, const DbArgs &) { return layout_work(a, fpb); }
inline unsigned long long layout_work(const FrontArgs &a, unsigned long long fpb, const BatchPcmArgs &, const DbArgs &) { return layout_work(a, fpb); }
inline unsigned long long layout_work(const FrontArgs &a, unsigned long long fpb, const VarRowsArgs &v, const DbArgs &) { return layout_work(a, fpb, v); }
inline unsigned long long layout_work(const FrontArgs &a, unsigned long long fpb, const VarRowsArgs &v, const BatchPcmArgs &, const DbArgs &)
{
    return layout_work(a, fpb, v);
}

// What ss_last_kernel_name() reports for an instantiation: ss_front_generic<suffix><LOG2C[,chirpz][,db]>, built once, kept for the process.
template <int LOG2C, bool BLU, typename... V>
const char *front_kernel_name(const V &...v)
{
    struct Name {
        char s[48];
    };
    static const Name name = [&] {
        Name n;
        snprintf(n.s, sizeof n.s, "ss_front_generic%s<%d%s%s>", layout_suffix(v...), LOG2C, BLU ? ",chirpz" : "",
                 (std::is_same_v<V, DbArgs> || ...) ? ",db" : "");
        return n;
    }();
    return name.s;
}

template <int LOG2C, bool BLU, typename... V>
hipError_t launch_one(const FrontArgs &a, hipStream_t stream, int num_cus, LaunchInfo *info, const V &...v)
{
    const size_t lds = front_lds_bytes<LOG2C>(a) + layout_lds(v...);
    if (lds > 160 * 1024) return hipErrorInvalidValue;
    if (lds > 48 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&ss_front_generic<LOG2C, BLU, V...>),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds));
        if (e != hipSuccess) return e;
    }
    const unsigned long long work = layout_work(a, Geo<LOG2C>::FPB, v...);
    if (work == 0) return hipSuccess;
    if (work == kTooManyRows) return hipErrorInvalidValue;
    const unsigned long long cap = cu_cap(num_cus) * 8ull;
    const unsigned grid = static_cast<unsigned>(work < cap ? work : cap);
    if (info) *info = LaunchInfo{front_kernel_name<LOG2C, BLU>(v...), grid, static_cast<unsigned>(kBlock), lds, (std::is_same_v<V, DbArgs> || ...)};
    hipLaunchKernelGGL((ss_front_generic<LOG2C, BLU, V...>), dim3(grid), dim3(kBlock), lds, stream, a, v...);
    return hipGetLastError();
}

// every build of the generic kernel for one layout: log2c 4 .. 12, chirp-z (a.blu_n != 0) or not
template <typename... V>
hipError_t dispatch_front(const FrontArgs &a, uint32_t log2c, hipStream_t stream, int num_cus, LaunchInfo *info, const V &...v)
{
    if (a.blu_n) {
        switch (log2c) {
            case 4: return launch_one<4, true>(a, stream, num_cus, info, v...);
            case 5: return launch_one<5, true>(a, stream, num_cus, info, v...);
            case 6: return launch_one<6, true>(a, stream, num_cus, info, v...);
            case 7: return launch_one<7, true>(a, stream, num_cus, info, v...);
            case 8: return launch_one<8, true>(a, stream, num_cus, info, v...);
            case 9: return launch_one<9, true>(a, stream, num_cus, info, v...);
            case 10: return launch_one<10, true>(a, stream, num_cus, info, v...);
            case 11: return launch_one<11, true>(a, stream, num_cus, info, v...);
            case 12: return launch_one<12, true>(a, stream, num_cus, info, v...);
            default: return hipErrorInvalidValue;
        }
    }
    switch (log2c) {
        case 4: return launch_one<4, false>(a, stream, num_cus, info, v...);
        case 5: return launch_one<5, false>(a, stream, num_cus, info, v...);
        case 6: return launch_one<6, false>(a, stream, num_cus, info, v...);
        case 7: return launch_one<7, false>(a, stream, num_cus, info, v...);
        case 8: return launch_one<8, false>(a, stream, num_cus, info, v...);
        case 9: return launch_one<9, false>(a, stream, num_cus, info, v...);
        case 10: return launch_one<10, false>(a, stream, num_cus, info, v...);
        case 11: return launch_one<11, false>(a, stream, num_cus, info, v...);
        case 12: return launch_one<12, false>(a, stream, num_cus, info, v...);
        default: return hipErrorInvalidValue;
    }
}

// State advance (functions.rs:152-160 over a call's chunks): row s := the last S samples of old row ++ x_s[0 .. advance), zeros
// past n_samples.  A workgroup per stream (grid-stride over the streams) walks its row upwards in blocks of 256: block i0 reads
// state[i0 + advance ..] (above every index written so far: advance >= 1) and the chunk, waits at the barrier until every lane has
// read, then writes state[i0 ..].  Plain vector loads and stores.
__global__ __launch_bounds__(256) void ss_stream_advance(float *__restrict__ state, unsigned S, const float *__restrict__ x,
                                                          unsigned long long ld, unsigned n_samples, unsigned advance, unsigned batch)
{
    for (unsigned s = blockIdx.x; s < batch; s += gridDim.x) {
        float *st = state + static_cast<unsigned long long>(s) * S;
        const float *xc = x + static_cast<unsigned long long>(s) * ld;
        for (unsigned i0 = 0; i0 < S; i0 += 256) {
            const unsigned i = i0 + threadIdx.x;
            float v = 0.0f;
            if (i < S) {
                const unsigned long long k = static_cast<unsigned long long>(i) + advance;  // index into old row ++ chunk
                if (k < S) v = st[k];
                else if (k - S < n_samples) v = xc[k - S];
            }
            __syncthreads();
            if (i < S) st[i] = v;
        }
    }
}

// The same over a pool of states (launch_stream_advance_packed): a workgroup per entry (grid-stride over the entries); an entry that
// stream_entry() finds inconsistent, or that has no samples, leaves its pool row alone.  (The entry is uniform over the workgroup:
// every lane reaches the barriers.)
__global__ __launch_bounds__(256) void ss_stream_advance_packed(const FrameStreamPackedArgs v, const float *__restrict__ x)
{
    const unsigned S = v.state_len;
    for (unsigned e = blockIdx.x; e < v.n_active; e += gridDim.x) {
        const StreamEntry en = stream_entry(v, e);
        if (!en.ok || en.n == 0u) continue;
        float *st = v.pool + static_cast<unsigned long long>(en.slot) * S;
        const float *xc = x + en.s0;
        for (unsigned i0 = 0; i0 < S; i0 += 256) {
            const unsigned i = i0 + threadIdx.x;
            float val = 0.0f;
            if (i < S) {
                const unsigned long long k = static_cast<unsigned long long>(i) + en.n;  // index into old row ++ chunk
                val = k < S ? st[k] : xc[k - S];  // (k - S < n: i < S)
            }
            __syncthreads();
            if (i < S) st[i] = val;
        }
    }
}

// ss_stream_advance_packed behind a PCM call (launch_stream_advance_packed, FrameStreamPackedPcmArgs): the chunk's samples are
// (float)int16 * scale, so a pool row ends up holding exactly the floats the float call would have stored.  Same blocks, same
// read-all-then-write discipline; plain vector loads and stores.
__global__ __launch_bounds__(256) void ss_stream_advance_packed_i16(const FrameStreamPackedPcmArgs vp)
{
    const FrameStreamPackedArgs &v = vp.e;
    const unsigned S = v.state_len;
    for (unsigned e = blockIdx.x; e < v.n_active; e += gridDim.x) {
        const StreamEntry en = stream_entry(v, e);
        if (!en.ok || en.n == 0u) continue;
        float *st = v.pool + static_cast<unsigned long long>(en.slot) * S;
        const int16_t *xc = vp.x + en.s0;
        for (unsigned i0 = 0; i0 < S; i0 += 256) {
            const unsigned i = i0 + threadIdx.x;
            float val = 0.0f;
            if (i < S) {
                const unsigned long long k = static_cast<unsigned long long>(i) + en.n;  // index into old row ++ chunk
                val = k < S ? st[k] : pcm_sample(xc, static_cast<long long>(k - S), vp.scale);  // (k - S < n: i < S)
            }
            __syncthreads();
            if (i < S) st[i] = val;
        }
    }
}

__global__ void ss_preemphasis_kernel(const float *__restrict__ x, float *__restrict__ y, size_t n, size_t shift, float cof)
{
    // processing.rs:31-53: y[i] = x[i] - cof * x[(i - shift) mod n]
    for (size_t i = blockIdx.x * static_cast<size_t>(blockDim.x) + threadIdx.x; i < n;
         i += static_cast<size_t>(gridDim.x) * blockDim.x) {
        const size_t jx = i >= shift ? i - shift : i + n - shift;
        y[i] = x[i] - cof * x[jx];
    }
}

#if SS_LAB
// (lab library only: ss_debug_poison_lds)
// One workgroup takes a CU's whole LDS (160 KB), so a grid of several workgroups per CU sweeps every CU several times.
__global__ __launch_bounds__(256) void ss_poison_lds_kernel(unsigned words)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    unsigned *w = reinterpret_cast<unsigned *>(smem_raw);
    for (unsigned i = threadIdx.x; i < words; i += 256) w[i] = 0xFFFFFFFFu;
    __syncthreads();
    // keep the stores observable
    if (w[(threadIdx.x * 97u) % words] != 0xFFFFFFFFu) __builtin_trap();
}
#endif

}  // namespace

#if SS_LAB
hipError_t launch_poison_lds(hipStream_t stream, int num_cus)
{
    const size_t lds = 160 * 1024;
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&ss_poison_lds_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds));
    if (e != hipSuccess) return e;
    const unsigned grid = cu_cap(num_cus) * 4;
    hipLaunchKernelGGL(ss_poison_lds_kernel, dim3(grid), dim3(256), lds, stream, static_cast<unsigned>(lds / 4));
    return hipGetLastError();
}
#endif

// (db, here and on the PCM and the two packed-rows launchers below: the dB build of the same layout, mel output only)
hipError_t launch_front_generic(const FrontArgs &a, uint32_t log2c, hipStream_t stream, int num_cus, LaunchInfo *info, const DbArgs *db)
{
    if (db) return a.out_kind == OUT_MEL ? dispatch_front(a, log2c, stream, num_cus, info, *db) : hipErrorInvalidValue;
    return dispatch_front(a, log2c, stream, num_cus, info);
}

hipError_t launch_front_generic_varlen(const FrontArgs &a, const VarlenArgs &v, uint32_t log2c, hipStream_t stream, int num_cus,
                                       LaunchInfo *info)
{
    if (a.out_kind != OUT_MFCC && a.out_kind != OUT_MFE) return hipErrorInvalidValue;
    return dispatch_front(a, log2c, stream, num_cus, info, v);
}

hipError_t launch_front_generic(const FrontArgs &a, const BatchPcmArgs &p, uint32_t log2c, hipStream_t stream, int num_cus, LaunchInfo *info,
                                const DbArgs *db)
{
    if (!p.x) return hipErrorInvalidValue;  // (every output: MFCC / mfe / power, and the mel / stft rows of the STFT path)
    if (db) return a.out_kind == OUT_MEL ? dispatch_front(a, log2c, stream, num_cus, info, p, *db) : hipErrorInvalidValue;
    return dispatch_front(a, log2c, stream, num_cus, info, p);
}

hipError_t launch_front_generic_varlen(const FrontArgs &a, const VarlenPcmArgs &v, uint32_t log2c, hipStream_t stream, int num_cus,
                                       LaunchInfo *info)
{
    if ((a.out_kind != OUT_MFCC && a.out_kind != OUT_MFE) || !v.x) return hipErrorInvalidValue;
    return dispatch_front(a, log2c, stream, num_cus, info, v);
}

// The PCM calls' fallback (launch_pcm_to_float): dst[r * ld + k] = (float)src[r * ld + k] * scale, k < n.  Grid-stride over the
// rows' samples; plain vector loads and stores.
__global__ __launch_bounds__(256) void ss_pcm_to_float(const int16_t *__restrict__ src, float *__restrict__ dst, unsigned long long rows,
                                                        unsigned long long n, unsigned long long ld, float scale)
{
    const unsigned long long total = rows * n, stride = static_cast<unsigned long long>(gridDim.x) * 256u;
    for (unsigned long long i = static_cast<unsigned long long>(blockIdx.x) * 256u + threadIdx.x; i < total; i += stride) {
        const unsigned long long r = ld == n ? 0ull : i / n;
        const unsigned long long k = i - r * n + r * ld;
        dst[k] = pcm_sample(src, static_cast<long long>(k), scale);
    }
}

hipError_t launch_pcm_to_float(const int16_t *src, float *dst, size_t rows, size_t n, size_t ld, float scale, hipStream_t stream)
{
    if (rows == 0 || n == 0) return hipSuccess;
    if (!src || !dst || ld < n) return hipErrorInvalidValue;
    const unsigned long long total = static_cast<unsigned long long>(rows) * n, blocks = (total + 255) / 256;
    hipLaunchKernelGGL(ss_pcm_to_float, dim3(static_cast<unsigned>(blocks < 8192 ? blocks : 8192)), dim3(256), 0, stream, src, dst,
                       static_cast<unsigned long long>(rows), static_cast<unsigned long long>(n), static_cast<unsigned long long>(ld), scale);
    return hipGetLastError();
}

hipError_t launch_front_generic_varrows(const FrontArgs &a, const VarRowsArgs &v, uint32_t log2c, hipStream_t stream, int num_cus,
                                        LaunchInfo *info, const DbArgs *db)
{
    if (a.out_kind != OUT_MEL && a.out_kind != OUT_STFT) return hipErrorInvalidValue;
    if (db) return a.out_kind == OUT_MEL ? dispatch_front(a, log2c, stream, num_cus, info, v, *db) : hipErrorInvalidValue;
    return dispatch_front(a, log2c, stream, num_cus, info, v);
}

hipError_t launch_front_generic_varrows(const FrontArgs &a, const VarRowsArgs &v, const BatchPcmArgs &p, uint32_t log2c, hipStream_t stream,
                                        int num_cus, LaunchInfo *info, const DbArgs *db)
{
    if ((a.out_kind != OUT_MEL && a.out_kind != OUT_STFT) || !p.x) return hipErrorInvalidValue;
    if (db) return a.out_kind == OUT_MEL ? dispatch_front(a, log2c, stream, num_cus, info, v, p, *db) : hipErrorInvalidValue;
    return dispatch_front(a, log2c, stream, num_cus, info, v, p);
}

hipError_t launch_front_generic_stream(const FrontArgs &a, const StreamArgs &s, uint32_t log2c, hipStream_t stream, int num_cus,
                                       LaunchInfo *info)
{
    if (a.out_kind != OUT_MEL && a.out_kind != OUT_STFT) return hipErrorInvalidValue;
    return dispatch_front(a, log2c, stream, num_cus, info, s);
}

hipError_t launch_front_generic_frame_stream(const FrontArgs &a, const FrameStreamArgs &s, uint32_t log2c, hipStream_t stream, int num_cus,
                                             LaunchInfo *info)
{
    if (a.out_kind != OUT_MFCC && a.out_kind != OUT_MFE) return hipErrorInvalidValue;
    return dispatch_front(a, log2c, stream, num_cus, info, s);
}

hipError_t launch_front_generic_frame_stream_packed(const FrontArgs &a, const FrameStreamPackedArgs &s, uint32_t log2c, hipStream_t stream,
                                                    int num_cus, LaunchInfo *info)
{
    if (a.out_kind != OUT_MFCC && a.out_kind != OUT_MFE) return hipErrorInvalidValue;
    if (s.n_active == 0 || s.step == 0 || (s.state_len > 0 && !s.pool) || s.total_rows >= 0x7fffffffu) return hipErrorInvalidValue;
    return dispatch_front(a, log2c, stream, num_cus, info, s);
}

hipError_t launch_front_generic_frame_stream_packed(const FrontArgs &a, const FrameStreamPackedPcmArgs &s, uint32_t log2c, hipStream_t stream,
                                                    int num_cus, LaunchInfo *info)
{
    if (a.out_kind != OUT_MFCC && a.out_kind != OUT_MFE) return hipErrorInvalidValue;
    if (!s.x || s.e.n_active == 0 || s.e.step == 0 || (s.e.state_len > 0 && !s.e.pool) || s.e.total_rows >= 0x7fffffffu)
        return hipErrorInvalidValue;
    return dispatch_front(a, log2c, stream, num_cus, info, s);
}

// the ragged streaming launch for either chunk format: p = empty (floats at a.x) or one BatchPcmArgs
template <typename... P>
static hipError_t launch_stream_packed_any(const FrontArgs &a, const StftStreamPackedArgs &s, uint32_t log2c, hipStream_t stream, int num_cus,
                                           LaunchInfo *info, const P &...p)
{
    if (a.out_kind != OUT_MEL && a.out_kind != OUT_STFT) return hipErrorInvalidValue;
    // the windows the kernel reads: W samples ending (t + 1) hops into the chunk, the first W - hop = S of them at most in the pool row
    const uint32_t W = a.blu_n ? a.blu_n : 2u << log2c;
    if (s.e.n_active == 0 || a.hop == 0 || s.e.step != a.hop || a.n_pad != 0 || s.e.state_len + a.hop != W || !s.e.pool ||
        s.e.total_rows >= 0x7fffffffu)
        return hipErrorInvalidValue;
    return dispatch_front(a, log2c, stream, num_cus, info, s, p...);
}

hipError_t launch_front_generic_stream_packed(const FrontArgs &a, const StftStreamPackedArgs &s, uint32_t log2c, hipStream_t stream,
                                              int num_cus, LaunchInfo *info)
{
    return launch_stream_packed_any(a, s, log2c, stream, num_cus, info);
}

hipError_t launch_front_generic_stream_packed(const FrontArgs &a, const StftStreamPackedArgs &s, const BatchPcmArgs &p, uint32_t log2c,
                                              hipStream_t stream, int num_cus, LaunchInfo *info)
{
    if (!p.x) return hipErrorInvalidValue;
    return launch_stream_packed_any(a, s, log2c, stream, num_cus, info, p);
}

hipError_t launch_stream_advance_packed(const FrameStreamPackedArgs &s, const float *x, hipStream_t stream)
{
    if (s.n_active == 0 || s.state_len == 0) return hipSuccess;
    if (!s.pool || s.step == 0) return hipErrorInvalidValue;
    const unsigned grid = s.n_active < 65536u ? s.n_active : 65536u;
    hipLaunchKernelGGL(ss_stream_advance_packed, dim3(grid), dim3(256), 0, stream, s, x);
    return hipGetLastError();
}

hipError_t launch_stream_advance_packed(const FrameStreamPackedPcmArgs &s, hipStream_t stream)
{
    if (s.e.n_active == 0 || s.e.state_len == 0) return hipSuccess;
    if (!s.e.pool || s.e.step == 0 || !s.x) return hipErrorInvalidValue;
    const unsigned grid = s.e.n_active < 65536u ? s.e.n_active : 65536u;
    hipLaunchKernelGGL(ss_stream_advance_packed_i16, dim3(grid), dim3(256), 0, stream, s);
    return hipGetLastError();
}

hipError_t launch_stream_advance(float *state, uint32_t state_len, const float *x, unsigned long long ld, uint32_t n_samples,
                                 uint32_t advance, uint32_t batch, hipStream_t stream)
{
    if (batch == 0 || state_len == 0) return hipSuccess;
    if (advance == 0) return hipErrorInvalidValue;
    const unsigned grid = batch < 65536u ? batch : 65536u;
    hipLaunchKernelGGL(ss_stream_advance, dim3(grid), dim3(256), 0, stream, state, state_len, x, ld, n_samples, advance, batch);
    return hipGetLastError();
}

hipError_t launch_preemphasis(const float *x, float *y, size_t n, size_t shift, float cof, hipStream_t stream)
{
    if (n == 0) return hipSuccess;
    const unsigned block = 256;
    size_t blocks = (n + block - 1) / block;
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(ss_preemphasis_kernel, dim3(static_cast<unsigned>(blocks)), dim3(block), 0, stream, x, y, n, shift, cof);
    return hipGetLastError();
}

}  // namespace ss
