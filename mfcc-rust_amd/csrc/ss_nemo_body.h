// ss_nemo_c256, the one copy of the kernel (ss_nemo512.hip: the dense and packed builds; ss_nemo512_pool.hip: the stream-pool and
// flush builds).  Everything behind the load -- the whole-clip pre-emphasis on the input registers, the window, both radix-16
// passes, the untangle, the P row, the banded mel, ln and the stores -- exists here once, so that a frame's bits do not depend on
// where its samples came from.  What a source kind (NSrc) adds is its row lookup and its loader:
//   * kNDense / kNVarlen: frame_of + load_quad_n (see ss_nemo512.hip's header).
//   * kNPool / kNPoolPcm (a FrameStreamPackedArgs / FrameStreamPackedPcmArgs in the kernel's trailing argument pack): the flat work
//     list is the packed output rows of a ragged streaming launch; a row's frame lies in the tail of its entry's pool row and the
//     head of its chunk (load_quad_npool below).  Nothing is masked: a row's frame ends inside its chunk.
//   * kNFlush (a NemoFlushArgs): the work list is the L rows of every named stream; a frame lies in the pool row and, from the
//     stream's end on, in the zeros the dense call's masked fill leaves there (load_quad_nflush below).
#pragma once

#include "ss_device.h"
#include "ss_fft_reg.h"
#include "ss_internal.h"
#include "ss_quad256.h"
#include "ss_wave.h"

namespace ss {

namespace {  // (each kernel file has its own copy: the files that include this share no symbol)

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

// The source kinds of the body
enum NSrc : int { kNDense = 0, kNVarlen = 1, kNPool = 2, kNPoolPcm = 3, kNFlush = 4 };

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

// ---- pool builds: the row of a ragged streaming launch (ss_nstream_log_mel_packed*_device) ----
// the entry block of either pool argument
__device__ __forceinline__ const FrameStreamPackedArgs &pool_block(const FrameStreamPackedArgs &s) { return s; }
__device__ __forceinline__ const FrameStreamPackedArgs &pool_block(const FrameStreamPackedPcmArgs &s) { return s.e; }

// Issues the loads of one quad of a pool launch: packed output row g = q4 + f belongs to the entry row_owner() finds over ro; row t
// of entry i is the frame whose first live sample is chunk position s0 = 160 t - lead, lead = 160 L + W / 2 = S - 1, position p < 0
// being pool[slot * S + S + p].  The frame ends inside the chunk (s0 + W <= 160 (t + 1): W / 2 <= 160 (L + 1)) and its
// pre-emphasis predecessor s0 - 1 >= -S lies inside the pool row, so nothing is masked: lim says "every position" and edge is false
// (the consumer clears nothing).  A lane whose entry stream_entry() finds bad, or whose row lies past the last entry, loads nothing
// and (lim = 0) stores nothing.
// The choice between the two paths is per quad and wave-uniform, and changes no bit (both fetch the same samples):
//   * interior: the quad's four frames start inside their chunks (s0 >= 0) -- no per-sample test: a float2 where the four starts are
//     8-byte aligned, else two floats; a PCM pair is ONE dword at either parity and stays raw in the pair's .x (raw = true); pcm_pair
//     converts it at the top of the iteration that consumes vin[] -- converting here would wait for the loads right behind pass 1.
//   * any other quad: single samples with a per-sample source select, PCM converted on the spot (raw = false).
template <int NE, typename SPT>
__device__ __forceinline__ void load_quad_npool(const NemoArgs &a, const SPT &sp, unsigned quad, unsigned total, int f, int j, unsigned &cursor,
                                                float2 (&vin)[NE], float &pred, int &lim, bool &edge, bool &raw)
{
    constexpr bool PCM = std::is_same_v<SPT, FrameStreamPackedPcmArgs>;
    const FrameStreamPackedArgs &s = pool_block(sp);
    const unsigned q4 = quad * 4;                                           // uniform
    const unsigned g = q4 + min(static_cast<unsigned>(f), total - 1 - q4);  // lanes past the last row redo it
    const unsigned c = row_owner(s.ro, s.n_active, q4, g, cursor);
    const StreamEntry en = stream_entry(s, c);
    const long long tl = static_cast<long long>(g) - en.r0;
    const bool ok = en.ok && tl >= 0 && tl < static_cast<long long>(en.R);
    const int W = static_cast<int>(a.win_len);
    const int s0 = ok ? static_cast<int>(tl) * kHop - s.lead : 0;  // (t * 160 < n_i < 2^31)
#pragma unroll
    for (int e = 0; e < NE; ++e) vin[e] = make_float2(0.f, 0.f);
    pred = 0.f;
    lim = ok ? 1024 : 0;
    edge = false;
    const bool interior = __all(ok && s0 >= 0);  // uniform
    raw = PCM && interior;
    if (!ok) return;
    const float *sr = s.pool + static_cast<unsigned long long>(en.slot) * s.state_len + s.state_len;  // sample p < 0 is sr[p]
    auto sample = [&](int p) -> float {
        if constexpr (PCM) return p < 0 ? sr[p] : pcm_sample(sp.x + en.s0, p, sp.scale);
        else return (p < 0 ? sr : a.x + en.s0)[p];
    };
    if (j == 0) pred = sample(s0 - 1);
    if (interior) {
        if constexpr (PCM) {
            const int16_t *p = sp.x + en.s0 + s0 + 2 * j;
#pragma unroll
            for (int e = 0; e < NE; ++e)
                if (e < NE - 3 || 2 * (j + 16 * e) < W) vin[e].x = pcm_raw_pair(p + 32 * e);
        } else {
            const float *src = a.x + en.s0 + s0;
            const bool pairs = __all((reinterpret_cast<uintptr_t>(src) & 7u) == 0u);  // uniform
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
        }
    } else {
#pragma unroll
        for (int e = 0; e < NE; ++e) {
            const int n2 = 2 * (j + 16 * e);
            if (e < NE - 3 || n2 < W) vin[e] = make_float2(sample(s0 + n2), sample(s0 + n2 + 1));
        }
    }
}

// Issues the loads of one quad of a flush launch: row g = i * L + u is row u of entry i, the frame whose first live sample lies at
// p0 = 160 (u - L) - W / 2 relative to the end of the stream whose state is pool row slots[i]; position p < 0 is pool[slot * S + S + p]
// (p0 - 1 >= -S), and every position at or beyond the end is nobody's: not fetched, and cleared after the pre-emphasis (lim = -p0,
// edge = true: the dense edge path's clear).  An entry whose slot lies outside the pool loads and (lim = 0) stores nothing.
template <int NE>
__device__ __forceinline__ void load_quad_nflush(const NemoArgs &a, const NemoFlushArgs &s, unsigned quad, unsigned total, int f, int j,
                                                 float2 (&vin)[NE], float &pred, int &lim, bool &edge)
{
    const unsigned q4 = quad * 4;                                           // uniform
    const unsigned g = q4 + min(static_cast<unsigned>(f), total - 1 - q4);  // lanes past the last row redo it
    const unsigned i = g / s.delay, u = g - i * s.delay;
    const int slot = s.slots[i];
    const bool ok = slot >= 0 && static_cast<unsigned>(slot) < s.pool_streams;
    const int W = static_cast<int>(a.win_len);
    const int p0 = (static_cast<int>(u) - static_cast<int>(s.delay)) * kHop - (W >> 1);
#pragma unroll
    for (int e = 0; e < NE; ++e) vin[e] = make_float2(0.f, 0.f);
    pred = 0.f;
    lim = ok ? -p0 : 0;
    edge = true;
    if (!ok) return;
    const float *sr = s.pool + static_cast<unsigned long long>(slot) * s.state_len + s.state_len + p0;  // the frame's position 0
    if (j == 0) pred = sr[-1];
#pragma unroll
    for (int e = 0; e < NE; ++e) {
        const int n2 = 2 * (j + 16 * e);
        const bool live = e < NE - 3 || n2 < W;
        if (live && n2 < lim) vin[e].x = sr[n2];
        if (live && n2 + 1 < lim) vin[e].y = sr[n2 + 1];
    }
}

// The trailing argument of a launch (the pool's or the flush's): the one element of the kernel's trailing pack, or nothing
struct NoPool {};
__device__ __forceinline__ NoPool pack_first() { return {}; }
template <typename T>
__device__ __forceinline__ const T &pack_first(const T &t) { return t; }

// the loads of `quad` for this lane group in a pool or flush build (the dense and packed builds call frame_of + load_quad_n)
template <int NE, int SRC, typename PL>
__device__ __forceinline__ void load_quad_pool_any(const NemoArgs &a, const PL &pl, unsigned quad, unsigned total, int f, int j, unsigned &cursor,
                                                   float2 (&vin)[NE], float &pred, int &lim, bool &edge, bool &raw)
{
    if constexpr (SRC == kNFlush) load_quad_nflush<NE>(a, pl, quad, total, f, j, vin, pred, lim, edge);
    else load_quad_npool<NE>(a, pl, quad, total, f, j, cursor, vin, pred, lim, edge, raw);
}

// SP: empty (equal-length clips, or packed clips with VARLEN), or the one trailing argument of a pool build -- a
// FrameStreamPackedArgs (float chunks: a.x), a FrameStreamPackedPcmArgs (16-bit PCM chunks) or a NemoFlushArgs; those builds leave
// VARLEN false and vl unused.
template <int NE, bool VARLEN, int WAVES, typename... SP>
__global__ __launch_bounds__(WAVES * 64) void ss_nemo_c256(const NemoArgs a, const NemoVarlenArgs vl, const SP... sp)
{
    constexpr bool PCM = (std::is_same_v<SP, FrameStreamPackedPcmArgs> || ...);
    constexpr bool POOL = PCM || (std::is_same_v<SP, FrameStreamPackedArgs> || ...);
    constexpr bool FLUSH = (std::is_same_v<SP, NemoFlushArgs> || ...);
    constexpr int SRC = PCM ? kNPoolPcm : POOL ? kNPool : FLUSH ? kNFlush : VARLEN ? kNVarlen : kNDense;
    static_assert(sizeof...(SP) == (POOL || FLUSH ? 1 : 0) && !((POOL || FLUSH) && VARLEN), "one pool argument, or none");
    [[maybe_unused]] const auto &pl = pack_first(sp...);
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

    unsigned total;
    if constexpr (POOL) total = pool_block(pl).total_rows;
    else if constexpr (FLUSH) total = pl.n_active * pl.delay;
    else total = VARLEN ? static_cast<unsigned>(vl.total_frames) : a.batch * a.n_frames;
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
    // one pass over the entries, spread over the grid: a bad entry raises the error word (stream_check_entries: a vector store).
    // (The flush's entries are checked by the launch that zeroes their rows.)
    if constexpr (POOL) stream_check_entries(pool_block(pl), blockIdx.x * (WAVES * 64) + tid, gridDim.x * (WAVES * 64));
    unsigned quad = __builtin_amdgcn_readfirstlane(q_lo + wave);  // uniform: kept scalar
    unsigned cursor = 0;
    if constexpr (VARLEN) {
        if (quad < q_hi) cursor = offset_find(vl.fo, vl.n_clips, static_cast<long long>(quad) * 4);
    }
    if constexpr (POOL) {
        if (quad < q_hi) cursor = offset_find(pool_block(pl).ro, pool_block(pl).n_active, static_cast<long long>(quad) * 4);
    }
    [[maybe_unused]] const int W = static_cast<int>(a.win_len);
    float2 vin[NE];
    float pred_next = 0.f;
    int lim_next = 0;
    bool edge_next = false;
    [[maybe_unused]] bool raw_next = false;  // PCM pool builds: vin[]'s pairs are raw dwords (load_quad_npool)
    if (quad < q_hi) {
        if constexpr (SRC == kNDense || SRC == kNVarlen) {
            const Frame fr = frame_of<VARLEN>(a, vl, quad, total, f, cursor);
            load_quad_n<NE>(fr, W, j, vin, pred_next, lim_next, edge_next);
        } else {
            load_quad_pool_any<NE, SRC>(a, pl, quad, total, f, j, cursor, vin, pred_next, lim_next, edge_next, raw_next);
        }
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
            if constexpr (SRC == kNPoolPcm) {
                // the pairs an interior quad left as raw dwords become the floats the float build loads (pcm_pair: exact; a raw
                // zero is the zero pair)
                if (raw_next) {
#pragma unroll
                    for (int e = 0; e < NE; ++e) s[e] = pcm_pair(__float_as_int(s[e].x), pl.scale);
                }
            }
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
            if constexpr (SRC == kNDense || SRC == kNVarlen) {
                const Frame fr = frame_of<VARLEN>(a, vl, next, total, f, cursor);
                load_quad_n<NE>(fr, W, j, vin, pred_next, lim_next, edge_next);
            } else {
                load_quad_pool_any<NE, SRC>(a, pl, next, total, f, j, cursor, vin, pred_next, lim_next, edge_next, raw_next);
            }
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

}  // namespace

}  // namespace ss
