// ss_kaldi_c256, the one copy of the kernel (ss_kaldi512.hip: the dense and packed builds; ss_kaldi512_pool.hip: the stream-pool builds).
// Everything behind the load -- the conditioning stage, both radix-16 passes, the untangle, the P row, the banded mel, ln, the DCT
// and the stores -- exists here once, so that a frame's bits do not depend on where its samples came from.  What a source kind
// (KSrc) adds is its row lookup and its loader:
//   * kDense / kVarlen: frame_src + load_quad_k (see ss_kaldi512.hip's header).
//   * kDensePcm / kVarlenPcm (a KaldiPcmArgs / KaldiVarlenPcmArgs in the trailing pack): frame_src over the int16 buffer +
//     load_quad_pcm -- one raw dword per sample pair at any parity, converted where the body consumes vin[].
//   * kPool / kPoolPcm (a FrameStreamPackedArgs / FrameStreamPackedPcmArgs in the kernel's trailing argument pack): the flat work
//     list is the packed output rows of a ragged streaming launch; a row is the tail of its entry's pool row followed by the head
//     of its chunk (load_quad_pool below).
#pragma once

#include "ss_device.h"
#include "ss_fft_reg.h"
#include "ss_internal.h"
#include "ss_quad256.h"
#include "ss_wave.h"

namespace ss {

namespace {  // (each kernel file has its own copy: the files that include this share no symbol)

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

// The source kinds of the body
enum KSrc : int { kDense = 0, kVarlen = 1, kPool = 2, kPoolPcm = 3, kDensePcm = 4, kVarlenPcm = 5 };

// (row_owner, the owner of a quad's row over a packed launch's or a pool launch's row offsets: ss_device.h, next to offset_seek)

// Where this lane group's frame starts and whether it exists.  Dense: lanes past the last frame redo it.  VARLEN: `cursor` is the
// wave's clip of its last quad's first row (claims only increase); a lane's frame lies at most three clips WITH rows further on.
// x: the call's samples, floats (a.x) or int16 (the PCM pack's): the offsets are in samples either way.  (Taken by reference, as
// `a` is: the float builds then compile to the instruction streams they had when this read a.x itself.)
template <bool VARLEN, typename T>
__device__ __forceinline__ const T *frame_src(const T *const &x, const KaldiArgs &a, const KaldiVarlenArgs &v, unsigned quad, unsigned total, int f, unsigned &cursor,
                                              bool &ok)
{
    const unsigned q4 = quad * 4;                                           // uniform
    const unsigned g = q4 + min(static_cast<unsigned>(f), total - 1 - q4);  // lanes past the last row redo it
    if constexpr (VARLEN) {
        const unsigned c = row_owner(v.fo, v.n_clips, q4, g, cursor);
        const KClip cl = kaldi_clip(v, a.flen, a.step, c);
        const long long tl = static_cast<long long>(g) - cl.f0;
        ok = cl.ok && tl >= 0 && tl < static_cast<long long>(cl.T);
        return x + (ok ? cl.s0 + tl * static_cast<long long>(a.step) : 0ll);
    } else {
        unsigned clip, t;
        locate_frame(q4, g - q4, a.n_frames, a.nf_magic, a.nf_shift, clip, t);
        ok = true;
        return x + static_cast<unsigned long long>(clip) * a.ld + static_cast<unsigned long long>(t) * a.step;
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

// The PCM form of load_quad_k: pair n = j + 16 e of the frame at src is ONE dword at 2-byte alignment (pcm_raw_pair), whatever the
// parity of the frame start -- odd ld, odd clip offset, odd shift, odd base -- so there is no pair / single split.  The dword stays
// raw in the pair's .x; the body converts it (pcm_pair) at the top of the iteration that consumes vin[]: converting here would wait
// for the loads right behind pass 1.  An odd frame length's half pair is one 16-bit load, kept as the low half of a raw word whose
// high half is zero (pcm_pair makes it (sample, 0)).  A raw zero is the pair (0, 0): beyond flen, and for a frame that does not
// exist, nothing is fetched -- a frame that ends on the buffer's last sample reads nothing past it.
template <int NE>
__device__ __forceinline__ void load_quad_pcm(const int16_t *src, bool ok, uint32_t flen, int j, float2 (&vin)[NE])
{
#pragma unroll
    for (int e = 0; e < NE; ++e) vin[e] = make_float2(0.f, 0.f);
    if (!ok) return;
    const int16_t *p = src + 2 * j;
#pragma unroll
    for (int e = 0; e < NE; ++e) {
        if (e < NE - 3) {
            vin[e].x = pcm_raw_pair(p + 32 * e);
        } else {
            const int rem = static_cast<int>(flen) - 2 * (j + 16 * e);
            if (rem >= 2) vin[e].x = pcm_raw_pair(p + 32 * e);
            else if (rem == 1) vin[e].x = __int_as_float(static_cast<int>(static_cast<uint16_t>(p[32 * e])));
        }
    }
}

// ---- pool builds: the row of a ragged streaming launch ----
// a sample pair at 4-byte alignment (gfx950 global loads take any alignment in the unaligned access mode the HSA ABI sets)
__device__ __forceinline__ float2 load_pair4(const float *p)
{
    float2 v;
    __builtin_memcpy(&v, __builtin_assume_aligned(p, 4), sizeof v);
    return v;
}

// the entry block of either pool argument
__device__ __forceinline__ const FrameStreamPackedArgs &pool_block(const FrameStreamPackedArgs &s) { return s; }
__device__ __forceinline__ const FrameStreamPackedArgs &pool_block(const FrameStreamPackedPcmArgs &s) { return s.e; }

// a lane that holds no raw PCM pair (see load_quad_pool)
constexpr int kNoRaw = -(1 << 30);

// Issues the loads of one quad of a pool launch: packed output row g = q4 + f belongs to the entry row_owner() finds over ro; row t
// of entry i is the Kaldi frame that starts at chunk sample s0 = t * step - S, sample p < 0 being pool[slot * S + S + p].  The frame
// ends inside the chunk (flen <= (D + 1) * step) and starts inside the pool row (s0 >= -S); beyond flen nothing is fetched (the `rem`
// tests of load_quad_k), so a frame that ends on the buffer's last sample reads nothing past it.  A lane whose entry
// stream_entry() finds bad, or whose row lies past the last entry, loads nothing and (ok = false) stores nothing.
// The choice between the two paths is per quad and wave-uniform, and changes no bit (both fetch the same samples):
//   * pairs: the frame length is even and no row's pair straddles the pool / chunk boundary (s0 >= 0, or s0 even) -- every pair
//     comes whole from one source: a float2 of the pool row's tail, or a float2 / one PCM dword of the chunk.  PCM builds keep the
//     dword as raw bits in the pair's .x; raw_from = s0 tells the consumer which pairs those are (pair n is raw where
//     raw_from + 2 n >= 0), and pcm_pair converts them at the top of the iteration that consumes vin[] -- converting here would wait
//     for the loads right behind pass 1.
//   * samples: any other quad (odd step or state length with a row that starts at an odd p < 0, an odd frame length's half pair):
//     single samples with a per-sample source select, PCM converted on the spot (raw_from = kNoRaw: nothing left to convert).
template <int NE, typename SPT>
__device__ __forceinline__ void load_quad_pool(const KaldiArgs &a, const SPT &sp, unsigned quad, unsigned total, int f, int j, unsigned &cursor,
                                               float2 (&vin)[NE], bool &ok, int &raw_from)
{
    constexpr bool PCM = std::is_same_v<SPT, FrameStreamPackedPcmArgs>;
    const FrameStreamPackedArgs &s = pool_block(sp);
    const unsigned q4 = quad * 4;                                           // uniform
    const unsigned g = q4 + min(static_cast<unsigned>(f), total - 1 - q4);  // lanes past the last row redo it
    const unsigned c = row_owner(s.ro, s.n_active, q4, g, cursor);
    const StreamEntry en = stream_entry(s, c);
    const long long tl = static_cast<long long>(g) - en.r0;
    ok = en.ok && tl >= 0 && tl < static_cast<long long>(en.R);
    const int flen = static_cast<int>(a.flen);
    // (t * step < n_i < 2^31)
    const int s0 = ok ? static_cast<int>(static_cast<unsigned>(tl) * a.step) - static_cast<int>(s.state_len) : 0;
    const bool pairs = (flen & 1) == 0 && __all(s0 >= 0 || (s0 & 1) == 0);
#pragma unroll
    for (int e = 0; e < NE; ++e) vin[e] = make_float2(0.f, 0.f);
    raw_from = kNoRaw;
    if (!ok) return;
    const float *sr = s.pool + static_cast<unsigned long long>(en.slot) * s.state_len + s.state_len;  // sample p < 0 is sr[p]
    [[maybe_unused]] const float *xf = a.x + en.s0;
    if (pairs) {
        if (PCM) raw_from = s0;
#pragma unroll
        for (int e = 0; e < NE; ++e) {
            const int n = j + 16 * e, p = s0 + 2 * n;
            if (e < NE - 3 || flen - 2 * n >= 2) {
                if constexpr (PCM) {
                    if (p < 0) vin[e] = load_pair4(sr + p);
                    else vin[e].x = pcm_raw_pair(sp.x + en.s0 + p);
                } else {
                    vin[e] = load_pair4((p < 0 ? sr : xf) + p);
                }
            }
        }
    } else {
        auto sample = [&](int p) -> float {
            if constexpr (PCM) return p < 0 ? sr[p] : pcm_sample(sp.x + en.s0, p, sp.scale);
            else return (p < 0 ? sr : xf)[p];
        };
#pragma unroll
        for (int e = 0; e < NE; ++e) {
            const int n = j + 16 * e, p = s0 + 2 * n;
            const int rem = e < NE - 3 ? 2 : flen - 2 * n;
            if (rem >= 1) vin[e].x = sample(p);
            if (rem >= 2) vin[e].y = sample(p + 1);
        }
    }
}

// The trailing argument of a launch (the pool's, or the PCM samples'): the one element of the kernel's trailing pack, or nothing
struct NoPool {};
__device__ __forceinline__ NoPool pack_first() { return {}; }
template <typename T>
__device__ __forceinline__ const T &pack_first(const T &t) { return t; }

// the clip tables of a packed launch: the kernel's own argument, or the ones the packed PCM pack carries
template <typename PL>
__device__ __forceinline__ const KaldiVarlenArgs &varlen_block(const KaldiVarlenArgs &vl, const PL &) { return vl; }
__device__ __forceinline__ const KaldiVarlenArgs &varlen_block(const KaldiVarlenArgs &, const KaldiVarlenPcmArgs &p) { return p.v; }

// the loads of `quad` for this lane group, whatever the source kind
template <int NE, int SRC, typename PL>
__device__ __forceinline__ void load_quad_any(const KaldiArgs &a, const KaldiVarlenArgs &vl, const PL &pl, unsigned quad, unsigned total, int f, int j,
                                              unsigned &cursor, float2 (&vin)[NE], bool &ok, int &raw_from)
{
    if constexpr (SRC == kPool || SRC == kPoolPcm) {
        load_quad_pool<NE>(a, pl, quad, total, f, j, cursor, vin, ok, raw_from);
    } else if constexpr (SRC == kDensePcm || SRC == kVarlenPcm) {
        const int16_t *src = frame_src<SRC == kVarlenPcm>(pl.x, a, vl, quad, total, f, cursor, ok);
        load_quad_pcm<NE>(src, ok, a.flen, j, vin);
    } else {
        const float *src = frame_src<SRC == kVarlen>(a.x, a, vl, quad, total, f, cursor, ok);
        load_quad_k<NE, SRC == kVarlen>(src, ok, a.flen, j, vin);
    }
}

// SP: empty (equal-length clips, or packed clips with VARLEN), or the pool's argument -- one FrameStreamPackedArgs (float chunks: a.x)
// or one FrameStreamPackedPcmArgs (16-bit PCM chunks); the pool builds leave VARLEN false and vl unused -- or the 16-bit PCM samples
// of a one-shot call: one KaldiPcmArgs (equal-length clips), or with VARLEN one KaldiVarlenPcmArgs (packed clips: its tables, vl unused).
template <int NE, bool POW2, bool MFCC, bool VARLEN, int WAVES, typename... SP>
__global__ __launch_bounds__(WAVES * 64) void ss_kaldi_c256(const KaldiArgs a, const KaldiVarlenArgs vl, const SP... sp)
{
    constexpr bool PCM = (std::is_same_v<SP, FrameStreamPackedPcmArgs> || ...);
    constexpr bool POOL = PCM || (std::is_same_v<SP, FrameStreamPackedArgs> || ...);
    constexpr bool DPCM = (std::is_same_v<SP, KaldiPcmArgs> || ...), VPCM = (std::is_same_v<SP, KaldiVarlenPcmArgs> || ...);
    constexpr int SRC = PCM ? kPoolPcm : POOL ? kPool : VPCM ? kVarlenPcm : DPCM ? kDensePcm : VARLEN ? kVarlen : kDense;
    static_assert(sizeof...(SP) == (POOL || DPCM || VPCM ? 1 : 0) && !(POOL && VARLEN), "one pool argument, or none");
    static_assert(!(DPCM && VARLEN) && (!VPCM || VARLEN), "the PCM pack follows the layout");
    [[maybe_unused]] const auto &pl = pack_first(sp...);
    [[maybe_unused]] const KaldiVarlenArgs &vt = varlen_block(vl, pl);
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

    unsigned total;
    if constexpr (POOL) total = pool_block(pl).total_rows;
    else total = VARLEN ? static_cast<unsigned>(vt.total_frames) : a.batch * a.n_frames;
    const unsigned quads = (total + 3) / 4;
    const unsigned q_lo = static_cast<unsigned>(static_cast<unsigned long long>(quads) * blockIdx.x / gridDim.x);
    const unsigned q_hi = static_cast<unsigned>(static_cast<unsigned long long>(quads) * (blockIdx.x + 1) / gridDim.x);
    stage_tables(s_tab, a.tab, (L::kMelW + 16 * a.mel_wpitch + 512) / 4, tid, WAVES * 64);
    if (tid == 0) *s_next = q_lo + WAVES;
    if constexpr (VARLEN) {
        // one pass over the clips, spread over the grid: an inconsistent clip raises the error word (a vector store to the pinned word)
        bool bad = false;
        for (unsigned b = blockIdx.x * (WAVES * 64) + tid; b < vt.n_clips; b += gridDim.x * (WAVES * 64)) bad |= !kaldi_clip(vt, a.flen, a.step, b).ok;
        if (bad && vt.err) __hip_atomic_store(vt.err, kVarlenError, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    // one pass over the entries, spread over the grid: a bad entry raises the error word (stream_check_entries: a vector store)
    if constexpr (POOL) stream_check_entries(pool_block(pl), blockIdx.x * (WAVES * 64) + tid, gridDim.x * (WAVES * 64));
    unsigned quad = __builtin_amdgcn_readfirstlane(q_lo + wave);  // uniform: kept scalar
    unsigned cursor = 0;
    if constexpr (VARLEN) {
        if (quad < q_hi) cursor = offset_find(vt.fo, vt.n_clips, static_cast<long long>(quad) * 4);
    }
    if constexpr (POOL) {
        if (quad < q_hi) cursor = offset_find(pool_block(pl).ro, pool_block(pl).n_active, static_cast<long long>(quad) * 4);
    }
    float2 vin[NE];
    bool ok_next = false;
    [[maybe_unused]] int raw_next = kNoRaw;  // PCM pool builds: which of vin[]'s pairs are raw dwords (load_quad_pool)
    if (quad < q_hi) load_quad_any<NE, SRC>(a, vt, pl, quad, total, f, j, cursor, vin, ok_next, raw_next);

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
            if constexpr (SRC == kPoolPcm) {
                // the pairs the loader left as raw dwords become the floats the float build loads (pcm_pair: exact)
#pragma unroll
                for (int e = 0; e < NE; ++e)
                    if (raw_next + 2 * (j + 16 * e) >= 0) s[e] = pcm_pair(__float_as_int(s[e].x), pl.scale);
            }
            if constexpr (SRC == kDensePcm || SRC == kVarlenPcm) {
                // every pair is a raw dword (load_quad_pcm; a raw zero is the float loader's zero pair)
#pragma unroll
                for (int e = 0; e < NE; ++e) s[e] = pcm_pair(__float_as_int(s[e].x), pl.scale);
            }
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
        if (next < q_hi) load_quad_any<NE, SRC>(a, vt, pl, next, total, f, j, cursor, vin, ok_next, raw_next);
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
                    for (int k = 0; k < 5; ++k) {
                        // (pool builds fetch the column again: five registers the loader needs more than this store does)
                        const int col = POOL ? s_filt[k * 16 + j] : fi[k];
                        if (col >= 0) row[col] = m[k];
                    }
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

}  // namespace

}  // namespace ss
