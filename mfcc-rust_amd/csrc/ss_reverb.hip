// Reverberation of packed clips from a bank of room impulse responses: ss_reverb_* of include/speechsauce_amd.h, whose comment is the
// definition; the reference crate has no such stage, so this file restates nothing of it.  The draws are Philox4x32-10 (ss_philox.h)
// in integer and f64 arithmetic, as in ss_noise.hip; a plan row is a pure function of (seed, epoch, clip id), the clip's segment and
// the bank.
//
// Two launches per combined call.
//   ss_reverb_plan_kernel      one lane per clip: the draws, the plan row.
//   ss_reverb_apply_kernel<T>  partitioned overlap-save in the frequency domain, B = 512 taps per partition, N = 1024 points.
//                              Workgroup (b, y) serves the groups y, y + gridDim.y, .. of clip b; a group is eight block pairs =
//                              8192 clip-relative output samples, one block pair per half-wave (32 lanes, 32 complex points per
//                              lane, the 32 x 32 register transform of ss_mel2048.hip with its one transposing exchange through
//                              wave-private LDS).  For partition p the half-wave loads the two real windows of its block pair as ONE
//                              complex signal (re: w[a .. a + N), im: w[a + B .. a + B + N), 48 dwords per lane since the two
//                              overlap), transforms it and accumulates FFT(z_p) . H_p in registers; H_p comes through LDS once
//                              per workgroup and partition (double-buffered: the next partition's 8 KiB are requested in front of
//                              the transform and written behind it, one barrier per partition).  One inverse transform per block
//                              pair, as a forward one between two exchanges of re and im; its last B real parts are the first
//                              block's outputs, its last B imaginary parts the second's (h is real: no untangle).  Where the
//                              clip's first output is 16-byte aligned the outputs pass through the exchange region once more
//                              and leave as 16-byte stores, otherwise as coalesced dwords.  Rows that are not reverberated are
//                              copied bit for bit by the same workgroups.  Lane 0 of workgroup (0, 0) stores epoch + 1 in the
//                              combined call.
// Blocks are clip-relative, so what a clip's lanes compute does not depend on where the clip lies in the packed block; float and PCM
// builds differ in the conversion on load alone (__fmul_rn: never contracted into the butterflies).
#include "ss_device.h"
#include "ss_fft_reg.h"
#include "ss_hip_staging.h"
#include "ss_host_checks.h"
#include "ss_internal.h"
#include "ss_philox.h"
#include "ss_reverb.h"
#include "ss_wave.h"

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <mutex>
#include <string>
#include <type_traits>
#include <vector>

// The handle: the normalised taps, the partition spectra behind the twiddle block, and the device copy of that block (made by the
// first device call, on the device that is current then).
struct ss_reverb_bank {
    std::vector<float> taps;     // every response, normalised, packed
    std::vector<int64_t> offs;   // n_rir + 1 offsets into taps
    std::vector<int64_t> peaks;  // first index of max |h| per response
    std::vector<ss::reverb::RirMeta> meta;
    std::vector<float> block;    // twiddles [kPartFloats], then kPartFloats per partition
    size_t max_taps = 0;
    std::mutex mu;
    void *d_block = nullptr;  // block, then meta
    int device = -1;
};

namespace ss {

namespace {

using namespace wv;
using reverb::RirMeta;

constexpr unsigned kB = reverb::kBlock, kN = reverb::kFft;
constexpr unsigned kWaves = 4, kThreads = kWaves * 64;
constexpr unsigned kGroup = 2 * kWaves * kN;  // clip-relative outputs of one workgroup pass: a block pair per half-wave
constexpr unsigned kStream = 0x30000u;        // counter word 1 of the draw: apart from SpecAugment's mask indices and the noise stage's words
constexpr unsigned long long kCountLimit = 1ull << 31;
constexpr int kExSlots = 2 * 16 * 34;  // float2 of a wave's exchange region: two transforms x half the columns (8704 B)

__host__ __device__ inline bool good_segment(long long lo, long long hi, unsigned long long total)
{
    return lo >= 0 && lo <= hi && static_cast<unsigned long long>(hi) <= total && hi - lo < static_cast<long long>(kCountLimit);
}

struct DrawScalars {
    unsigned long long total_samples;
    unsigned n_rir, clip_base;
    float prob;
};

// the plan row of clip b with the segment lo .. hi: the one definition ss_reverb_draws and the plan launch share
__host__ __device__ inline ss_reverb_plan_row draw_row(uint64_t seed, uint64_t epoch, const DrawScalars &d, unsigned b, long long lo, long long hi,
                                                       const RirMeta *meta)
{
    if (!good_segment(lo, hi, d.total_samples)) return ss_reverb_plan_row{-2, 0};
    const uint32_t id = d.clip_base + b;
    const Philox4 u = philox4x32_10(id, kStream, static_cast<uint32_t>(epoch), static_cast<uint32_t>(epoch >> 32), static_cast<uint32_t>(seed),
                                    static_cast<uint32_t>(seed >> 32));
    const uint64_t bar = static_cast<uint64_t>(static_cast<double>(d.prob) * 4294967296.0);
    if (d.n_rir == 0 || !(static_cast<uint64_t>(u.w[0]) < bar)) return ss_reverb_plan_row{-1, 0};
    const uint32_t c = static_cast<uint32_t>((static_cast<uint64_t>(u.w[1]) * d.n_rir) >> 32);
    return ss_reverb_plan_row{static_cast<int32_t>(c), meta[c].shift};
}

__global__ __launch_bounds__(256) void ss_reverb_plan_kernel(const long long *__restrict__ so, const unsigned long long *__restrict__ rng, DrawScalars d,
                                                            const RirMeta *__restrict__ meta, unsigned n_clips, ss_reverb_plan_row *__restrict__ plan)
{
    const unsigned b = blockIdx.x * 256u + threadIdx.x;
    if (b < n_clips) plan[b] = draw_row(rng[0], rng[1], d, b, so[b], so[b + 1], meta);
}

// sample i of a float block, or of a 16-bit PCM block with its power-of-two scale (the product is exact)
template <typename T>
__device__ __forceinline__ float sample(const T *p, size_t i, float scale)
{
    if constexpr (std::is_same<T, float>::value) return p[i];
    else return __fmul_rn(static_cast<float>(p[i]), scale);
}
// the same as the word that is stored: a float sample keeps every bit (NaN payloads, -0.0, denormals)
template <typename T>
__device__ __forceinline__ unsigned sample_bits(const T *p, size_t i, float scale)
{
    if constexpr (std::is_same<T, float>::value) return reinterpret_cast<const unsigned *>(p)[i];
    else return __float_as_uint(__fmul_rn(static_cast<float>(p[i]), scale));
}

// A value every lane of the wave holds alike, moved to scalar registers.  The tables are read with vector loads (the kernel also
// stores, so the compiler may not use scalar loads for them): left in vector registers the clip's bounds, its row and the response's
// sizes cost ~20 registers for the whole kernel.
__device__ __forceinline__ int uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ long long uniform(long long v)
{
    const unsigned lo = __builtin_amdgcn_readfirstlane(static_cast<unsigned>(v));
    const unsigned hi = __builtin_amdgcn_readfirstlane(static_cast<unsigned>(static_cast<unsigned long long>(v) >> 32));
    return static_cast<long long>((static_cast<unsigned long long>(hi) << 32) | lo);
}

struct ApplyArgs {
    const long long *so;
    const ss_reverb_plan_row *plan;
    const RirMeta *meta;
    const float *tw;    // the twiddle block
    const float *spec;  // the partition spectra
    unsigned long long total_samples;
    unsigned n_clips, n_rir;
    float x_scale;
};

// 1024-point forward transform of the half-wave's v (lane j: points j + 32 e) into u (lane j: bins j + 32 q): radix-32, the
// transposing exchange through the half's slice of the wave's region in two register halves, twiddles, radix-32 -- the transform
// of ss_mel2048.hip.  v is consumed.
__device__ __forceinline__ void fft1024(float2 (&v)[32], float2 (&u)[32], float2 *exf, const float4 *s_tw, int j)
{
    fft_reg<32>(v);
    const int wbh = 34 * (j >> 1) + (j & 1);
    const int jl = j & 15;
#pragma unroll
    for (int k = 0; k < 16; ++k) exf[wbh + 2 * k] = v[k];
    wave_order();
    // every lane fills u in ONE of the two half-wave phases: "defined" here (an empty asm per register, no instruction)
#pragma unroll
    for (int k = 0; k < 32; ++k) u[k] = make_float2(defined_garbage(), defined_garbage());
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
    for (int p = 0; p < 16; ++p) {  // two twiddles per ds_read_b128: W^(j 2p), W^(j (2p + 1))
        const float4 w2 = s_tw[p * 32 + j];
        if (p > 0) u[2 * p] = cmul(u[2 * p], make_float2(w2.x, w2.y));
        u[2 * p + 1] = cmul(u[2 * p + 1], make_float2(w2.z, w2.w));
    }
    fft_reg<32>(u);
}

// The not-reverberated clip's samples [i0, i1) as they are: 16-byte stores over the aligned middle, single words at its ends.
template <typename T>
__device__ __forceinline__ void copy_range(const T *xc, float *oc, unsigned i0, unsigned i1, float scale, unsigned tid)
{
    const unsigned lead = (4u - (static_cast<unsigned>(reinterpret_cast<uintptr_t>(oc + i0) >> 2) & 3u)) & 3u;
    const unsigned m0 = i0 + lead < i1 ? i0 + lead : i1, quads = (i1 - m0) / 4, m1 = m0 + 4 * quads;
    unsigned *ow = reinterpret_cast<unsigned *>(oc);
    if (tid < m0 - i0) ow[i0 + tid] = sample_bits(xc, i0 + tid, scale);
    if (tid < i1 - m1) ow[m1 + tid] = sample_bits(xc, m1 + tid, scale);
    for (unsigned q = tid; q < quads; q += kThreads) {
        const unsigned i = m0 + 4 * q;
        T xv[4];
        __builtin_memcpy(xv, __builtin_assume_aligned(xc + i, sizeof(T)), sizeof xv);
        *reinterpret_cast<uint4 *>(ow + i) = make_uint4(sample_bits(xv, 0, scale), sample_bits(xv, 1, scale), sample_bits(xv, 2, scale), sample_bits(xv, 3, scale));
    }
}

template <typename T>
__global__ __launch_bounds__(kThreads, 2) void ss_reverb_apply_kernel(const T *__restrict__ x, ApplyArgs a, float *__restrict__ out, unsigned long long *rng)
{
    __shared__ __attribute__((aligned(16))) float s_tw[reverb::kPartFloats];
    __shared__ __attribute__((aligned(16))) float s_h[2][reverb::kPartFloats];
    __shared__ __attribute__((aligned(16))) float2 s_ex[kWaves][kExSlots];
    if (rng && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) {  // the combined call: epoch + 1, both dwords in one vector store
        const unsigned long long e = rng[1] + 1;
        *reinterpret_cast<uint2 *>(rng + 1) = make_uint2(static_cast<unsigned>(e), static_cast<unsigned>(e >> 32));
    }
    const unsigned b = blockIdx.x, tid = threadIdx.x;
    const long long lo = uniform(a.so[b]), hi = uniform(a.so[b + 1]);
    if (!good_segment(lo, hi, a.total_samples)) return;  // everything up to the loops is uniform per workgroup
    const int rir = uniform(a.plan[b].rir), shift = uniform(a.plan[b].shift);
    if (rir == -2) return;
    const unsigned L = static_cast<unsigned>(hi - lo), groups = (L + kGroup - 1) / kGroup;
    if (blockIdx.y >= groups) return;
    const T *xc = x + lo;
    float *oc = out + lo;
    RirMeta m{0, 0, 0, 0};
    bool conv = rir >= 0 && static_cast<unsigned>(rir) < a.n_rir;
    if (conv) {
        m = RirMeta{uniform(a.meta[rir].taps), uniform(a.meta[rir].parts), 0, uniform(a.meta[rir].first)};
        conv = shift >= 0 && shift < m.taps;
    }
    if (!conv) {  // not reverberated, or a row that is out of range for the bank: a copy
        for (unsigned k = blockIdx.y; k < groups; k += gridDim.y) {
            const unsigned i0 = k * kGroup, i1 = L - i0 < kGroup ? L : i0 + kGroup;
            copy_range(xc, oc, i0, i1, a.x_scale, tid);
        }
        return;
    }
    const int wave = __builtin_amdgcn_readfirstlane(static_cast<int>(tid >> 6));  // uniform: kept scalar, and what derives from it
    const float4 *tw4 = reinterpret_cast<const float4 *>(s_tw);
    const float4 *spec4 = reinterpret_cast<const float4 *>(a.spec) + static_cast<size_t>(m.first) * (reverb::kPartFloats / 4);
    const int parts = m.parts;
    const bool wide = (reinterpret_cast<uintptr_t>(oc) & 15u) == 0;  // the clip's first output is 16-byte aligned: so is every block's
    stage_tables(s_tw, a.tw, reverb::kPartFloats / 4, static_cast<int>(tid), kThreads);

    for (unsigned k = blockIdx.y; k < groups; k += gridDim.y) {
        // what depends on the lane number only is derived again in every pass (the lane number is made opaque here and behind the
        // partitions): hoisted out of the loops these values -- output addresses above all -- live in ~70 registers for the whole
        // kernel and spill
        int lane = static_cast<int>(tid & 63);
        asm volatile("" : "+v"(lane));
        int half = (lane >> 5) & 1, j = lane & 31;
        float2 *exf = s_ex[wave] + half * (16 * 34);
        // this half-wave's block pair: outputs [o0, o0 + N) of the clip; o0 < 2^31 + kGroup
        long long o0 = static_cast<long long>(k) * kGroup + static_cast<long long>(2 * wave + half) * kN;
        const bool wave_live = static_cast<long long>(k) * kGroup + static_cast<long long>(2 * wave) * kN < static_cast<long long>(L);
        float2 acc[32];
#pragma unroll
        for (int q = 0; q < 32; ++q) acc[q] = make_float2(0.f, 0.f);
        // partition 0's spectrum: the barrier in front keeps the last pass's readers of the buffer (and, first time, nothing) apart
        __syncthreads();
        {
            unsigned tl = tid;
            asm volatile("" : "+v"(tl));
            float4 *dst = reinterpret_cast<float4 *>(s_h[0]);
            dst[tl] = spec4[tl];
            dst[tl + kThreads] = spec4[tl + kThreads];
        }
        __syncthreads();
        for (int p = 0; p < parts; ++p) {
            float4 hn[2] = {make_float4(0.f, 0.f, 0.f, 0.f), make_float4(0.f, 0.f, 0.f, 0.f)};
            unsigned tl = tid;
            asm volatile("" : "+v"(tl));
            if (p + 1 < parts) {
                const float4 *src = spec4 + static_cast<size_t>(p + 1) * (reverb::kPartFloats / 4);
                hn[0] = src[tl];
                hn[1] = src[tl + kThreads];
            }
            // the windows of partition p: clip samples [ap0, ap0 + 3B + N) for the wave, this half's 3B of them from ap0 + half N
            const long long ap0 = static_cast<long long>(k) * kGroup + static_cast<long long>(2 * wave) * kN + shift - static_cast<long long>(kB) -
                                  static_cast<long long>(p) * kB;
            constexpr long long kSpan = 3 * kB + kN;
            const bool work = wave_live && ap0 < static_cast<long long>(L) && ap0 + kSpan > 0;  // uniform per wave
            float s[48];
            if (work) {
                const unsigned first = static_cast<unsigned>(half) * kN + static_cast<unsigned>(j);  // this lane's first sample of the span
                if (ap0 >= 0 && ap0 + kSpan <= static_cast<long long>(L)) {  // uniform base + a 32-bit lane offset
                    const T *wb = xc + ap0;
#pragma unroll
                    for (int t = 0; t < 48; ++t) s[t] = sample(wb, first + 32u * t, a.x_scale);
                } else {
                    // a clip edge: samples outside the clip's own segment are +0.0.  -kSpan < ap0 < L < 2^31: as an unsigned word an
                    // index below 0 is at least 2^32 - kSpan, and none above wraps
                    const unsigned u0 = static_cast<unsigned>(static_cast<int>(ap0)) + first;
#pragma unroll
                    for (int t = 0; t < 48; ++t) {
                        const unsigned i = u0 + 32u * t;
                        s[t] = i < L ? sample(xc, i, a.x_scale) : 0.f;
                    }
                }
            }
            // the next spectrum goes to the buffer nobody reads in this pass as soon as it is here: it was requested first
            if (p + 1 < parts) {
                float4 *dst = reinterpret_cast<float4 *>(s_h[(p + 1) & 1]);
                dst[tl] = hn[0];
                dst[tl + kThreads] = hn[1];
            }
            if (work) {
                float2 v[32], u[32];
#pragma unroll
                for (int e = 0; e < 32; ++e) v[e] = make_float2(s[e], s[e + 16]);
                fft1024(v, u, exf, tw4, j);
                const float4 *h4 = reinterpret_cast<const float4 *>(s_h[p & 1]);
#pragma unroll
                for (int t = 0; t < 16; ++t) {  // acc += u . H, two bins per ds_read_b128
                    const float4 h = h4[t * 32 + j];
                    acc[2 * t].x = fmaf(-u[2 * t].y, h.y, fmaf(u[2 * t].x, h.x, acc[2 * t].x));
                    acc[2 * t].y = fmaf(u[2 * t].y, h.x, fmaf(u[2 * t].x, h.y, acc[2 * t].y));
                    acc[2 * t + 1].x = fmaf(-u[2 * t + 1].y, h.w, fmaf(u[2 * t + 1].x, h.z, acc[2 * t + 1].x));
                    acc[2 * t + 1].y = fmaf(u[2 * t + 1].y, h.z, fmaf(u[2 * t + 1].x, h.w, acc[2 * t + 1].y));
                }
            }
            __syncthreads();
        }
        if (!wave_live) continue;
        asm volatile("" : "+v"(lane));
        half = (lane >> 5) & 1;
        j = lane & 31;
        exf = s_ex[wave] + half * (16 * 34);
        o0 = static_cast<long long>(k) * kGroup + static_cast<long long>(2 * wave + half) * kN;
        // ifft(Y) = swap(fft(swap(Y))) / N: point n = j + 32 q of the result is (u[q].y, u[q].x) / N
        float2 v[32], u[32];
#pragma unroll
        for (int e = 0; e < 32; ++e) v[e] = make_float2(acc[e].y, acc[e].x);
        fft1024(v, u, exf, tw4, j);
        constexpr float inv = 1.0f / static_cast<float>(kN);  // a power of two: exact
        if (wide) {
            // points N/2 .. N - 1 through the half's slice: re -> floats [0, B), im -> [B, 2B); then four consecutive outputs per lane
            float *ot = reinterpret_cast<float *>(exf);
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                ot[j + 32 * q] = u[16 + q].y * inv;
                ot[kB + j + 32 * q] = u[16 + q].x * inv;
            }
            wave_order();
#pragma unroll
            for (int t = 0; t < 8; ++t) {
                const int n = 4 * (j + 32 * t);
                const float4 r = *reinterpret_cast<const float4 *>(ot + n);
                const long long i = o0 + n;
                if (i + 4 <= static_cast<long long>(L)) {
                    *reinterpret_cast<float4 *>(oc + i) = r;
                } else {
                    if (i < static_cast<long long>(L)) oc[i] = r.x;
                    if (i + 1 < static_cast<long long>(L)) oc[i + 1] = r.y;
                    if (i + 2 < static_cast<long long>(L)) oc[i + 2] = r.z;
                }
            }
            wave_order();
        } else {
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const long long i = o0 + j + 32 * q;
                if (i < static_cast<long long>(L)) oc[i] = u[16 + q].y * inv;
                if (i + kB < static_cast<long long>(L)) oc[i + kB] = u[16 + q].x * inv;
            }
        }
    }
}

// ---- host side ----

struct Call {  // the arguments every form shares
    const void *x;
    size_t n_clips;
    const int64_t *so;
    size_t total_samples;
    size_t elem;  // bytes per sample of x: 4 or 2
};

int check_counts(size_t n_clips, size_t total_samples)
{
    if (n_clips >= kCountLimit || total_samples >= kCountLimit) return fail(SS_ERR_ARG, "n_clips and total_samples must be below 2^31");
    return SS_OK;
}

int check_draw_scalars(size_t clip_base, size_t n_clips, float prob)
{
    if (!(prob >= 0.0f && prob <= 1.0f)) return fail(SS_ERR_ARG, "prob must lie in [0, 1]");
    if (clip_base > (1ull << 32) || n_clips > (1ull << 32) - clip_base) return fail(SS_ERR_ARG, "clip_base + n_clips must not exceed 2^32");
    return SS_OK;
}

// null buffers, alignment and the overlap rules; x, out and rng are null where the form has none
int check_buffers(const Call &c, const ss_reverb_bank *bank, const float *out, const ss_reverb_plan_row *plan, const uint64_t *rng, bool has_x, bool has_rng)
{
    if (!bank || !c.so || !plan || (has_x && (!c.x || !out)) || (has_rng && !rng)) return fail(SS_ERR_ARG, "null buffer");
    const auto off = [](const void *p, size_t a) { return reinterpret_cast<uintptr_t>(p) % a != 0; };
    if (off(c.x, c.elem) || off(out, 4)) return fail(SS_ERR_ARG, "samples and out must be aligned to their element size");
    if (off(c.so, 8) || off(plan, 8) || off(rng, 8)) return fail(SS_ERR_ARG, "the offset table, plan and rng must be 8-byte aligned");
    const size_t xbytes = has_x ? c.total_samples * c.elem : 0, obytes = has_x ? c.total_samples * sizeof(float) : 0;
    const size_t pbytes = c.n_clips * sizeof(ss_reverb_plan_row), rbytes = has_rng ? 16u : 0u;
    if (xbytes && ranges_overlap(c.x, xbytes, out, obytes)) return fail(SS_ERR_ARG, "out overlaps the samples: the convolution is not in place");
    const struct {
        const void *p;
        size_t bytes;
        const char *name;
    } others[] = {{plan, pbytes, "plan"}, {rng, rbytes, "rng"}};
    for (const auto &o : others)
        if (o.bytes && ((xbytes && ranges_overlap(c.x, xbytes, o.p, o.bytes)) || (obytes && ranges_overlap(out, obytes, o.p, o.bytes))))
            return fail(SS_ERR_ARG, std::string(o.name) + " overlaps the samples or out");
    if (rbytes && ranges_overlap(plan, pbytes, rng, rbytes)) return fail(SS_ERR_ARG, "rng overlaps plan");
    return SS_OK;
}

struct DeviceBank {
    const float *tw, *spec;
    const RirMeta *meta;
};

int device_bank(const ss_reverb_bank *bank_c, DeviceBank *d)
{
    ss_reverb_bank *t = const_cast<ss_reverb_bank *>(bank_c);  // the lazy upload is the handle's one mutable part
    std::lock_guard<std::mutex> lock(t->mu);
    int dev = -1;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return no_device();
    const size_t fbytes = t->block.size() * sizeof(float), mbytes = t->meta.size() * sizeof(RirMeta);
    if (!t->d_block) {
        void *p = nullptr;
        e = hipMalloc(&p, fbytes + (mbytes ? mbytes : 16));
        if (e == hipSuccess) e = hipMemcpy(p, t->block.data(), fbytes, hipMemcpyHostToDevice);
        if (e == hipSuccess && mbytes) e = hipMemcpy(static_cast<char *>(p) + fbytes, t->meta.data(), mbytes, hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            if (p) (void)hipFree(p);
            return hip_fail(e, "reverb bank upload");
        }
        t->d_block = p;
        t->device = dev;
    } else if (dev != t->device) {
        return fail(SS_ERR_ARG, "the bank's spectra live on device " + std::to_string(t->device) + ", the current device is " + std::to_string(dev));
    }
    d->tw = static_cast<const float *>(t->d_block);
    d->spec = d->tw + reverb::kPartFloats;
    d->meta = reinterpret_cast<const RirMeta *>(static_cast<const char *>(t->d_block) + fbytes);
    return SS_OK;
}

int launch_plan(const Call &c, const ss_reverb_bank *bank, const DeviceBank &db, const uint64_t *d_rng, size_t clip_base, float prob, ss_reverb_plan_row *d_plan,
                hipStream_t stream)
{
    const DrawScalars d{c.total_samples, static_cast<unsigned>(bank->meta.size()), static_cast<unsigned>(clip_base), prob};
    const unsigned n = static_cast<unsigned>(c.n_clips);
    hipLaunchKernelGGL(ss_reverb_plan_kernel, dim3((n + 255u) / 256u), dim3(256), 0, stream, reinterpret_cast<const long long *>(c.so),
                       reinterpret_cast<const unsigned long long *>(d_rng), d, db.meta, n, d_plan);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "ss_reverb_plan_kernel");
    note_kernel("ss_reverb_plan_kernel");
    return SS_OK;
}

// d_rng != nullptr: the combined call, whose apply launch stores epoch + 1
template <typename T>
int launch_apply(const Call &c, const ss_reverb_bank *bank, const DeviceBank &db, float x_scale, const ss_reverb_plan_row *d_plan, float *d_out, uint64_t *d_rng,
                 hipStream_t stream)
{
    const ApplyArgs a{reinterpret_cast<const long long *>(c.so), d_plan, db.meta, db.tw, db.spec, c.total_samples, static_cast<unsigned>(c.n_clips),
                      static_cast<unsigned>(bank->meta.size()), x_scale};
    const dim3 grid(static_cast<unsigned>(c.n_clips), packed_split(c.n_clips, (c.total_samples + kGroup - 1) / kGroup));
    hipLaunchKernelGGL(ss_reverb_apply_kernel<T>, grid, dim3(kThreads), 0, stream, static_cast<const T *>(c.x), a, d_out, reinterpret_cast<unsigned long long *>(d_rng));
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "ss_reverb_apply_kernel");
    note_kernel(sizeof(T) == 4 ? "ss_reverb_apply_kernel<f32>" : "ss_reverb_apply_kernel<i16>");
    return SS_OK;
}

int check_scale(size_t elem, float x_scale) { return elem == 4 ? SS_OK : check_pcm_scale(x_scale); }

int plan_device(const Call &c, const ss_reverb_bank *bank, const uint64_t *d_rng, size_t clip_base, float prob, ss_reverb_plan_row *d_plan, void *stream)
{
    if (c.n_clips == 0) return SS_OK;
    int rc = check_counts(c.n_clips, c.total_samples);
    if (rc || (rc = check_buffers(c, bank, nullptr, d_plan, d_rng, false, true)) || (rc = check_draw_scalars(clip_base, c.n_clips, prob))) return rc;
    DeviceBank db;
    if ((rc = device_bank(bank, &db))) return rc;
    return launch_plan(c, bank, db, d_rng, clip_base, prob, d_plan, static_cast<hipStream_t>(stream));
}

// d_rng != nullptr: plan + apply and the epoch bump; otherwise apply on the caller's plan
template <typename T>
int run_device(const Call &c, const ss_reverb_bank *bank, float x_scale, uint64_t *d_rng, bool combined, size_t clip_base, float prob, float *d_out,
               ss_reverb_plan_row *d_plan, void *stream)
{
    if (c.n_clips == 0) return SS_OK;
    int rc = check_counts(c.n_clips, c.total_samples);
    if (rc || (rc = check_buffers(c, bank, d_out, d_plan, d_rng, true, combined)) || (combined && (rc = check_draw_scalars(clip_base, c.n_clips, prob))) ||
        (rc = check_scale(c.elem, x_scale)))
        return rc;
    DeviceBank db;
    if ((rc = device_bank(bank, &db))) return rc;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    if (combined && (rc = launch_plan(c, bank, db, d_rng, clip_base, prob, d_plan, st))) return rc;
    return launch_apply<T>(c, bank, db, x_scale, d_plan, d_out, combined ? d_rng : nullptr, st);
}

// The host-pointer forms (synchronous).  The table is checked on the host before the device is touched; a checked table covers
// samples 0 .. so[n_clips) without a gap, so exactly those come down.  out goes up first: a caller's plan may leave rows unwritten.
template <typename T>
int host_call(const char *name, const Call &c, const ss_reverb_bank *bank, float x_scale, uint64_t *rng, bool combined, size_t clip_base, float prob, float *out,
              ss_reverb_plan_row *plan)
{
    if (c.n_clips == 0) return SS_OK;
    int rc = check_counts(c.n_clips, c.total_samples);
    if (rc || (rc = check_buffers(c, bank, out, plan, rng, true, combined)) || (combined && (rc = check_draw_scalars(clip_base, c.n_clips, prob))) ||
        (rc = check_scale(c.elem, x_scale)) || (rc = check_clip_table(c.so, c.n_clips, c.total_samples)))
        return rc;
    if (!have_device()) return no_device();
    const size_t covered = static_cast<size_t>(c.so[c.n_clips]);
    const size_t xbytes = c.total_samples * c.elem, obytes = c.total_samples * sizeof(float), pbytes = c.n_clips * sizeof(ss_reverb_plan_row);
    HostStage st(name);
    Call d = c;
    d.x = st.up(static_cast<const char *>(c.x), xbytes);
    float *d_out = st.room<float>(obytes);
    if (!combined) st.fill(d_out, out, covered * sizeof(float));
    d.so = st.up(c.so, (c.n_clips + 1) * sizeof(int64_t));
    ss_reverb_plan_row *d_plan = combined ? st.room<ss_reverb_plan_row>(pbytes) : st.up(plan, pbytes);
    uint64_t *d_rng = combined ? st.up(rng, 16) : nullptr;
    if (st.ok()) st.ran(run_device<T>(d, bank, x_scale, d_rng, combined, clip_base, prob, d_out, d_plan, nullptr));
    st.sync();
    st.down(out, d_out, covered * sizeof(float));
    if (combined) {
        st.down(plan, d_plan, pbytes);
        st.down(rng + 1, d_rng + 1, 8);  // of the generator's two words the advanced counter alone
    }
    return st.status();
}

}  // namespace

}  // namespace ss

#define SS_REVERB_CALL(elem) \
    ss::Call { x, n_clips, sample_offsets, total_samples, elem }
#define SS_REVERB_DCALL(elem) \
    ss::Call { d_x, n_clips, d_sample_offsets, total_samples, elem }

extern "C" {

int ss_reverb_bank_create(const float *rir, size_t n_rir, const int64_t *rir_offsets, size_t total_rir, int normalize, int align_peak, ss_reverb_bank **bank)
{
    if (!bank) return ss::fail(SS_ERR_ARG, "null output");
    *bank = nullptr;
    if (!rir_offsets || (total_rir && !rir)) return ss::fail(SS_ERR_ARG, "null buffer");
    if (normalize < 0 || normalize > 2) return ss::fail(SS_ERR_ARG, "normalize must be 0 (as given), 1 (unit energy) or 2 (unit peak)");
    if (align_peak < 0 || align_peak > 1) return ss::fail(SS_ERR_ARG, "align_peak must be 0 or 1");
    if (n_rir >= ss::kCountLimit / ss::reverb::kMaxParts || total_rir >= (1ull << 40)) return ss::fail(SS_ERR_ARG, "n_rir must be below 2^26 and total_rir below 2^40");
    if (rir_offsets[0] != 0) return ss::fail(SS_ERR_ARG, "rir_offsets[0] must be 0");
    for (size_t c = 0; c < n_rir; ++c) {
        const int64_t lo = rir_offsets[c], hi = rir_offsets[c + 1];
        if (hi <= lo) return ss::fail(SS_ERR_ARG, "response " + std::to_string(c) + " is empty or reversed");
        if (hi - lo > static_cast<int64_t>(ss::reverb::kMaxTaps))
            return ss::fail(SS_ERR_ARG, "response " + std::to_string(c) + " has " + std::to_string(hi - lo) + " taps, at most 16384 are served");
        if (static_cast<uint64_t>(hi) > total_rir) return ss::fail(SS_ERR_ARG, "response " + std::to_string(c) + " ends past total_rir");
        for (int64_t k = lo; k < hi; ++k)
            if (!std::isfinite(rir[k])) return ss::fail(SS_ERR_ARG, "response " + std::to_string(c) + " holds a tap that is not finite");
    }
    ss_reverb_bank *t = new ss_reverb_bank;
    t->offs.assign(rir_offsets, rir_offsets + n_rir + 1);
    ss::reverb::build_twiddles(t->block);
    std::vector<float> h;
    int32_t first = 0;
    for (size_t c = 0; c < n_rir; ++c) {
        const size_t lo = static_cast<size_t>(rir_offsets[c]), n = static_cast<size_t>(rir_offsets[c + 1]) - lo;
        const size_t peak = ss::reverb::normalise_taps(rir + lo, n, normalize, h);
        t->taps.insert(t->taps.end(), h.begin(), h.end());
        t->peaks.push_back(static_cast<int64_t>(peak));
        const int32_t parts = static_cast<int32_t>((n + ss::reverb::kBlock - 1) / ss::reverb::kBlock);
        t->meta.push_back(ss::reverb::RirMeta{static_cast<int32_t>(n), parts, align_peak ? static_cast<int32_t>(peak) : 0, first});
        ss::reverb::append_partition_spectra(h.data(), n, t->block);
        first += parts;
        if (n > t->max_taps) t->max_taps = n;
    }
    *bank = t;
    return SS_OK;
}

void ss_reverb_bank_destroy(ss_reverb_bank *bank)
{
    if (!bank) return;
    if (bank->d_block) (void)hipFree(bank->d_block);
    delete bank;
}

int ss_reverb_bank_info(const ss_reverb_bank *bank, size_t *n_rir, size_t *block, size_t *max_taps, size_t *n_partitions)
{
    if (!bank || !n_rir || !block || !max_taps || !n_partitions) return ss::fail(SS_ERR_ARG, "null argument");
    *n_rir = bank->meta.size();
    *block = ss::reverb::kBlock;
    *max_taps = bank->max_taps;
    *n_partitions = bank->block.size() / ss::reverb::kPartFloats - 1;
    return SS_OK;
}

int ss_reverb_bank_rir(const ss_reverb_bank *bank, size_t c, float *taps, size_t cap, size_t *n_taps, size_t *peak)
{
    if (!bank || !n_taps || !peak) return ss::fail(SS_ERR_ARG, "null argument");
    if (c >= bank->meta.size()) return ss::fail(SS_ERR_ARG, "response " + std::to_string(c) + " is outside the bank of " + std::to_string(bank->meta.size()));
    const size_t n = static_cast<size_t>(bank->meta[c].taps);
    *n_taps = n;
    *peak = static_cast<size_t>(bank->peaks[c]);
    if (!taps) return SS_OK;  // the sizes alone
    if (cap < n) return ss::fail(SS_ERR_ARG, "cap is below the response's " + std::to_string(n) + " taps");
    std::memcpy(taps, bank->taps.data() + (bank->offs[c] - bank->offs[0]), n * sizeof(float));
    return SS_OK;
}

int ss_reverb_bank_spectrum(const ss_reverb_bank *bank, size_t c, size_t p, float *out)
{
    if (!bank || !out) return ss::fail(SS_ERR_ARG, "null argument");
    if (c >= bank->meta.size()) return ss::fail(SS_ERR_ARG, "response " + std::to_string(c) + " is outside the bank of " + std::to_string(bank->meta.size()));
    if (p >= static_cast<size_t>(bank->meta[c].parts)) return ss::fail(SS_ERR_ARG, "partition " + std::to_string(p) + " is outside the response's " + std::to_string(bank->meta[c].parts));
    const float *src = bank->block.data() + (1 + static_cast<size_t>(bank->meta[c].first) + p) * ss::reverb::kPartFloats;
    for (unsigned j = 0; j < 32; ++j)
        for (unsigned r = 0; r < 32; ++r) {
            out[2 * (j + 32 * r)] = src[ss::reverb::part_slot(r, j)];
            out[2 * (j + 32 * r) + 1] = src[ss::reverb::part_slot(r, j) + 1];
        }
    return SS_OK;
}

// host only, no device: the rows the plan launch writes, from the same draw_row
int ss_reverb_draws(const uint64_t *rng, size_t clip_base, size_t n_clips, const int64_t *sample_offsets, size_t total_samples, const ss_reverb_bank *bank, float prob,
                    ss_reverb_plan_row *plan)
{
    if (n_clips == 0) return SS_OK;
    if (!rng || !sample_offsets || !plan || !bank) return ss::fail(SS_ERR_ARG, "null buffer");
    int rc = ss::check_counts(n_clips, total_samples);
    if (rc || (rc = ss::check_draw_scalars(clip_base, n_clips, prob))) return rc;
    const ss::DrawScalars d{total_samples, static_cast<unsigned>(bank->meta.size()), static_cast<unsigned>(clip_base), prob};
    for (size_t b = 0; b < n_clips; ++b) plan[b] = ss::draw_row(rng[0], rng[1], d, static_cast<unsigned>(b), sample_offsets[b], sample_offsets[b + 1], bank->meta.data());
    return SS_OK;
}

int ss_reverb_plan_packed_device(size_t n_clips, const int64_t *d_sample_offsets, size_t total_samples, const ss_reverb_bank *bank, const uint64_t *d_rng,
                                 size_t clip_base, float prob, ss_reverb_plan_row *d_plan, void *stream)
{
    return ss::plan_device(ss::Call{nullptr, n_clips, d_sample_offsets, total_samples, 4}, bank, d_rng, clip_base, prob, d_plan, stream);
}

int ss_reverb_apply_packed_device(const float *d_x, size_t n_clips, const int64_t *d_sample_offsets, size_t total_samples, const ss_reverb_bank *bank,
                                  const ss_reverb_plan_row *d_plan, float *d_out, void *stream)
{
    return ss::run_device<float>(SS_REVERB_DCALL(4), bank, 1.0f, nullptr, false, 0, 0.0f, d_out, const_cast<ss_reverb_plan_row *>(d_plan), stream);
}

int ss_reverb_apply_packed_i16_device(const int16_t *d_x, float x_scale, size_t n_clips, const int64_t *d_sample_offsets, size_t total_samples,
                                      const ss_reverb_bank *bank, const ss_reverb_plan_row *d_plan, float *d_out, void *stream)
{
    return ss::run_device<int16_t>(SS_REVERB_DCALL(2), bank, x_scale, nullptr, false, 0, 0.0f, d_out, const_cast<ss_reverb_plan_row *>(d_plan), stream);
}

int ss_reverb_packed_device(const float *d_x, size_t n_clips, const int64_t *d_sample_offsets, size_t total_samples, const ss_reverb_bank *bank, uint64_t *d_rng,
                            size_t clip_base, float prob, float *d_out, ss_reverb_plan_row *d_plan, void *stream)
{
    return ss::run_device<float>(SS_REVERB_DCALL(4), bank, 1.0f, d_rng, true, clip_base, prob, d_out, d_plan, stream);
}

int ss_reverb_packed_i16_device(const int16_t *d_x, float x_scale, size_t n_clips, const int64_t *d_sample_offsets, size_t total_samples,
                                const ss_reverb_bank *bank, uint64_t *d_rng, size_t clip_base, float prob, float *d_out, ss_reverb_plan_row *d_plan, void *stream)
{
    return ss::run_device<int16_t>(SS_REVERB_DCALL(2), bank, x_scale, d_rng, true, clip_base, prob, d_out, d_plan, stream);
}

int ss_reverb_apply_packed(const float *x, size_t n_clips, const int64_t *sample_offsets, size_t total_samples, const ss_reverb_bank *bank,
                           const ss_reverb_plan_row *plan, float *out)
{
    return ss::host_call<float>("ss_reverb_apply_packed", SS_REVERB_CALL(4), bank, 1.0f, nullptr, false, 0, 0.0f, out, const_cast<ss_reverb_plan_row *>(plan));
}

int ss_reverb_apply_packed_i16(const int16_t *x, float x_scale, size_t n_clips, const int64_t *sample_offsets, size_t total_samples, const ss_reverb_bank *bank,
                               const ss_reverb_plan_row *plan, float *out)
{
    return ss::host_call<int16_t>("ss_reverb_apply_packed_i16", SS_REVERB_CALL(2), bank, x_scale, nullptr, false, 0, 0.0f, out,
                                  const_cast<ss_reverb_plan_row *>(plan));
}

int ss_reverb_packed(const float *x, size_t n_clips, const int64_t *sample_offsets, size_t total_samples, const ss_reverb_bank *bank, uint64_t *rng,
                     size_t clip_base, float prob, float *out, ss_reverb_plan_row *plan)
{
    return ss::host_call<float>("ss_reverb_packed", SS_REVERB_CALL(4), bank, 1.0f, rng, true, clip_base, prob, out, plan);
}

int ss_reverb_packed_i16(const int16_t *x, float x_scale, size_t n_clips, const int64_t *sample_offsets, size_t total_samples, const ss_reverb_bank *bank,
                         uint64_t *rng, size_t clip_base, float prob, float *out, ss_reverb_plan_row *plan)
{
    return ss::host_call<int16_t>("ss_reverb_packed_i16", SS_REVERB_CALL(2), bank, x_scale, rng, true, clip_base, prob, out, plan);
}

}  // extern "C"
