// Additive noise at a drawn SNR and gain perturbation of packed clips, seeded on the device: ss_noise_* of
// include/speechsauce_amd.h, whose comment is the definition; the reference crate has no such stage, so this file restates nothing of
// it.  The draws are Philox4x32-10 (ss_philox.h) in integer and f64 arithmetic: a plan row's draw fields are a pure function of
// (seed, epoch, clip id) and the two offset tables, so every launch that needs them forms them again and no launch waits for a table
// of draws.
//
// Three launches per mix call.
//   ss_noise_energy_kernel<T>  workgroup (b, y) serves the 2048-sample chunks y, y + gridDim.y, .. of clip b (packed_split: sixteen
//                              one-minute clips are 1024 workgroups): 256 strided f64 partials per chunk, the fixed tree over them
//                              (two steps through LDS, six by lane shuffles inside wave 0: the same pairs), and one f64 word per
//                              chunk and operand in the caller's scratch.  The chunk of clip b, index k, has the scratch slot
//                              so[b] / 2048 + b + k: slots of clips that do not overlap are disjoint and below total / 2048 + n_clips.
//   ss_noise_fold_kernel       one wave per clip: the chunk words in ascending order (64 of them fetched at a time, added one by one),
//                              the draws, the two gains in f64, the plan row.
//   ss_noise_apply_kernel<T>   a flat walk over the packed block in 16-byte groups of `out`: lane q owns the four outputs of group q,
//                              finds their clip by offset_find / offset_seek, and takes the wide path -- one 16-byte (PCM: 8-byte) load
//                              of speech and one of noise -- where the group lies inside one clip and inside one noise period, and the
//                              per-sample path otherwise (clip boundaries, the block's ends, a wrap, noise clips shorter than four
//                              samples).  Both paths form fmaf(noise_gain, n, __fmul_rn(speech_gain, x)): the choice changes no bit.
//                              Lane 0 of workgroup 0 stores epoch + 1 in the combined call.
#include "ss_device.h"
#include "ss_hip_staging.h"
#include "ss_host_checks.h"
#include "ss_internal.h"
#include "ss_philox.h"

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <type_traits>

// the draws and the gains are sums and products in a stated order: nothing here is contracted (fmaf below is asked for by name)
#pragma clang fp contract(off)

namespace ss {

namespace {

constexpr unsigned kChunk = 2048;          // clip-relative samples of one partial sum
constexpr unsigned kLanes = 256;           // strided partials of a chunk
constexpr unsigned kSnrStream = 0x20000u;  // counter word 1 of the two draws: apart from SpecAugment's mask indices
constexpr unsigned kGainStream = 0x20001u;
constexpr unsigned kApplyGroups = 4;       // 16-byte groups per lane of the apply walk
constexpr unsigned long long kCountLimit = 1ull << 31;

struct DrawScalars {
    unsigned long long total_samples, total_noise;
    unsigned n_noise, clip_base;
    float prob, snr_lo, snr_hi, gain_lo, gain_hi;
};

struct Draw {
    int32_t noise_clip, start;  // -1, 0: not mixed; -2, 0: a bad speech segment
    float snr_db, gain_db;
    long long noise_base;  // no[noise_clip] of a mixed clip
    unsigned period;       // N_c of a mixed clip
};

__host__ __device__ inline bool good_segment(long long lo, long long hi, unsigned long long total)
{
    return lo >= 0 && lo <= hi && static_cast<unsigned long long>(hi) <= total && hi - lo < static_cast<long long>(kCountLimit);
}

// lo + (hi - lo) * (u * 2^-32) in f64, rounded once to f32
__host__ __device__ inline float draw_db(float lo, float hi, uint32_t u)
{
    const double t = static_cast<double>(u) * (1.0 / 4294967296.0);
    const double span = static_cast<double>(hi) - static_cast<double>(lo);
    const double scaled = span * t;
    return static_cast<float>(static_cast<double>(lo) + scaled);
}

// the draw fields of clip b with the speech segment lo .. hi: the one definition ss_noise_draws and the launches share
__host__ __device__ inline Draw draw_row(uint64_t seed, uint64_t epoch, const DrawScalars &d, unsigned b, long long lo, long long hi, const long long *no)
{
    const uint32_t id = d.clip_base + b, e0 = static_cast<uint32_t>(epoch), e1 = static_cast<uint32_t>(epoch >> 32);
    const uint32_t k0 = static_cast<uint32_t>(seed), k1 = static_cast<uint32_t>(seed >> 32);
    const Philox4 u = philox4x32_10(id, kSnrStream, e0, e1, k0, k1), v = philox4x32_10(id, kGainStream, e0, e1, k0, k1);
    Draw r{-1, 0, draw_db(d.snr_lo, d.snr_hi, u.w[3]), draw_db(d.gain_lo, d.gain_hi, v.w[0]), 0, 0};
    if (!good_segment(lo, hi, d.total_samples)) {
        r.noise_clip = -2;
        return r;
    }
    const uint64_t bar = static_cast<uint64_t>(static_cast<double>(d.prob) * 4294967296.0);
    if (d.n_noise == 0 || !(static_cast<uint64_t>(u.w[0]) < bar)) return r;
    const uint32_t c = static_cast<uint32_t>((static_cast<uint64_t>(u.w[1]) * d.n_noise) >> 32);
    const long long nlo = no[c], nhi = no[c + 1];
    if (!(good_segment(nlo, nhi, d.total_noise) && nlo < nhi)) return r;  // empty, reversed or outside the bank
    r.period = static_cast<unsigned>(nhi - nlo);
    r.noise_base = nlo;
    r.noise_clip = static_cast<int32_t>(c);
    r.start = static_cast<int32_t>((static_cast<uint64_t>(u.w[2]) * r.period) >> 32);
    return r;
}

// sample i of a float block, or of a 16-bit PCM block with its power-of-two scale (the product is exact)
template <typename T>
__device__ __forceinline__ float sample(const T *p, size_t i, float scale)
{
    if constexpr (std::is_same<T, float>::value) return p[i];
    else return __fmul_rn(static_cast<float>(p[i]), scale);
}

__device__ __forceinline__ double square(float v) { return static_cast<double>(v) * static_cast<double>(v); }  // exact in f64

// first scratch slot of a clip that starts at sample lo (>= 0)
__device__ __forceinline__ size_t first_slot(long long lo, unsigned b) { return static_cast<size_t>(lo) / kChunk + b; }

template <typename T>
__global__ __launch_bounds__(kLanes) void ss_noise_energy_kernel(const T *__restrict__ x, const long long *__restrict__ so, const T *__restrict__ nz,
                                                                const long long *__restrict__ no, const unsigned long long *__restrict__ rng,
                                                                DrawScalars d, double *__restrict__ work, size_t slots, float x_scale, float n_scale)
{
    __shared__ double s_p[2][kLanes];
    const unsigned b = blockIdx.x, t = threadIdx.x;
    const long long lo = so[b], hi = so[b + 1];
    if (!good_segment(lo, hi, d.total_samples)) return;  // uniform per workgroup
    const unsigned L = static_cast<unsigned>(hi - lo), chunks = (L + kChunk - 1) / kChunk;
    if (blockIdx.y >= chunks) return;
    const Draw dr = draw_row(rng[0], rng[1], d, b, lo, hi, no);  // uniform: every lane forms the same row
    const bool mixed = dr.noise_clip >= 0;
    const unsigned N = mixed ? dr.period : 1u, step = kLanes % N;
    const size_t slot0 = first_slot(lo, b);
    for (unsigned k = blockIdx.y; k < chunks; k += gridDim.y) {
        const unsigned i0 = k * kChunk + t;  // < 2^31 + 2048
        // (start + i) mod N moves on by 256 mod N per step: start < N < 2^31 and i0 < 2^32 - 2^31
        unsigned pos = mixed ? static_cast<unsigned>((static_cast<unsigned long long>(dr.start) + i0) % N) : 0u;
        double ps = 0.0, pn = 0.0;
#pragma unroll
        for (unsigned j = 0; j < kChunk / kLanes; ++j) {
            const unsigned i = i0 + j * kLanes;
            if (i < L) {
                ps += square(sample(x, static_cast<size_t>(lo) + i, x_scale));
                if (mixed) pn += square(sample(nz, static_cast<size_t>(dr.noise_base) + pos, n_scale));
            }
            pos += step;
            if (pos >= N) pos -= N;
        }
        // p[l] += p[l + h] for h = 128 .. 1: across the waves through LDS, inside wave 0 by shuffles
        s_p[0][t] = ps;
        s_p[1][t] = pn;
        __syncthreads();
        if (t < 128) {
            ps += s_p[0][t + 128];
            pn += s_p[1][t + 128];
            s_p[0][t] = ps;
            s_p[1][t] = pn;
        }
        __syncthreads();
        if (t < 64) {
            ps += s_p[0][t + 64];
            pn += s_p[1][t + 64];
#pragma unroll
            for (unsigned h = 32; h >= 1; h >>= 1) {
                ps += __shfl_down(ps, h, 64);
                pn += __shfl_down(pn, h, 64);
            }
            if (t == 0 && slot0 + k < slots) {
                work[slot0 + k] = ps;
                work[slots + slot0 + k] = pn;
            }
        }
        __syncthreads();  // the next chunk writes s_p again
    }
}

__global__ __launch_bounds__(64) void ss_noise_fold_kernel(const long long *__restrict__ so, const long long *__restrict__ no,
                                                          const unsigned long long *__restrict__ rng, DrawScalars d, const double *__restrict__ work,
                                                          size_t slots, ss_noise_plan_row *__restrict__ plan)
{
    const unsigned b = blockIdx.x, t = threadIdx.x;
    const long long lo = so[b], hi = so[b + 1];
    const Draw dr = draw_row(rng[0], rng[1], d, b, lo, hi, no);
    ss_noise_plan_row row{dr.noise_clip, dr.start, dr.snr_db, dr.gain_db, 0.0f, 0.0f, 0.0, 0.0};
    if (dr.noise_clip != -2) {
        const unsigned L = static_cast<unsigned>(hi - lo), chunks = (L + kChunk - 1) / kChunk;
        const size_t slot0 = first_slot(lo, b);
        double es = 0.0, en = 0.0;
        for (unsigned base = 0; base < chunks; base += 64) {
            const unsigned have = chunks - base < 64 ? chunks - base : 64;
            const bool mine = t < have && slot0 + base + t < slots;
            const double vs = mine ? work[slot0 + base + t] : 0.0, vn = mine ? work[slots + slot0 + base + t] : 0.0;
            for (unsigned j = 0; j < have; ++j) {  // ascending, one addition per chunk
                es += __shfl(vs, j, 64);
                en += __shfl(vn, j, 64);
            }
        }
        const bool mixed = dr.noise_clip >= 0;
        const double g = dr.gain_db == 0.0f ? 1.0 : pow(10.0, static_cast<double>(dr.gain_db) / 20.0);
        row.speech_energy = es;
        row.noise_energy = mixed ? en : 0.0;
        row.speech_gain = static_cast<float>(g);
        if (mixed && es > 0.0 && en > 0.0) {
            const double ratio = sqrt(es / en), att = pow(10.0, -static_cast<double>(dr.snr_db) / 20.0);
            const double gr = g * ratio;
            row.noise_gain = static_cast<float>(gr * att);
        }
    }
    if (t == 0) plan[b] = row;
}

// what the apply walk knows of a clip: its segment, its two gains and its noise operand, each checked against its own table
struct ClipMix {
    long long lo, hi, noise_base;
    float speech_gain, noise_gain;
    unsigned period, start;
    bool live, mixed;
};

struct ApplyArgs {
    const long long *so, *no;
    const ss_noise_plan_row *plan;
    unsigned long long total_samples, total_noise;
    unsigned n_clips, n_noise;
    float x_scale, n_scale;
};

__device__ __forceinline__ ClipMix load_clip(const ApplyArgs &a, unsigned c)
{
    ClipMix m{a.so[c], a.so[c + 1], 0, 0.0f, 0.0f, 1u, 0u, false, false};
    const int32_t nc = a.plan[c].noise_clip, start = a.plan[c].start;
    m.live = good_segment(m.lo, m.hi, a.total_samples) && nc != -2;
    m.speech_gain = a.plan[c].speech_gain;
    m.noise_gain = a.plan[c].noise_gain;
    if (m.live && m.noise_gain != 0.0f && nc >= 0 && static_cast<unsigned>(nc) < a.n_noise) {
        const long long nlo = a.no[nc], nhi = a.no[nc + 1];
        if (good_segment(nlo, nhi, a.total_noise) && start >= 0 && static_cast<long long>(start) < nhi - nlo) {
            m.noise_base = nlo;
            m.period = static_cast<unsigned>(nhi - nlo);
            m.start = static_cast<unsigned>(start);
            m.mixed = true;
        }
    }
    return m;
}

template <typename T>
__global__ __launch_bounds__(256) void ss_noise_apply_kernel(const T *x, const T *__restrict__ nz, ApplyArgs a, float *out, unsigned long long *rng)
{
    if (rng && blockIdx.x == 0 && threadIdx.x == 0) {  // the combined call: epoch + 1, both dwords in one vector store
        const unsigned long long e = rng[1] + 1;
        *reinterpret_cast<uint2 *>(rng + 1) = make_uint2(static_cast<unsigned>(e), static_cast<unsigned>(e >> 32));
    }
    // group q holds samples 4q - lead .. 4q - lead + 3: out + 4q - lead is 16-byte aligned
    const unsigned lead = static_cast<unsigned>(reinterpret_cast<uintptr_t>(out) >> 2) & 3u;
    const long long total = static_cast<long long>(a.total_samples);
    const unsigned long long groups = (a.total_samples + lead + 3) / 4;
    unsigned c = 0;
    bool found = false;
    ClipMix m{};
    for (unsigned u = 0; u < kApplyGroups; ++u) {
        const unsigned long long q = (static_cast<unsigned long long>(blockIdx.x) * kApplyGroups + u) * 256u + threadIdx.x;
        if (q >= groups) break;
        const long long g0 = static_cast<long long>(q * 4) - lead;
        const long long first = g0 < 0 ? 0 : g0, last = g0 + 4 < total ? g0 + 4 : total;
        const unsigned at = found ? offset_seek(a.so, a.n_clips, c, first) : offset_find(a.so, a.n_clips, first);
        if (!found || at != c) m = load_clip(a, at);
        c = at;
        found = true;
        if (g0 >= 0 && g0 + 4 <= total && m.live && g0 >= m.lo && g0 + 4 <= m.hi) {  // the group lies inside one clip
            T xv[4];
            __builtin_memcpy(xv, __builtin_assume_aligned(x + g0, sizeof(T)), sizeof xv);
            float s[4];
#pragma unroll
            for (unsigned j = 0; j < 4; ++j) s[j] = __fmul_rn(m.speech_gain, sample(xv, j, a.x_scale));
            if (m.mixed) {
                const unsigned pos = static_cast<unsigned>((static_cast<unsigned long long>(m.start) + static_cast<unsigned long long>(g0 - m.lo)) % m.period);
                if (pos + 4u <= m.period) {  // ... and inside one noise period
                    T nv[4];
                    __builtin_memcpy(nv, __builtin_assume_aligned(nz + m.noise_base + pos, sizeof(T)), sizeof nv);
#pragma unroll
                    for (unsigned j = 0; j < 4; ++j) s[j] = fmaf(m.noise_gain, sample(nv, j, a.n_scale), s[j]);
                } else {
#pragma unroll
                    for (unsigned j = 0; j < 4; ++j)
                        s[j] = fmaf(m.noise_gain, sample(nz, static_cast<size_t>(m.noise_base) + (pos + j) % m.period, a.n_scale), s[j]);
                }
            }
            *reinterpret_cast<float4 *>(out + g0) = make_float4(s[0], s[1], s[2], s[3]);
            continue;
        }
        for (long long g = first; g < last; ++g) {  // sample by sample: each finds its own clip
            const unsigned cg = offset_seek(a.so, a.n_clips, c, g);
            if (cg != c) m = load_clip(a, cg);
            c = cg;
            if (!(m.live && g >= m.lo && g < m.hi)) continue;  // in no clip, or in a bad one: untouched
            float s = __fmul_rn(m.speech_gain, sample(x, static_cast<size_t>(g), a.x_scale));
            if (m.mixed) {
                const unsigned pos = static_cast<unsigned>((static_cast<unsigned long long>(m.start) + static_cast<unsigned long long>(g - m.lo)) % m.period);
                s = fmaf(m.noise_gain, sample(nz, static_cast<size_t>(m.noise_base) + pos, a.n_scale), s);
            }
            out[g] = s;
        }
    }
}

// ---- host side ----

struct Call {  // the arguments every form shares
    const void *x;
    size_t n_clips;
    const int64_t *so;
    size_t total_samples;
    const void *nz;
    size_t n_noise;
    const int64_t *no;
    size_t total_noise;
    size_t elem;  // bytes per sample of x and nz: 4 or 2
};

int check_counts(const Call &c)
{
    if (c.n_clips >= kCountLimit || c.total_samples >= kCountLimit || c.n_noise >= kCountLimit || c.total_noise >= kCountLimit)
        return fail(SS_ERR_ARG, "n_clips, total_samples, n_noise and total_noise must be below 2^31");
    return SS_OK;
}

int check_draw_scalars(size_t clip_base, size_t n_clips, float prob, float snr_lo, float snr_hi, float gain_lo, float gain_hi)
{
    if (!(prob >= 0.0f && prob <= 1.0f)) return fail(SS_ERR_ARG, "prob must lie in [0, 1]");
    if (!(std::isfinite(snr_lo) && std::isfinite(snr_hi) && snr_lo <= snr_hi)) return fail(SS_ERR_ARG, "snr_lo_db <= snr_hi_db must be finite");
    if (!(std::isfinite(gain_lo) && std::isfinite(gain_hi) && gain_lo <= gain_hi)) return fail(SS_ERR_ARG, "gain_lo_db <= gain_hi_db must be finite");
    if (clip_base > (1ull << 32) || n_clips > (1ull << 32) - clip_base) return fail(SS_ERR_ARG, "clip_base + n_clips must not exceed 2^32");
    return SS_OK;
}

size_t work_slots(size_t n_clips, size_t total_samples) { return total_samples / kChunk + n_clips; }

// null buffers, alignment and the overlap rules; out, plan, rng and work are null where the form has none
int check_buffers(const Call &c, const float *out, const ss_noise_plan_row *plan, const uint64_t *rng, const void *work, size_t work_bytes, bool has_out,
                  bool has_rng, bool has_work)
{
    if (!c.x || !c.so || !plan || (has_out && !out) || (has_rng && !rng) || (has_work && !work) || (c.n_noise && (!c.nz || !c.no)))
        return fail(SS_ERR_ARG, "null buffer");
    const auto off = [](const void *p, size_t a) { return reinterpret_cast<uintptr_t>(p) % a != 0; };
    if (off(c.x, c.elem) || off(c.nz, c.elem) || off(out, 4)) return fail(SS_ERR_ARG, "samples, bank and out must be aligned to their element size");
    if (off(c.so, 8) || off(c.no, 8) || off(plan, 8) || off(rng, 8) || off(work, 8))
        return fail(SS_ERR_ARG, "offset tables, plan, rng and work must be 8-byte aligned");
    const size_t xbytes = c.total_samples * c.elem, obytes = has_out ? c.total_samples * sizeof(float) : 0, nbytes = c.total_noise * c.elem;
    const size_t pbytes = c.n_clips * sizeof(ss_noise_plan_row);
    if (has_work && work_bytes < 2 * work_slots(c.n_clips, c.total_samples) * sizeof(double))
        return fail(SS_ERR_ARG, "work_bytes is below ss_noise_mix_work_bytes");
    if (has_out && !(c.elem == 4 && out == c.x) && ranges_overlap(c.x, xbytes, out, obytes))
        return fail(SS_ERR_ARG, "out partly overlaps the samples (out == x is the in-place call of the float form)");
    const struct {
        const void *p;
        size_t bytes;
        const char *name;
    } others[] = {{c.nz, c.nz ? nbytes : 0, "bank"}, {plan, pbytes, "plan"}, {rng, has_rng ? 16u : 0u, "rng"}, {work, has_work ? work_bytes : 0, "work"}};
    for (const auto &o : others)
        if (o.bytes && (ranges_overlap(c.x, xbytes, o.p, o.bytes) || (obytes && ranges_overlap(out, obytes, o.p, o.bytes))))
            return fail(SS_ERR_ARG, std::string(o.name) + " overlaps the samples or out");
    for (size_t i = 1; i < 4; ++i)  // plan, rng and work are written: none may lie on another, or on the bank
        for (size_t j = 0; j < i; ++j)
            if (others[i].bytes && others[j].bytes && ranges_overlap(others[i].p, others[i].bytes, others[j].p, others[j].bytes))
                return fail(SS_ERR_ARG, std::string(others[i].name) + " overlaps " + others[j].name);
    return SS_OK;
}

// the bank's table of a host-pointer call, as check_clip_table checks the speech table
int check_bank_table(const Call &c)
{
    if (c.n_noise == 0) return SS_OK;
    if (c.no[0] != 0) return fail(SS_ERR_ARG, "noise_offsets[0] must be 0");
    for (size_t i = 0; i < c.n_noise; ++i)
        if (c.no[i + 1] < c.no[i]) return fail(SS_ERR_ARG, "decreasing noise offsets at noise clip " + std::to_string(i));
    if (static_cast<uint64_t>(c.no[c.n_noise]) > c.total_noise) return fail(SS_ERR_ARG, "the bank's table ends past total_noise");
    return SS_OK;
}

DrawScalars draw_scalars(const Call &c, size_t clip_base, float prob, float snr_lo, float snr_hi, float gain_lo, float gain_hi)
{
    return DrawScalars{static_cast<unsigned long long>(c.total_samples), static_cast<unsigned long long>(c.total_noise), static_cast<unsigned>(c.n_noise),
                       static_cast<unsigned>(clip_base), prob, snr_lo, snr_hi, gain_lo, gain_hi};
}

template <typename T>
int launch_plan(const Call &c, const uint64_t *d_rng, const DrawScalars &d, float x_scale, float n_scale, ss_noise_plan_row *d_plan, void *d_work,
                hipStream_t stream)
{
    const size_t slots = work_slots(c.n_clips, c.total_samples);
    const auto *rng = reinterpret_cast<const unsigned long long *>(d_rng);
    const auto *so = reinterpret_cast<const long long *>(c.so), *no = reinterpret_cast<const long long *>(c.no);
    const dim3 grid(static_cast<unsigned>(c.n_clips), packed_split(c.n_clips, (c.total_samples + kChunk - 1) / kChunk));
    hipLaunchKernelGGL(ss_noise_energy_kernel<T>, grid, dim3(kLanes), 0, stream, static_cast<const T *>(c.x), so, static_cast<const T *>(c.nz), no, rng, d,
                       static_cast<double *>(d_work), slots, x_scale, n_scale);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "ss_noise_energy_kernel");
    note_kernel(sizeof(T) == 4 ? "ss_noise_energy_kernel<f32>" : "ss_noise_energy_kernel<i16>");
    hipLaunchKernelGGL(ss_noise_fold_kernel, dim3(static_cast<unsigned>(c.n_clips)), dim3(64), 0, stream, so, no, rng, d, static_cast<const double *>(d_work),
                       slots, d_plan);
    e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "ss_noise_fold_kernel");
    note_kernel("ss_noise_fold_kernel");
    return SS_OK;
}

// d_rng != nullptr: the combined call, whose apply launch stores epoch + 1
template <typename T>
int launch_apply(const Call &c, float x_scale, float n_scale, const ss_noise_plan_row *d_plan, float *d_out, uint64_t *d_rng, hipStream_t stream)
{
    const ApplyArgs a{reinterpret_cast<const long long *>(c.so), reinterpret_cast<const long long *>(c.no), d_plan, c.total_samples, c.total_noise,
                      static_cast<unsigned>(c.n_clips), static_cast<unsigned>(c.n_noise), x_scale, n_scale};
    // at most (total + 6) / 4 groups, whatever the alignment of out: the grid is a function of total_samples
    const unsigned grid = static_cast<unsigned>(((c.total_samples + 6) / 4 + 256u * kApplyGroups - 1) / (256u * kApplyGroups));
    hipLaunchKernelGGL(ss_noise_apply_kernel<T>, dim3(grid ? grid : 1), dim3(256), 0, stream, static_cast<const T *>(c.x), static_cast<const T *>(c.nz), a, d_out,
                       reinterpret_cast<unsigned long long *>(d_rng));
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "ss_noise_apply_kernel");
    note_kernel(sizeof(T) == 4 ? "ss_noise_apply_kernel<f32>" : "ss_noise_apply_kernel<i16>");
    return SS_OK;
}

int check_scales(size_t elem, float x_scale, float n_scale)
{
    if (elem == 4) return SS_OK;
    const int rc = check_pcm_scale(x_scale);
    return rc ? rc : check_pcm_scale(n_scale);
}

template <typename T>
int plan_device(const Call &c, float x_scale, float n_scale, const uint64_t *d_rng, size_t clip_base, float prob, float snr_lo, float snr_hi, float gain_lo,
                float gain_hi, ss_noise_plan_row *d_plan, void *d_work, size_t work_bytes, void *stream)
{
    if (c.n_clips == 0) return SS_OK;
    int rc = check_counts(c);
    if (rc || (rc = check_buffers(c, nullptr, d_plan, d_rng, d_work, work_bytes, false, true, true)) || (rc = check_draw_scalars(clip_base, c.n_clips, prob, snr_lo, snr_hi, gain_lo, gain_hi)) ||
        (rc = check_scales(c.elem, x_scale, n_scale)))
        return rc;
    return launch_plan<T>(c, d_rng, draw_scalars(c, clip_base, prob, snr_lo, snr_hi, gain_lo, gain_hi), x_scale, n_scale, d_plan, d_work,
                          static_cast<hipStream_t>(stream));
}

template <typename T>
int apply_device(const Call &c, float x_scale, float n_scale, const ss_noise_plan_row *d_plan, float *d_out, void *stream)
{
    if (c.n_clips == 0) return SS_OK;
    int rc = check_counts(c);
    if (rc || (rc = check_buffers(c, d_out, d_plan, nullptr, nullptr, 0, true, false, false)) || (rc = check_scales(c.elem, x_scale, n_scale))) return rc;
    return launch_apply<T>(c, x_scale, n_scale, d_plan, d_out, nullptr, static_cast<hipStream_t>(stream));
}

template <typename T>
int mix_device(const Call &c, float x_scale, float n_scale, uint64_t *d_rng, size_t clip_base, float prob, float snr_lo, float snr_hi, float gain_lo,
               float gain_hi, float *d_out, ss_noise_plan_row *d_plan, void *d_work, size_t work_bytes, void *stream)
{
    if (c.n_clips == 0) return SS_OK;
    int rc = check_counts(c);
    if (rc || (rc = check_buffers(c, d_out, d_plan, d_rng, d_work, work_bytes, true, true, true)) || (rc = check_draw_scalars(clip_base, c.n_clips, prob, snr_lo, snr_hi, gain_lo, gain_hi)) ||
        (rc = check_scales(c.elem, x_scale, n_scale)))
        return rc;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    rc = launch_plan<T>(c, d_rng, draw_scalars(c, clip_base, prob, snr_lo, snr_hi, gain_lo, gain_hi), x_scale, n_scale, d_plan, d_work, st);
    return rc ? rc : launch_apply<T>(c, x_scale, n_scale, d_plan, d_out, d_rng, st);
}

// The host-pointer forms (synchronous).  Both tables are checked on the host before the device is touched; a checked speech table
// covers samples 0 .. so[n_clips) without a gap, so exactly those come down.  rng == nullptr: the apply form, on the caller's plan.
template <typename T>
int host_call(const char *name, const Call &c, float x_scale, float n_scale, uint64_t *rng, size_t clip_base, float prob, float snr_lo, float snr_hi,
              float gain_lo, float gain_hi, float *out, ss_noise_plan_row *plan)
{
    if (c.n_clips == 0) return SS_OK;
    int rc = check_counts(c);
    if (rc || (rc = check_buffers(c, out, plan, rng, nullptr, 0, true, rng != nullptr, false)) || (rng && (rc = check_draw_scalars(clip_base, c.n_clips, prob, snr_lo, snr_hi, gain_lo, gain_hi))) ||
        (rc = check_scales(c.elem, x_scale, n_scale)) || (rc = check_clip_table(c.so, c.n_clips, c.total_samples)) || (rc = check_bank_table(c)))
        return rc;
    if (!have_device()) return no_device();
    const size_t xbytes = c.total_samples * c.elem, obytes = c.total_samples * sizeof(float), pbytes = c.n_clips * sizeof(ss_noise_plan_row);
    const size_t wbytes = 2 * work_slots(c.n_clips, c.total_samples) * sizeof(double);
    HostStage st(name);
    Call d = c;
    d.x = st.up(static_cast<const char *>(c.x), xbytes);
    float *d_out = static_cast<const void *>(out) == c.x ? static_cast<float *>(const_cast<void *>(d.x)) : st.room<float>(obytes);
    d.so = st.up(c.so, (c.n_clips + 1) * sizeof(int64_t));
    d.nz = st.up(static_cast<const char *>(c.nz), c.n_noise ? c.total_noise * c.elem : 0);
    d.no = st.up(c.no, c.n_noise ? (c.n_noise + 1) * sizeof(int64_t) : 0);
    ss_noise_plan_row *d_plan = rng ? st.room<ss_noise_plan_row>(pbytes) : st.up(plan, pbytes);
    uint64_t *d_rng = rng ? st.up(rng, 16) : nullptr;
    void *d_work = rng ? st.room<char>(wbytes) : nullptr;
    if (st.ok())
        st.ran(rng ? mix_device<T>(d, x_scale, n_scale, d_rng, clip_base, prob, snr_lo, snr_hi, gain_lo, gain_hi, d_out, d_plan, d_work, wbytes, nullptr)
                   : apply_device<T>(d, x_scale, n_scale, d_plan, d_out, nullptr));
    st.sync();
    st.down(out, d_out, static_cast<size_t>(c.so[c.n_clips]) * sizeof(float));
    if (rng) {
        st.down(plan, d_plan, pbytes);
        st.down(rng + 1, d_rng + 1, 8);  // of the generator's two words the advanced counter alone
    }
    return st.status();
}

}  // namespace

}  // namespace ss

#define SS_NOISE_CALL(elem) \
    ss::Call { x, n_clips, sample_offsets, total_samples, bank, n_noise, noise_offsets, total_noise, elem }
#define SS_NOISE_DCALL(elem) \
    ss::Call { d_x, n_clips, d_sample_offsets, total_samples, d_bank, n_noise, d_noise_offsets, total_noise, elem }

extern "C" {

int ss_noise_mix_work_bytes(size_t n_clips, size_t total_samples, size_t *bytes)
{
    if (!bytes) return ss::fail(SS_ERR_ARG, "null buffer");
    if (n_clips >= ss::kCountLimit || total_samples >= ss::kCountLimit) return ss::fail(SS_ERR_ARG, "n_clips and total_samples must be below 2^31");
    *bytes = 2 * ss::work_slots(n_clips, total_samples) * sizeof(double);
    return SS_OK;
}

// host only, no device: the draw fields the plan launch writes, from the same draw_row
int ss_noise_draws(const uint64_t *rng, size_t clip_base, size_t n_clips, const int64_t *sample_offsets, size_t total_samples, size_t n_noise,
                   const int64_t *noise_offsets, size_t total_noise, float prob, float snr_lo_db, float snr_hi_db, float gain_lo_db, float gain_hi_db,
                   ss_noise_plan_row *plan)
{
    if (n_clips == 0) return SS_OK;
    if (!rng || !sample_offsets || !plan || (n_noise && !noise_offsets)) return ss::fail(SS_ERR_ARG, "null buffer");
    const ss::Call c{nullptr, n_clips, sample_offsets, total_samples, nullptr, n_noise, noise_offsets, total_noise, 4};
    int rc = ss::check_counts(c);
    if (rc || (rc = ss::check_draw_scalars(clip_base, n_clips, prob, snr_lo_db, snr_hi_db, gain_lo_db, gain_hi_db))) return rc;
    const ss::DrawScalars d = ss::draw_scalars(c, clip_base, prob, snr_lo_db, snr_hi_db, gain_lo_db, gain_hi_db);
    for (size_t b = 0; b < n_clips; ++b) {
        const ss::Draw r = ss::draw_row(rng[0], rng[1], d, static_cast<unsigned>(b), sample_offsets[b], sample_offsets[b + 1],
                                        reinterpret_cast<const long long *>(noise_offsets));
        plan[b] = ss_noise_plan_row{r.noise_clip, r.start, r.snr_db, r.gain_db, 0.0f, 0.0f, 0.0, 0.0};
    }
    return SS_OK;
}

int ss_noise_plan_packed_device(const float *d_x, size_t n_clips, const int64_t *d_sample_offsets, size_t total_samples, const float *d_bank, size_t n_noise,
                                const int64_t *d_noise_offsets, size_t total_noise, const uint64_t *d_rng, size_t clip_base, float prob, float snr_lo_db,
                                float snr_hi_db, float gain_lo_db, float gain_hi_db, ss_noise_plan_row *d_plan, void *d_work, size_t work_bytes, void *stream)
{
    return ss::plan_device<float>(SS_NOISE_DCALL(4), 1.0f, 1.0f, d_rng, clip_base, prob, snr_lo_db, snr_hi_db, gain_lo_db, gain_hi_db, d_plan, d_work,
                                  work_bytes, stream);
}

int ss_noise_plan_packed_i16_device(const int16_t *d_x, float x_scale, size_t n_clips, const int64_t *d_sample_offsets, size_t total_samples,
                                    const int16_t *d_bank, float noise_scale, size_t n_noise, const int64_t *d_noise_offsets, size_t total_noise,
                                    const uint64_t *d_rng, size_t clip_base, float prob, float snr_lo_db, float snr_hi_db, float gain_lo_db, float gain_hi_db,
                                    ss_noise_plan_row *d_plan, void *d_work, size_t work_bytes, void *stream)
{
    return ss::plan_device<int16_t>(SS_NOISE_DCALL(2), x_scale, noise_scale, d_rng, clip_base, prob, snr_lo_db, snr_hi_db, gain_lo_db, gain_hi_db, d_plan,
                                    d_work, work_bytes, stream);
}

int ss_noise_apply_packed_device(const float *d_x, size_t n_clips, const int64_t *d_sample_offsets, size_t total_samples, const float *d_bank, size_t n_noise,
                                 const int64_t *d_noise_offsets, size_t total_noise, const ss_noise_plan_row *d_plan, float *d_out, void *stream)
{
    return ss::apply_device<float>(SS_NOISE_DCALL(4), 1.0f, 1.0f, d_plan, d_out, stream);
}

int ss_noise_apply_packed_i16_device(const int16_t *d_x, float x_scale, size_t n_clips, const int64_t *d_sample_offsets, size_t total_samples,
                                     const int16_t *d_bank, float noise_scale, size_t n_noise, const int64_t *d_noise_offsets, size_t total_noise,
                                     const ss_noise_plan_row *d_plan, float *d_out, void *stream)
{
    return ss::apply_device<int16_t>(SS_NOISE_DCALL(2), x_scale, noise_scale, d_plan, d_out, stream);
}

int ss_noise_mix_packed_device(const float *d_x, size_t n_clips, const int64_t *d_sample_offsets, size_t total_samples, const float *d_bank, size_t n_noise,
                               const int64_t *d_noise_offsets, size_t total_noise, uint64_t *d_rng, size_t clip_base, float prob, float snr_lo_db,
                               float snr_hi_db, float gain_lo_db, float gain_hi_db, float *d_out, ss_noise_plan_row *d_plan, void *d_work, size_t work_bytes,
                               void *stream)
{
    return ss::mix_device<float>(SS_NOISE_DCALL(4), 1.0f, 1.0f, d_rng, clip_base, prob, snr_lo_db, snr_hi_db, gain_lo_db, gain_hi_db, d_out, d_plan, d_work,
                                 work_bytes, stream);
}

int ss_noise_mix_packed_i16_device(const int16_t *d_x, float x_scale, size_t n_clips, const int64_t *d_sample_offsets, size_t total_samples,
                                   const int16_t *d_bank, float noise_scale, size_t n_noise, const int64_t *d_noise_offsets, size_t total_noise,
                                   uint64_t *d_rng, size_t clip_base, float prob, float snr_lo_db, float snr_hi_db, float gain_lo_db, float gain_hi_db,
                                   float *d_out, ss_noise_plan_row *d_plan, void *d_work, size_t work_bytes, void *stream)
{
    return ss::mix_device<int16_t>(SS_NOISE_DCALL(2), x_scale, noise_scale, d_rng, clip_base, prob, snr_lo_db, snr_hi_db, gain_lo_db, gain_hi_db, d_out,
                                   d_plan, d_work, work_bytes, stream);
}

int ss_noise_apply_packed(const float *x, size_t n_clips, const int64_t *sample_offsets, size_t total_samples, const float *bank, size_t n_noise,
                          const int64_t *noise_offsets, size_t total_noise, const ss_noise_plan_row *plan, float *out)
{
    return ss::host_call<float>("ss_noise_apply_packed", SS_NOISE_CALL(4), 1.0f, 1.0f, nullptr, 0, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, out,
                                const_cast<ss_noise_plan_row *>(plan));
}

int ss_noise_apply_packed_i16(const int16_t *x, float x_scale, size_t n_clips, const int64_t *sample_offsets, size_t total_samples, const int16_t *bank,
                              float noise_scale, size_t n_noise, const int64_t *noise_offsets, size_t total_noise, const ss_noise_plan_row *plan, float *out)
{
    return ss::host_call<int16_t>("ss_noise_apply_packed_i16", SS_NOISE_CALL(2), x_scale, noise_scale, nullptr, 0, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, out,
                                  const_cast<ss_noise_plan_row *>(plan));
}

int ss_noise_mix_packed(const float *x, size_t n_clips, const int64_t *sample_offsets, size_t total_samples, const float *bank, size_t n_noise,
                        const int64_t *noise_offsets, size_t total_noise, uint64_t *rng, size_t clip_base, float prob, float snr_lo_db, float snr_hi_db,
                        float gain_lo_db, float gain_hi_db, float *out, ss_noise_plan_row *plan)
{
    if (n_clips && !rng) return ss::fail(SS_ERR_ARG, "null buffer");
    return ss::host_call<float>("ss_noise_mix_packed", SS_NOISE_CALL(4), 1.0f, 1.0f, rng, clip_base, prob, snr_lo_db, snr_hi_db, gain_lo_db, gain_hi_db, out,
                                plan);
}

int ss_noise_mix_packed_i16(const int16_t *x, float x_scale, size_t n_clips, const int64_t *sample_offsets, size_t total_samples, const int16_t *bank,
                            float noise_scale, size_t n_noise, const int64_t *noise_offsets, size_t total_noise, uint64_t *rng, size_t clip_base, float prob,
                            float snr_lo_db, float snr_hi_db, float gain_lo_db, float gain_hi_db, float *out, ss_noise_plan_row *plan)
{
    if (n_clips && !rng) return ss::fail(SS_ERR_ARG, "null buffer");
    return ss::host_call<int16_t>("ss_noise_mix_packed_i16", SS_NOISE_CALL(2), x_scale, noise_scale, rng, clip_base, prob, snr_lo_db, snr_hi_db, gain_lo_db,
                                  gain_hi_db, out, plan);
}

}  // extern "C"
