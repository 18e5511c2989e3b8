// C ABI entry points that touch the device (include/speechsauce_amd.h).  Host-pointer variants
// stage through device buffers; device-pointer variants only enqueue kernels on the caller's
// stream.  There is no CPU compute path here: without a HIP device these return SS_ERR_HIP.
#include <hip/hip_runtime.h>

#include <dlfcn.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <unordered_set>
#include <vector>

#include "ss_device.h"
#include "ss_hip_staging.h"
#include "ss_host_checks.h"
#include "ss_internal.h"
#include "ss_launch_args.h"

struct ss_config {
    ss::HostTables host;
    int device = -1;
    int num_cus = 256;
    // device tables
    float *d_window_mfcc = nullptr;
    float *d_window_stft = nullptr;
    float2 *d_tw_c = nullptr;
    float2 *d_tw_n = nullptr;
    float2 *d_blu_c = nullptr;  // chirp-z tables (fft_points not a power of two)
    float2 *d_blu_b = nullptr;
    int32_t *d_f_start = nullptr, *d_f_len = nullptr, *d_f_off = nullptr;
    float *d_f_w = nullptr;
    float *d_dct = nullptr;
    // fft_points = 512 MFCC kernel tables (ss_mfcc512.hip)
    ss::Fast512Tables fast;
    float *d_fast_tab = nullptr;
    // fft_points = 2048 mel-spectrogram kernel tables (ss_mel2048.hip)
    ss::Mel2048Tables mel2048;
    float *d_mel2048_tab = nullptr;
    // fft_points = 4096 MFCC kernel tables (ss_mfcc4096.hip)
    ss::Mfcc4096Tables mfcc4096;
    float *d_mfcc4096_tab = nullptr;
    // fft_points = 2048 MFCC kernel tables (ss_mfcc2048.hip)
    ss::Mfcc2048Tables mfcc2048;
    float *d_mfcc2048_tab = nullptr;
    // fft_points = 1024 MFCC kernel tables (ss_mfcc1024.hip)
    ss::Mfcc1024Tables mfcc1024;
    float *d_mfcc1024_tab = nullptr;
    // fft_points = 256 MFCC kernel tables (ss_mfcc256.hip)
    ss::Mfcc256Tables mfcc256;
    float *d_mfcc256_tab = nullptr;
    // wide-bank fft_points = 512 MFCC kernel tables (ss_mfcc512w.hip)
    ss::Mfcc512wTables mfcc512w;
    float *d_mfcc512w_tab = nullptr;
    // fft_points = 512 mel-spectrogram kernel tables (ss_mel512.hip)
    ss::Mel512Tables mel512;
    float *d_mel512_tab = nullptr;
    // fft_points = 1024 mel-spectrogram kernel tables (ss_mel_c512 in ss_mfcc1024.hip)
    ss::Mfcc1024Tables mel1024;
    float *d_mel1024_tab = nullptr;
    // fft_points = 4096 mel-spectrogram kernel tables (ss_mel_c2048 in ss_mfcc4096.hip)
    ss::Mfcc4096Tables mel4096;
    float *d_mel4096_tab = nullptr;
    // Host-pointer entry points (ss_mfcc_batch, ...): two private streams and two sets of device buffers, kept with the
    // config so that a call costs no hipMalloc / hipFree and never touches the null stream.  One host call at a time per
    // config (the mutex); calls on different configs, and device-pointer calls, run concurrently.
    struct HostPipe {
        std::mutex mu;
        hipStream_t stream[2] = {nullptr, nullptr};
        hipEvent_t done[2] = {nullptr, nullptr};
        void *d_in[2] = {nullptr, nullptr}, *d_out0[2] = {nullptr, nullptr}, *d_out1[2] = {nullptr, nullptr};
        size_t cap_in = 0, cap_out0 = 0, cap_out1 = 0;
        // small calls (one utterance): pinned, device-mapped staging the kernel reads and writes over PCIe itself -- no
        // copy commands on the stream.  [0] input, [1] / [2] outputs; host address and the device's view of it
        void *h_small[3] = {nullptr, nullptr, nullptr}, *d_small[3] = {nullptr, nullptr, nullptr};
        size_t cap_small[3] = {0, 0, 0};
    };
    mutable HostPipe pipe;
    // Device error word: one pinned, device-mapped word a kernel sets when it detects a condition that must not pass for a
    // result (today: a tile hand-off of ss_mel_c1024<tile> that never came).  The host reads it without a copy; a non-zero
    // word turns into SS_ERR_DEVICE at the next launch or synchronisation point on this config (pending_device_error).
    unsigned *h_err = nullptr, *d_err = nullptr;
    mutable unsigned tile_spin_limit = 1u << 24;  // what the word behind the 2048-point mel table block holds (test aid toggles it)
    mutable unsigned tile_spin_stage[4] = {0, 0, 0, 0};
};

#if SS_LAB
// Process-wide test aids of include/speechsauce_amd_debug.h: LAB BUILDS ONLY.  The product library's kernel selection is a pure
// function of the configuration and the call (ss_device.h has the constant forms of these accessors).
namespace {
extern std::atomic<int> g_force_generic, g_mel_tile_off;
extern std::atomic<unsigned> g_tile_fault;
}  // namespace
namespace ss {
bool dbg_force_generic() { return g_force_generic.load(std::memory_order_relaxed) != 0; }
bool dbg_mel_tile_off() { return g_mel_tile_off.load(std::memory_order_relaxed) == 1; }
int dbg_mel_build() { return g_mel_tile_off.load(std::memory_order_relaxed); }
// a forced fault: no polling at all -- the first hand-off that is not there at once counts as lost
unsigned dbg_tile_spin_limit() { return g_tile_fault.load(std::memory_order_relaxed) ? 0u : (1u << 24); }
}  // namespace ss
#endif

namespace {

thread_local const char *g_last_kernel = "";
// per-wave stamps of the 512-point MFCC kernel: the buffer of the CURRENT call on this thread (ss_mfcc_shader_clock sets it
// around its own launches; nothing process-wide in the product build)
thread_local unsigned long long *g_call_stamps = nullptr;
// the same for the kernels that write two words per wave (cycles lived, 100 MHz ticks lived): the twelve-wave builds of the
// 4096-point MFCC and the 2048-point mel kernel (the *_timed_region diagnostics set it around their own launches)
thread_local unsigned long long *g_call_stamps2 = nullptr;
#if SS_LAB
std::atomic<unsigned long long *> g_stamp_buffer{nullptr};  // ss_debug_stamp_buffer
// test aids of include/speechsauce_amd_debug.h (process-wide)
std::atomic<int> g_force_generic{0}, g_mel_tile_off{0};
std::atomic<unsigned> g_tile_fault{0};
#endif

using ss::DeviceBuf;
using ss::hip_fail;
using ss::check_pcm_scale;
using ss::ranges_overlap;

#define SS_HIP(call)                                  \
    do {                                              \
        hipError_t e_ = (call);                       \
        if (e_ != hipSuccess) return hip_fail(e_, #call); \
    } while (0)

template <typename T>
int upload(T **dst, const void *src, size_t bytes)
{
    *dst = nullptr;
    if (bytes == 0) return SS_OK;
    SS_HIP(hipMalloc(reinterpret_cast<void **>(dst), bytes));
    SS_HIP(hipMemcpy(*dst, src, bytes, hipMemcpyHostToDevice));
    return SS_OK;
}

int check_device(const ss_config *cfg);

// SS_ERR_DEVICE if a kernel of an earlier launch on this config has set the device error word (and clears it).
int pending_device_error(const ss_config *cfg)
{
    if (!cfg->h_err || __atomic_load_n(cfg->h_err, __ATOMIC_ACQUIRE) == 0) return SS_OK;
    const unsigned w = __atomic_exchange_n(cfg->h_err, 0u, __ATOMIC_ACQ_REL);
    if (w == 0) return SS_OK;
    return ss::fail(SS_ERR_DEVICE, "a kernel launched on this config reported a device-side protocol error (error word " + std::to_string(w) +
                                       "): the results of that launch are incomplete");
}

void fill_common(const ss_config *cfg, ss::FrontArgs &a)
{
    const ss::HostTables &h = cfg->host;
    a.tw_c = cfg->d_tw_c;
    a.tw_n = cfg->d_tw_n;
    a.blu_c = cfg->d_blu_c;
    a.blu_b = cfg->d_blu_b;
    a.blu_n = h.d.bluestein ? h.params.fft_points : 0u;
    a.f_start = cfg->d_f_start;
    a.f_len = cfg->d_f_len;
    a.f_off = cfg->d_f_off;
    a.f_w = cfg->d_f_w;
    a.n_filters = h.params.num_filters;
    a.dct = cfg->d_dct;
    a.n_ceps = h.params.num_cepstral;
    a.dc_elimination = h.params.dc_elimination;
    a.spectrum_exponent = h.params.spectrum_exponent;
}

// The device-side launchers' prologue.  The tables live on the device the config was created on: a launch from another current
// device would hand this device pointers into that one's memory; and no more work goes behind a launch that reported a
// device-side error.
int device_ready(const ss_config *cfg)
{
    const int drc = check_device(cfg);
    return drc ? drc : pending_device_error(cfg);
}

// The configuration's part of an MFCC-path argument block (OUT_MFCC / OUT_MFE / OUT_POWER): frame shape, pad mode, pre-emphasis,
// window, the 1/N scale and the outputs.  The caller adds the samples, its shape, frame_mode and the DCT scales.
ss::FrontArgs mfcc_front_args(const ss_config *cfg, int out_kind, float *out0, float *out1)
{
    const ss::HostTables &h = cfg->host;
    ss::FrontArgs a{};
    fill_common(cfg, a);
    a.flen = h.d.flen;
    a.step = h.d.step;
    a.pad_reflect = h.params.pad_mode == SS_PAD_REFLECT;
    a.preemph = h.params.preemph_coef;
    a.preemph_shift = static_cast<uint32_t>(h.params.preemph_shift > 0 ? h.params.preemph_shift : 1);
    a.window = cfg->d_window_mfcc;
    a.scale = 1.0f / static_cast<float>(h.params.fft_points);  // processing.rs:180
    a.out_kind = out_kind;
    a.out0 = out0;
    a.out1 = out1;
    return a;
}
void set_dct_scales(ss::FrontArgs &a, const ss::DctScales &s)
{
    a.dct_scale_k = s.k;
    a.dct_scale_0 = s.s0;
    a.dct_scale_00 = s.s00;
}

// The configuration's part of an STFT-path argument block (OUT_MEL / OUT_STFT): hop, padding rows, the Vorbis window, wnorm and
// the output.  The caller adds the samples and its shape (a continuous stream has no padding rows and says n_pad = 0).
ss::FrontArgs stft_front_args(const ss_config *cfg, int out_kind, float *out0)
{
    const ss::HostTables &h = cfg->host;
    ss::FrontArgs a{};
    fill_common(cfg, a);
    a.hop = h.d.hop;
    a.n_pad = h.d.n_pad;
    a.window = cfg->d_window_stft;
    a.scale = h.d.wnorm;
    a.out_kind = out_kind;
    a.out0 = out0;
    return a;
}

// One rung of a launcher's candidate ladder, from what its launch function returned: launched (g_last_kernel names what ran),
// declined -- hipErrorInvalidValue BEFORE the launch: the configuration does not fit this kernel (no build for the shape, LDS
// budget), the next candidate is tried -- or failed (rc: the SS_ERR_HIP code, `what` in its message).  last: nothing stands behind
// this candidate, so whatever is not a launch is a failure.
enum class Tried { launched, declined, failed };
struct Step {
    Tried t;
    int rc;
    bool done() const { return t != Tried::declined; }
};
Step tried(hipError_t e, const char *what, const ss::LaunchInfo &info, bool last = false)
{
    if (e == hipSuccess) {
        g_last_kernel = info.kernel_name;
        return {Tried::launched, SS_OK};
    }
    if (e == hipErrorInvalidValue && !last) return {Tried::declined, SS_OK};
    return {Tried::failed, hip_fail(e, what)};
}

// The samples of a call: floats, or signed 16-bit PCM with its scale (the _i16 entry points -- the pool's chunks, the packed one-shot
// calls' clips: the same chain on the kernels' PCM builds).
struct PoolChunks {
    const float *f = nullptr;
    const int16_t *pcm = nullptr;
    float scale = 1.0f;
    bool is_pcm = false;
    PoolChunks(const float *x) : f(x) {}
    PoolChunks(const int16_t *x, float s) : pcm(x), scale(s), is_pcm(true) {}
    const void *ptr() const { return is_pcm ? static_cast<const void *>(pcm) : f; }
    size_t sample_bytes() const { return is_pcm ? sizeof(int16_t) : sizeof(float); }
};

// The float copy of an equal-length PCM batch for a kernel without a PCM build (launch_frames, launch_stft): one conversion launch
// into a stream-ordered temporary, freed in stream order when the call returns.  (Stream-ordered allocation: this path is not
// offered for stream capture.)  Made once, on the first candidate that needs it: need() is a no-op for a float call and once
// a.x is set.
struct PcmFloatCopy {
    const ss::BatchPcmArgs *pcm;
    size_t batch, n, ld;
    hipStream_t st;
    float *p = nullptr;
    ~PcmFloatCopy()
    {
        if (p) (void)hipFreeAsync(p, st);
    }
    int need(ss::FrontArgs &a)
    {
        if (!pcm || a.x) return SS_OK;
        SS_HIP(hipMallocAsync(reinterpret_cast<void **>(&p), ((batch - 1) * ld + n) * sizeof(float), st));
        const hipError_t ec = ss::launch_pcm_to_float(pcm->x, p, batch, n, ld, pcm->scale, st);
        if (ec != hipSuccess) return hip_fail(ec, "launch_pcm_to_float");
        a.x = p;
        return SS_OK;
    }
};

// The dB step of a log-mel call (ss_log_mel_spectrogram*) around its ONE mel launch (launch_stft / launch_packed_stft): `args` goes to
// the launcher, which runs the dB build of the kernel it would pick anyway where that kernel has one (ran.db_fused) and the plain
// build everywhere else.  prepare() runs behind the launcher's own checks: with a top_db floor it makes the per-clip maxima, a
// stream-ordered block of ordered-integer keys (DbArgs::max_key) set to 0x80808080 by one small launch, below the key of every finite
// float; it is freed in stream order when the call returns.  Without a floor nothing is allocated: the call is the one launch.
struct DbCall {
    float ref, amin, top_db;
};
// ss_power_to_db_packed_device's checks, before anything runs
int check_db(const DbCall &c)
{
    if (!(c.amin > 0.0f)) return ss::fail(SS_ERR_ARG, "amin must be strictly positive");
    if (c.ref != c.ref) return ss::fail(SS_ERR_ARG, "ref must not be NaN");
    return SS_OK;
}
struct DbStep {
    ss::DbArgs args{};
    float top_db = -1.0f;
    hipStream_t st = nullptr;
    ss::LaunchInfo ran{};  // what the mel launch was (kernel_name null: nothing was launched)
    ~DbStep()
    {
        if (args.max_key) (void)hipFreeAsync(args.max_key, st);
    }
    // the checks, and ref_db as ss_power_to_db_packed_device forms it
    int init(const DbCall &c)
    {
        const int rc = check_db(c);
        if (rc) return rc;
        args.amin = c.amin;
        args.ref_db = 10.0f * std::log10(std::max(c.amin, std::fabs(c.ref)));
        top_db = c.top_db;
        return SS_OK;
    }
    int prepare(size_t clips, hipStream_t stream)
    {
        st = stream;
        if (!(top_db >= 0.0f) || clips == 0) return SS_OK;
        SS_HIP(hipMallocAsync(reinterpret_cast<void **>(&args.max_key), clips * sizeof(int), st));
        // (a kernel, not hipMemsetAsync: in a captured call a memset node on this block was seen to run unordered against the kernel
        // behind it when the graph is replayed -- the maxima then start from whatever the replay before left, or are wiped under the
        // mel kernel)
        const hipError_t e = ss::launch_db_keys_init(args.max_key, clips, st);
        return e == hipSuccess ? SS_OK : hip_fail(e, "launch_db_keys_init");
    }
};
// what ss_last_kernel_name() reports where the dB step ran behind a mel kernel without a dB build: that kernel's name + "+db"
// (a handful of names, kept for the process)
const char *plus_db_name(const char *kernel)
{
    static std::mutex mu;
    static std::unordered_set<std::string> names;
    std::lock_guard<std::mutex> lock(mu);
    return names.insert(std::string(kernel) + "+db").first->c_str();
}

// SS_DEBUG_TIMES=<file> (lab build, diagnostic only): per-wave realtime stamps of ONE float MFCC launch of the 512-point kernel,
// taken on extra launches of the call's own argument block in front of the real one.
#if SS_LAB
int debug_times_launches(const ss_config *cfg, ss::Fast512Args f, hipStream_t stream)
{
    static const char *dbg_path = std::getenv("SS_DEBUG_TIMES");
    static bool dbg_done = false;
    if (!dbg_path || dbg_done || f.out_mfe) return SS_OK;
    dbg_done = true;
    ss::LaunchInfo info{};
    const size_t nwaves = static_cast<size_t>(cfg->num_cus) * 16;
    DeviceBuf db;
    int rc2 = db.alloc(nwaves * 6 * sizeof(unsigned long long));
    if (rc2) return rc2;
    DeviceBuf flush;  // larger than the Infinity Cache: the stamped launch reads its samples from HBM like a bench step
    rc2 = flush.alloc(512ull << 20);
    if (rc2) return rc2;
    // the last repetition has warm code / tables and cold samples; SS_DEBUG_TIMES_REPS=<n> stamps n launches and
    // writes <file>.<k> for each from the third on (are the same workgroups late every time?)
    const char *reps_env = std::getenv("SS_DEBUG_TIMES_REPS");
    const int reps = reps_env && std::atoi(reps_env) > 3 ? std::atoi(reps_env) : 3;
    std::vector<unsigned long long> hb(nwaves * 6);
    for (int rep = 0; rep < reps; ++rep) {
        SS_HIP(hipMemsetAsync(flush.p, rep, 512ull << 20, stream));
        SS_HIP(hipMemsetAsync(db.p, 0, nwaves * 6 * sizeof(unsigned long long), stream));
        f.dbg = db.as<unsigned long long>();
        hipError_t e2 = ss::launch_mfcc_c256(f, stream, cfg->num_cus, &info);
        if (e2 != hipSuccess) return hip_fail(e2, "launch_mfcc_c256");
        SS_HIP(hipStreamSynchronize(stream));
        if (rep < 2) continue;
        SS_HIP(hipMemcpy(hb.data(), db.p, hb.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        const std::string path = rep == reps - 1 ? std::string(dbg_path) : std::string(dbg_path) + "." + std::to_string(rep);
        if (FILE *fp = std::fopen(path.c_str(), "w")) {
            for (size_t w = 0; w < nwaves; ++w)
                if (hb[6 * w + 2])
                    std::fprintf(fp, "%zu %llu %llu %llu %llu %llu %llu %llu\n", w, hb[6 * w], hb[6 * w + 1], hb[6 * w + 2],
                                 hb[6 * w + 3] >> 32, hb[6 * w + 3] & 0xffffffffull, hb[6 * w + 4], hb[6 * w + 5]);
            std::fclose(fp);
        }
    }
    return SS_OK;
}
#else
constexpr int debug_times_launches(const ss_config *, const ss::Fast512Args &, hipStream_t) { return SS_OK; }
#endif

// launch_mfcc_c2048, in the lab build with SS_DEBUG_ROWS=<file> (diagnostic only): frame 0's P row and ln(mel) row of the launch,
// dumped to the file once it ran.
#if SS_LAB
hipError_t launch_mfcc_c2048_rows(ss::Mfcc4096Args &f, hipStream_t stream, int num_cus, ss::LaunchInfo *info)
{
    static const char *rows_path = std::getenv("SS_DEBUG_ROWS");
    constexpr size_t kDbgFloats = 131072;  // >= 1028 + 256 + 4 * 4096 (stage dumps) and >= waves x 16 x 2 (SS_PROF5 phase sums)
    if (rows_path && hipMalloc(reinterpret_cast<void **>(&f.dbg), kDbgFloats * sizeof(float)) == hipSuccess)
        (void)hipMemsetAsync(f.dbg, 0, kDbgFloats * sizeof(float), stream);
    const hipError_t e4 = ss::launch_mfcc_c2048(f, stream, num_cus, info);
    if (e4 != hipSuccess && f.dbg) (void)hipFree(f.dbg);
    if (e4 == hipSuccess && f.dbg) {
        std::vector<float> rows(kDbgFloats);
        (void)hipStreamSynchronize(stream);
        (void)hipMemcpy(rows.data(), f.dbg, rows.size() * sizeof(float), hipMemcpyDeviceToHost);
        (void)hipFree(f.dbg);
        if (FILE *fp = std::fopen(rows_path, "wb")) {
            std::fwrite(rows.data(), sizeof(float), rows.size(), fp);
            std::fclose(fp);
        }
    }
    return e4;
}
#else
inline hipError_t launch_mfcc_c2048_rows(const ss::Mfcc4096Args &f, hipStream_t stream, int num_cus, ss::LaunchInfo *info)
{
    return ss::launch_mfcc_c2048(f, stream, num_cus, info);
}
#endif

// MFCC-path launch (OUT_MFCC / OUT_MFE / OUT_POWER).
// rows_are_frames: d_x is a frames matrix [batch x n] (row stride ld) -- every row is one frame of n <= fft_points samples,
// no window, no pre-emphasis (processing::power_spectrum(frames, fft_points), processing.rs:179-181).
// `multi` (ss_mfcc_batches_device): several independent batches of the same clip shape for ONE launch; d_x / batch / out0 then
// describe the first of them.  Only the kernel builds that take a batch table serve it: for every other configuration NOTHING is
// launched and kNoMultiBuild comes back (the caller then launches batch by batch).
// `pcm` (the _i16 entry points; d_x is null then): the batch as signed 16-bit PCM.  The call runs the PCM build of the kernel the
// float call would pick where that kernel has one (the 512-point kernel's contract-framing builds without fused pre-emphasis, the
// generic kernel); every other dedicated kernel runs behind one conversion launch into a stream-ordered temporary (PcmFloatCopy)
// and reports its own name.  Either way the outputs are bit for bit those of the float call on (float)pcm * scale.
struct MultiBatches {
    int n;
    const float *const *x;
    float *const *out;
    const size_t *clips;
};
constexpr int kNoMultiBuild = -1;

int launch_frames(const ss_config *cfg, int out_kind, const float *d_x, size_t batch, size_t n, size_t ld,
                  float *out0, float *out1, hipStream_t stream, bool rows_are_frames = false, const MultiBatches *multi = nullptr,
                  const ss::BatchPcmArgs *pcm = nullptr)
{
    if (!cfg) return ss::fail(SS_ERR_ARG, "null config");
    if (pcm) {
        const int src = check_pcm_scale(pcm->scale);
        if (src) return src;
    }
    if (batch == 0) return SS_OK;  // an empty batch has no buffers (a zero-row tensor's data pointer is null)
    if (!(pcm ? static_cast<const void *>(pcm->x) : d_x) || !out0) return ss::fail(SS_ERR_ARG, "null buffer");
    if (ld < n) return ss::fail(SS_ERR_ARG, "leading dimension smaller than n_samples");
    if (n > 0x7fffffffull || batch > 0x7fffffffull) return ss::fail(SS_ERR_ARG, "clip too long / batch too large");
    int rc = device_ready(cfg);
    if (rc) return rc;
    const ss::HostTables &h = cfg->host;
    size_t T = 0;
    if (rows_are_frames) {
        if (n == 0 || n > h.params.fft_points) return ss::fail(SS_ERR_ARG, "frame length must be in [1, fft_points]");
        T = 1;
    } else {
        rc = ss::num_frames(h.params, n, T);
    }
    if (rc) return rc;
    ss::FrontArgs a = mfcc_front_args(cfg, out_kind, out0, out1);
    a.x = d_x;
    a.ld = ld;
    a.n_samples = static_cast<uint32_t>(n);
    a.batch = static_cast<uint32_t>(batch);
    a.n_frames = static_cast<uint32_t>(T);
    if (rows_are_frames) {  // every row is one frame of n samples: no window, no pre-emphasis
        a.flen = a.step = static_cast<uint32_t>(n);
        a.preemph = 0.0f;
        a.window = nullptr;
    }
    // processing.rs:110-120 as written: nothing is copied for > 2 frames, x[0..flen] into every row otherwise
    if (rows_are_frames) a.frame_mode = ss::FRAME_NORMAL;
    else if (h.params.framing == SS_FRAMING_LITERAL) a.frame_mode = T > 2 ? ss::FRAME_ZERO : ss::FRAME_FIRST;
    else if (h.params.framing == SS_FRAMING_CENTER) a.frame_mode = ss::FRAME_CENTER;  // librosa center=True (generic kernel only)
    else if (h.params.framing == SS_FRAMING_PADDED) a.frame_mode = ss::FRAME_PADDED;  // zero_padding = true (generic kernel only)
    else a.frame_mode = ss::FRAME_NORMAL;
    set_dct_scales(a, ss::dct_scales(h.params, T));
    ss::LaunchInfo info{};
    // pcm: the float copy of the batch for a kernel without a PCM build -- made once, on the first candidate that needs it
    PcmFloatCopy tmp{pcm, batch, n, ld, stream};
    // fft_points = 512 MFCC: the specialised wave-private kernel (its builds: default bank / run-time bank, window,
    // pre-emphasis, mfe and power outputs, librosa variants)
    const bool force_generic = ss::dbg_force_generic();
    // the mfe-output build of that kernel exists for the default bank shape only
    const bool mfe_shape = a.flen == 320 && a.spectrum_exponent != 2 && cfg->fast.q4[0] == 4 && cfg->fast.q4[1] == 2 &&
                           cfg->fast.q4[2] == 1 && a.n_filters <= 40;
    const bool front = a.preemph != 0.0f || a.window != nullptr;  // optional window / fused pre-emphasis: default-bank build only
    // librosa-compatible variants: centred frames and banks over the whole spectrum have MFCC builds of their own (optional
    // window, no fused pre-emphasis)
    const bool centre = a.frame_mode == ss::FRAME_CENTER;
    const bool lib_variant = centre || cfg->fast.fullp;
    const bool lib_ok = out_kind == ss::OUT_MFCC && a.preemph == 0.0f;
    // Sample pairs load as 8-byte words at dword alignment (gfx950 global loads need no more: tools/unaligned_probe.py), and an
    // odd frame length ends in a half pair that one lane loads as a single float -- so hops, leading dimensions, base offsets
    // and frame lengths of either parity reach the dedicated kernels.
    const bool fast_ok = !force_generic && cfg->fast.ok &&
                         (out_kind == ss::OUT_MFCC || (out_kind == ss::OUT_MFE && mfe_shape) || (out_kind == ss::OUT_POWER && mfe_shape && !front)) &&
                         (lib_variant ? lib_ok : (!front || mfe_shape)) && (a.frame_mode == ss::FRAME_NORMAL || centre);
    const bool fits32 = static_cast<unsigned long long>(batch) * T < 0xffffffffull;
    if (fast_ok && fits32) {
        ss::Fast512Args f = ss::fast512_args(cfg->fast, cfg->d_fast_tab, a);
        if (!multi && !pcm && (rc = debug_times_launches(cfg, f, stream))) return rc;
        f.dbg = g_call_stamps;
#if SS_LAB
        if (!f.dbg) f.dbg = g_stamp_buffer.load(std::memory_order_relaxed);
#endif
        if (multi) {
            const Step s = tried(ss::launch_mfcc_c256_multi(f, multi->n, multi->x, multi->out, multi->clips, stream, cfg->num_cus, &info),
                                 "launch_mfcc_c256_multi", info);
            return s.done() ? s.rc : kNoMultiBuild;  // (declined before the launch: this shape has no batch-table build)
        }
        if (pcm) {
            // declined: no PCM build for this shape (or no build at all) -> the float build on the copy
            const Step s = tried(ss::launch_mfcc_c256(f, *pcm, stream, cfg->num_cus, &info), "launch_mfcc_c256 (PCM)", info);
            if (s.done()) return s.rc;
            if ((rc = tmp.need(a))) return rc;
            f.x = a.x;
        }
        const Step s = tried(ss::launch_mfcc_c256(f, stream, cfg->num_cus, &info), "launch_mfcc_c256", info);
        if (s.done()) return s.rc;
    }
    // fft_points = 4096 MFCC: the twelve-wave default-shape build takes a batch table too
    if (multi) {
        if (!force_generic && cfg->mfcc4096.ok && out_kind == ss::OUT_MFCC && a.frame_mode == ss::FRAME_NORMAL) {
            ss::Mfcc4096Args f = ss::mfcc4096_args(cfg->mfcc4096, cfg->d_mfcc4096_tab, a);
            f.stamps = g_call_stamps2;
            const Step s = tried(ss::launch_mfcc_c2048_multi(f, multi->n, multi->x, multi->out, multi->clips, stream, cfg->num_cus, &info),
                                 "launch_mfcc_c2048_multi", info);
            if (s.done()) return s.rc;
        }
        return kNoMultiBuild;  // the other kernels take one batch per launch
    }
    // fft_points = 512 MFCC / mfe with more than 48 filters or 16 cepstra, and the output / window / framing combinations the
    // headline kernel has no build for (ss_mfcc512w.hip): optional frame window, centred frames, fused pre-emphasis
    if (!force_generic && cfg->mfcc512w.ok && static_cast<unsigned long long>(batch) * T + 4 < 0x7fffffffull &&
        (out_kind == ss::OUT_MFCC || out_kind == ss::OUT_MFE) && (a.frame_mode == ss::FRAME_NORMAL || centre)) {
        if ((rc = tmp.need(a))) return rc;
        const ss::Mfcc256Args f = ss::mfcc256_args(cfg->mfcc512w, cfg->d_mfcc512w_tab, a);
        const Step s = tried(ss::launch_mfcc_c256w(f, stream, cfg->num_cus, &info), "launch_mfcc_c256w", info);
        if (s.done()) return s.rc;
    }
    // fft_points = 256 MFCC / mfe: two frames per complex transform (ss_mfcc256.hip); optional frame window, fused pre-emphasis
    if (!force_generic && cfg->mfcc256.ok && static_cast<unsigned long long>(batch) * T + 8 < 0x7fffffffull &&
        (out_kind == ss::OUT_MFCC || out_kind == ss::OUT_MFE) && a.frame_mode == ss::FRAME_NORMAL && a.flen <= 256) {
        if ((rc = tmp.need(a))) return rc;
        const ss::Mfcc256Args f = ss::mfcc256_args(cfg->mfcc256, cfg->d_mfcc256_tab, a);
        const Step s = tried(ss::launch_mfcc_c256x2(f, stream, cfg->num_cus, &info), "launch_mfcc_c256x2", info);
        if (s.done()) return s.rc;
    }
    // fft_points = 2048 / 1024 MFCC / mfe: two frames per wave (ss_mfcc2048.hip, ss_mfcc1024.hip), optional frame window
    // (both have librosa-compatible builds: centred frames, banks up to fs/2)
    if (!force_generic && (cfg->mfcc2048.ok || cfg->mfcc1024.ok) && fits32 && (out_kind == ss::OUT_MFCC || out_kind == ss::OUT_MFE) &&
        (a.frame_mode == ss::FRAME_NORMAL || centre)) {
        if ((rc = tmp.need(a))) return rc;
        const bool k2048 = cfg->mfcc2048.ok;
        const ss::Mfcc2048Args f = k2048 ? ss::mfcc2048_args(cfg->mfcc2048, cfg->d_mfcc2048_tab, a) : ss::mfcc2048_args(cfg->mfcc1024, cfg->d_mfcc1024_tab, a);
        const hipError_t e = k2048 ? ss::launch_mfcc_c1024(f, stream, cfg->num_cus, &info) : ss::launch_mfcc_c512(f, stream, cfg->num_cus, &info);
        const Step s = tried(e, k2048 ? "launch_mfcc_c1024" : "launch_mfcc_c512", info);
        if (s.done()) return s.rc;
    }
    // fft_points = 4096 MFCC / mfe (up to 256 filters): the one-frame-per-wave kernel
    if (!force_generic && cfg->mfcc4096.ok && fits32 && (out_kind == ss::OUT_MFCC || out_kind == ss::OUT_MFE) && a.frame_mode == ss::FRAME_NORMAL) {
        if ((rc = tmp.need(a))) return rc;
        ss::Mfcc4096Args f = ss::mfcc4096_args(cfg->mfcc4096, cfg->d_mfcc4096_tab, a);
        f.stamps = g_call_stamps2;
        const Step s = tried(launch_mfcc_c2048_rows(f, stream, cfg->num_cus, &info), "launch_mfcc_c2048", info);
        if (s.done()) return s.rc;
    }
    // (pcm: the generic kernel's PCM build, unless a dedicated candidate above already made the float copy and then declined)
    return tried(pcm && !a.x ? ss::launch_front_generic(a, *pcm, h.d.log2c, stream, cfg->num_cus, &info)
                             : ss::launch_front_generic(a, h.d.log2c, stream, cfg->num_cus, &info),
                 "launch_front_generic", info, true)
        .rc;
}

// STFT-path launch (OUT_MEL / OUT_STFT).
// `pcm` (the _i16 entry points; d_x is null then): the channels as signed 16-bit PCM, as in launch_frames.  The call runs the PCM
// build of the kernel the float call would pick where that kernel has one (the twelve-wave 2048-point mel build, chosen by the
// float call's own rule; the generic kernel); the eight-wave 2048-point family and the 512 / 1024 / 4096-point mel kernels run
// behind one conversion launch into a stream-ordered temporary and report their own names.
// `dbs` (the ss_log_mel_spectrogram* entry points, OUT_MEL): the same candidates in the same order, each on its dB build where it has
// one -- the twelve-wave 2048-point mel build and the generic kernel; dbs->ran says what ran.
int launch_stft(const ss_config *cfg, int out_kind, const float *d_x, size_t channels, size_t n, size_t ld,
                float *out0, hipStream_t stream, const MultiBatches *multi = nullptr, const ss::BatchPcmArgs *pcm = nullptr, DbStep *dbs = nullptr)
{
    if (!cfg) return ss::fail(SS_ERR_ARG, "null config");
    if (pcm) {
        const int src = check_pcm_scale(pcm->scale);
        if (src) return src;
    }
    if (channels == 0) return SS_OK;  // nothing to do, and no buffers to check
    if (!(pcm ? static_cast<const void *>(pcm->x) : d_x) || !out0) return ss::fail(SS_ERR_ARG, "null buffer");
    if (ld < n) return ss::fail(SS_ERR_ARG, "leading dimension smaller than n_samples");
    if (n == 0 || n > 0x7fffffffull || channels > 0x7fffffffull) return ss::fail(SS_ERR_ARG, "bad clip length / channel count");
    int rc = device_ready(cfg);  // see launch_frames
    if (rc) return rc;
    const ss::HostTables &h = cfg->host;
    size_t R = 0, Rreal = 0;
    if ((rc = ss::stft_rows(h.params, n, R, Rreal))) return rc;
    ss::FrontArgs a = stft_front_args(cfg, out_kind, out0);
    a.x = d_x;
    a.ld = ld;
    a.n_samples = static_cast<uint32_t>(n);
    a.batch = static_cast<uint32_t>(channels);
    a.rows = static_cast<uint32_t>(R);
    a.real_rows = static_cast<uint32_t>(Rreal);
    ss::LaunchInfo own{};
    ss::LaunchInfo &info = dbs ? dbs->ran : own;
    if (dbs && (rc = dbs->prepare(channels, stream))) return rc;
    const ss::DbArgs *db = dbs ? &dbs->args : nullptr;
    // pcm: the float copy of the channels for a kernel without a PCM build -- made once, on the first candidate that needs it
    PcmFloatCopy tmp{pcm, channels, n, ld, stream};
    // fft_points = 2048 mel spectrogram: the wave-private kernel when its layout assumptions hold
    const bool force_generic = ss::dbg_force_generic();
    const bool want_stft = out_kind == ss::OUT_STFT;  // the stft builds do not use the bank (stft_only table blocks)
    if (!force_generic && (out_kind == ss::OUT_MEL || want_stft) && (cfg->mel2048.ok || (want_stft && cfg->mel2048.stft_only)) &&
        static_cast<unsigned long long>(a.rows + a.n_pad + 1) * a.hop < 0x7fffffffull) {
        ss::Mel2048Args m = ss::mel2048_args(ss::mel_view(cfg->mel2048, cfg->d_mel2048_tab), a);
        m.ctl = cfg->d_err;
        m.stamps = g_call_stamps2;
        {
            // the poll bound lives behind the table block in device memory; it changes only when the test aid is toggled
            const unsigned lim = ss::dbg_tile_spin_limit();
            if (lim != cfg->tile_spin_limit && cfg->d_mel2048_tab) {
                unsigned *h = static_cast<unsigned *>(static_cast<void *>(cfg->tile_spin_stage));
                SS_HIP(hipStreamSynchronize(stream));  // (debug toggle only) the staging word may still be in flight
                *h = lim;
                SS_HIP(hipMemcpyAsync(cfg->d_mel2048_tab + ss::mel2048_layout::kMelW + 32 * cfg->mel2048.wpitch, h, sizeof(unsigned),
                                      hipMemcpyHostToDevice, stream));
                cfg->tile_spin_limit = lim;
            }
        }
        if (multi) {
            // several blocks for one launch (ss_mel_spectrogram_batches_device): the twelve-wave mel build takes a batch table
            const Step s = tried(ss::launch_mel_c1024_multi(m, multi->n, multi->x, multi->out, multi->clips, stream, cfg->num_cus, &info),
                                 "launch_mel_c1024_multi", info);
            return s.done() ? s.rc : kNoMultiBuild;
        }
        if (pcm) {
            // declined: the float call would not run the twelve-wave mel build -> its build on the copy
            const Step s = tried(ss::launch_mel_c1024(m, *pcm, stream, cfg->num_cus, &info, db), "launch_mel_c1024 (PCM)", info);
            if (s.done()) return s.rc;
            if ((rc = tmp.need(a))) return rc;
            m.x = a.x;
        }
        const Step s = tried(ss::launch_mel_c1024(m, stream, cfg->num_cus, &info, db), "launch_mel_c1024", info);
        if (s.done()) return s.rc;
    }
    if (multi) return kNoMultiBuild;  // the other STFT-path kernels take one block per launch
    // fft_points = 512 mel spectrogram: four rows per wave (ss_mel512.hip), same layout assumptions
    if (!force_generic && (out_kind == ss::OUT_MEL || want_stft) && (cfg->mel512.ok || (want_stft && cfg->mel512.stft_only)) &&
        static_cast<unsigned long long>(a.rows + a.n_pad + 1) * a.hop < 0x7fffffffull) {
        if ((rc = tmp.need(a))) return rc;
        const ss::Mel512Args m = ss::mel512_args(cfg->mel512, cfg->d_mel512_tab, a);
        const Step s = tried(ss::launch_mel_c256(m, stream, cfg->num_cus, &info), "launch_mel_c256", info);
        if (s.done()) return s.rc;
    }
    // fft_points = 1024 / 4096 mel spectrogram: two rows / one row per wave (ss_mel_c512 in ss_mfcc1024.hip, ss_mel_c2048 in
    // ss_mfcc4096.hip), same layout assumptions
    const bool use1024 = cfg->mel1024.ok || (want_stft && cfg->mel1024.stft_only), use4096 = cfg->mel4096.ok || (want_stft && cfg->mel4096.stft_only);
    if (!force_generic && (out_kind == ss::OUT_MEL || want_stft) && (use1024 || use4096) &&
        static_cast<unsigned long long>(a.rows + a.n_pad + 1) * a.hop < 0x7fffffffull) {
        if ((rc = tmp.need(a))) return rc;
        const ss::Mel2048Args m = ss::mel2048_args(use1024 ? ss::mel_view(cfg->mel1024, cfg->d_mel1024_tab) : ss::mel_view(cfg->mel4096, cfg->d_mel4096_tab), a);
        const hipError_t e = use1024 ? ss::launch_mel_c512(m, stream, cfg->num_cus, &info) : ss::launch_mel_c2048(m, stream, cfg->num_cus, &info);
        const Step s = tried(e, use1024 ? "launch_mel_c512" : "launch_mel_c2048", info);
        if (s.done()) return s.rc;
    }
    // (pcm: the generic kernel's PCM build, unless a dedicated candidate above already made the float copy and then declined)
    return tried(pcm && !a.x ? ss::launch_front_generic(a, *pcm, h.d.log2c, stream, cfg->num_cus, &info, db)
                             : ss::launch_front_generic(a, h.d.log2c, stream, cfg->num_cus, &info, db),
                 "launch_front_generic", info, true)
        .rc;
}

// The loop of the two *_batches_device calls over their gathered non-empty batches: groups of up to ss::kMaxLaunchBatches go to ONE
// launch where launch(x, count, out, &group) finds a batch-table build, and batch by batch (launch(x, count, out, nullptr)) where
// it returns kNoMultiBuild.  too_large: the form's message for a count past 2^31.
template <typename Launch>
int launch_batches(size_t n_batches, const float *const *d_x, const size_t *count, float *const *d_out, const char *too_large, Launch launch)
{
    std::vector<const float *> xs;
    std::vector<float *> outs;
    std::vector<size_t> counts;
    try {  // (nothing unwinds across the boundary: a failed allocation of the three small tables is an error code)
        xs.reserve(n_batches);
        outs.reserve(n_batches);
        counts.reserve(n_batches);
    } catch (const std::exception &) {
        return ss::fail(SS_ERR_ARG, "n_batches too large for this host's memory");
    }
    for (size_t b = 0; b < n_batches; ++b) {
        if (count[b] == 0) continue;  // an empty batch has no buffers
        if (!d_x[b] || !d_out[b]) return ss::fail(SS_ERR_ARG, "null buffer in batch " + std::to_string(b));
        if (count[b] > 0x7fffffffull) return ss::fail(SS_ERR_ARG, too_large);
        xs.push_back(d_x[b]);
        outs.push_back(d_out[b]);
        counts.push_back(count[b]);
    }
    for (size_t g0 = 0; g0 < xs.size(); g0 += ss::kMaxLaunchBatches) {
        const size_t gn = std::min<size_t>(ss::kMaxLaunchBatches, xs.size() - g0);
        int rc = kNoMultiBuild;
        if (gn > 1) {
            const MultiBatches mb{static_cast<int>(gn), xs.data() + g0, outs.data() + g0, counts.data() + g0};
            rc = launch(xs[g0], counts[g0], outs[g0], &mb);
        }
        if (rc == kNoMultiBuild) {
            rc = SS_OK;
            for (size_t b = g0; b < g0 + gn && rc == SS_OK; ++b) rc = launch(xs[b], counts[b], outs[b], nullptr);
        }
        if (rc) return rc;
    }
    return SS_OK;
}

// Streaming STFT-path launch (ss_*_stream_device): the rows of one call over a carried state per stream, then the state advance --
// two kernels on `stream`, nothing else (a captured call is a linear chain of two nodes).  Candidate order as launch_stft's: the
// streaming build of the 2048-point mel kernel where mel2048.ok, else the streaming build of the generic kernel.
int launch_stft_stream(const ss_config *cfg, int out_kind, int mode, const float *d_x, size_t n_streams, size_t n, size_t ld,
                       float *d_state, float *out0, hipStream_t stream)
{
    if (!cfg) return ss::fail(SS_ERR_ARG, "null config");
    if (n_streams == 0) return SS_OK;
    if (!d_x || !d_state || !out0) return ss::fail(SS_ERR_ARG, "null buffer");
    if (ld < n) return ss::fail(SS_ERR_ARG, "leading dimension smaller than n_samples");
    if (n == 0 || n > 0x7fffffffull || n_streams > 0x7fffffffull) return ss::fail(SS_ERR_ARG, "bad chunk length / stream count");
    int rc = device_ready(cfg);  // see launch_frames
    if (rc) return rc;
    const ss::HostTables &h = cfg->host;
    size_t R = 0, Rreal = 0;
    if ((rc = ss_stream_rows(&h.params, mode, n, &R, &Rreal))) return rc;
    const size_t S = h.params.fft_points - h.d.hop;
    const size_t F = h.params.fft_points / 2 + 1;
    const size_t out_floats = n_streams * R * (out_kind == ss::OUT_STFT ? 2 * F : h.params.num_filters);
    if (ranges_overlap(d_state, n_streams * S * sizeof(float), d_x, ((n_streams - 1) * ld + n) * sizeof(float)) ||
        ranges_overlap(d_state, n_streams * S * sizeof(float), out0, out_floats * sizeof(float)))
        return ss::fail(SS_ERR_ARG, "the state buffer overlaps the input or the output");
    // reference mode: the chunk is zero-padded to whole hops (functions.rs:112-117) and the rows end at chunk i + n_pad
    const bool continuous = mode == SS_STREAM_CONTINUOUS;
    const size_t advance = continuous ? n : R * h.d.hop;
    if (advance > 0xffffffffull || R > 0x7fffffffull) return ss::fail(SS_ERR_ARG, "chunk too long");
    ss::FrontArgs a = stft_front_args(cfg, out_kind, out0);
    a.x = d_x;
    a.ld = ld;
    a.n_samples = static_cast<uint32_t>(n);
    a.batch = static_cast<uint32_t>(n_streams);
    if (continuous) a.n_pad = 0u;  // every row is real
    a.rows = static_cast<uint32_t>(R);
    a.real_rows = static_cast<uint32_t>(Rreal);
    ss::StreamArgs sa{d_state, static_cast<uint32_t>(S)};
    ss::LaunchInfo info{};
    Step s{Tried::declined, SS_OK};
    if (!ss::dbg_force_generic() && out_kind == ss::OUT_MEL && cfg->mel2048.ok &&
        static_cast<unsigned long long>(a.rows + a.n_pad + 1) * a.hop < 0x7fffffffull) {
        ss::Mel2048Args m = ss::mel2048_args(ss::mel_view(cfg->mel2048, cfg->d_mel2048_tab), a);
        m.ctl = cfg->d_err;
        // declined: the configuration does not fit this kernel -> the generic build
        s = tried(ss::launch_mel_c1024_stream(m, sa, stream, cfg->num_cus, &info), "launch_mel_c1024_stream", info);
    }
    if (!s.done()) s = tried(ss::launch_front_generic_stream(a, sa, h.d.log2c, stream, cfg->num_cus, &info), "launch_front_generic_stream", info, true);
    if (s.rc) return s.rc;
    const hipError_t e = ss::launch_stream_advance(d_state, static_cast<uint32_t>(S), d_x, ld, a.n_samples, static_cast<uint32_t>(advance), a.batch, stream);
    if (e != hipSuccess) return hip_fail(e, "launch_stream_advance");
    return SS_OK;
}

// Host-pointer form: one upload of x and the state, the device call, one download of out and the state on the config's first
// host-pipeline stream (host calls of a config are serialised by its mutex).  The caller's state is written only once everything
// before it succeeded.
int stream_host(const ss_config *cfg, int out_kind, int mode, const float *x, size_t n_streams, size_t n, size_t ld, float *state,
                float *out0)
{
    if (!cfg) return ss::fail(SS_ERR_ARG, "null config");
    if (n_streams == 0) return SS_OK;
    if (!x || !state || !out0) return ss::fail(SS_ERR_ARG, "null buffer");
    if (ld < n) return ss::fail(SS_ERR_ARG, "leading dimension smaller than n_samples");
    if (n == 0 || n > 0x7fffffffull || n_streams > 0x7fffffffull) return ss::fail(SS_ERR_ARG, "bad chunk length / stream count");
    const ss::HostTables &h = cfg->host;
    size_t R = 0, Rreal = 0;
    int rc = ss_stream_rows(&h.params, mode, n, &R, &Rreal);
    if (rc) return rc;
    const size_t S = h.params.fft_points - h.d.hop;
    const size_t out_floats = n_streams * R * (out_kind == ss::OUT_STFT ? 2 * (h.params.fft_points / 2 + 1) : h.params.num_filters);
    const size_t in_floats = (n_streams - 1) * ld + n;
    if (ranges_overlap(state, n_streams * S * sizeof(float), x, in_floats * sizeof(float)) ||
        ranges_overlap(state, n_streams * S * sizeof(float), out0, out_floats * sizeof(float)))
        return ss::fail(SS_ERR_ARG, "the state buffer overlaps the input or the output");
    if ((rc = check_device(cfg))) return rc;
    ss_config::HostPipe &hp = cfg->pipe;
    std::lock_guard<std::mutex> lock(hp.mu);
    if (!hp.stream[0]) {
        SS_HIP(hipStreamCreateWithFlags(&hp.stream[0], hipStreamNonBlocking));
        SS_HIP(hipEventCreateWithFlags(&hp.done[0], hipEventDisableTiming));
    }
    hipStream_t st = hp.stream[0];
    DeviceBuf dx, ds, d0;
    if ((rc = dx.alloc(in_floats * sizeof(float))) || (rc = ds.alloc(n_streams * S * sizeof(float))) ||
        (rc = d0.alloc(out_floats * sizeof(float))))
        return rc;
    hipError_t e = hipMemcpyAsync(dx.p, x, in_floats * sizeof(float), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(ds.p, state, n_streams * S * sizeof(float), hipMemcpyHostToDevice, st);
    if (e != hipSuccess) rc = hip_fail(e, "hipMemcpyAsync (H2D)");
    if (rc == SS_OK) rc = launch_stft_stream(cfg, out_kind, mode, dx.as<const float>(), n_streams, n, ld, ds.as<float>(), d0.as<float>(), st);
    if (rc == SS_OK) {
        e = hipMemcpyAsync(out0, d0.p, out_floats * sizeof(float), hipMemcpyDeviceToHost, st);
        if (e != hipSuccess) rc = hip_fail(e, "hipMemcpyAsync (D2H)");
    }
    // the copies may still touch the caller's buffers and ours: synchronise whatever happened
    e = hipStreamSynchronize(st);
    if (e != hipSuccess && rc == SS_OK) rc = hip_fail(e, "stream host call");
    if (rc == SS_OK) rc = pending_device_error(cfg);
    if (rc == SS_OK) {
        e = hipMemcpyAsync(state, ds.p, n_streams * S * sizeof(float), hipMemcpyDeviceToHost, st);
        const hipError_t es = hipStreamSynchronize(st);
        if (e != hipSuccess || es != hipSuccess) rc = hip_fail(e != hipSuccess ? e : es, "hipMemcpyAsync (state D2H)");
    }
    return rc;
}

// The argument block of a streaming MFCC / mfe launch without its shape (ld / n_samples / batch / n_frames: the caller's), shared by
// the dense and the ragged (pool) form: the same configuration gives the same block, so the same bits per frame.
ss::FrontArgs frame_stream_front_args(const ss_config *cfg, int out_kind, const float *d_x, uint32_t norm_frames, float *out0, float *out1)
{
    ss::FrontArgs a = mfcc_front_args(cfg, out_kind, out0, out1);
    a.x = d_x;
    a.frame_mode = ss::FRAME_NORMAL;  // every row's frame ends inside the chunk: contract and padded framing agree
    // the scales of launch_frames with T = norm_frames; a stream has no first frame, so [0,0] gets column 0's scale
    set_dct_scales(a, ss::dct_scales(cfg->host.params, norm_frames > 0 ? norm_frames : 1u));
    a.dct_scale_00 = a.dct_scale_0;
    return a;
}
// whether the streaming builds of the 512-point headline kernel are candidates for the configuration (their launchers decide)
bool frame_stream_fast_candidate(const ss_config *cfg, const ss::FrontArgs &a)
{
    return !ss::dbg_force_generic() && cfg->fast.ok && !cfg->fast.fullp && a.window == nullptr && a.preemph == 0.0f &&
           cfg->host.params.dct_norm != SS_DCT_ORTHO;
}
// The entry tables of a ragged streaming launch over a pool of stream states (either path: lead is the MFCC path's flen - step and
// unused on the STFT path, step the path's hop)
ss::FrameStreamPackedArgs stream_packed_args(const ss_config *cfg, size_t S, int32_t lead, uint32_t step, const int64_t *d_so, const int64_t *d_ro,
                                             const int32_t *d_slots, size_t n_active, size_t pool_streams, size_t total_rows, float *d_pool)
{
    ss::FrameStreamPackedArgs e{};
    e.pool = d_pool;
    e.state_len = static_cast<uint32_t>(S);
    e.lead = lead;
    e.so = reinterpret_cast<const long long *>(d_so);
    e.ro = reinterpret_cast<const long long *>(d_ro);
    e.slots = d_slots;
    e.n_active = static_cast<uint32_t>(n_active);
    e.pool_streams = static_cast<uint32_t>(pool_streams);
    e.total_rows = static_cast<uint32_t>(total_rows);
    e.step = step;
    e.err = cfg->d_err;
    return e;
}

// Streaming MFCC / mfe launch (ss_mfcc_stream_device / ss_mfe_stream_device): the rows of one call over a carried state per
// stream, then the state advance -- two kernels on `stream` (none for the advance where S == 0).  Candidate order: the streaming
// build of the 512-point headline kernel where it has one for the shape, else the streaming build of the generic kernel.
int launch_frame_stream(const ss_config *cfg, int out_kind, const float *d_x, size_t n_streams, size_t n, size_t ld, uint32_t norm_frames,
                        float *d_state, float *out0, float *out1, hipStream_t stream)
{
    if (!cfg) return ss::fail(SS_ERR_ARG, "null config");
    if (n_streams == 0) return SS_OK;
    const ss::HostTables &h = cfg->host;
    size_t S = 0, R = 0;
    int rc = ss_frame_stream_state_len(&h.params, &S);
    if (rc) return rc;
    if (!d_x || !out0 || (out_kind == ss::OUT_MFE && !out1) || (S > 0 && !d_state)) return ss::fail(SS_ERR_ARG, "null buffer");
    if (ld < n) return ss::fail(SS_ERR_ARG, "leading dimension smaller than n_samples");
    if (n == 0 || n > 0x7fffffffull || n_streams > 0x7fffffffull) return ss::fail(SS_ERR_ARG, "bad chunk length / stream count");
    const bool ortho = h.params.dct_norm == SS_DCT_ORTHO;
    if (out_kind == ss::OUT_MFCC && !ortho && norm_frames == 0)
        return ss::fail(SS_ERR_ARG, "norm_frames must be >= 1: the reference DCT scaling needs a frame count");
    if ((rc = ss_frame_stream_rows(&h.params, n, &R))) return rc;
    if (static_cast<unsigned long long>(n_streams) * R >= 0x7fffffffull) return ss::fail(SS_ERR_ARG, "too many rows in one call");
    const size_t cols = out_kind == ss::OUT_MFCC ? h.params.num_cepstral : h.params.num_filters;
    const size_t sbytes = n_streams * S * sizeof(float);
    if (S > 0 && (ranges_overlap(d_state, sbytes, d_x, ((n_streams - 1) * ld + n) * sizeof(float)) ||
                  ranges_overlap(d_state, sbytes, out0, n_streams * R * cols * sizeof(float)) ||
                  (out1 && ranges_overlap(d_state, sbytes, out1, n_streams * R * sizeof(float)))))
        return ss::fail(SS_ERR_ARG, "the state buffer overlaps the input or an output");
    if ((rc = device_ready(cfg))) return rc;  // see launch_frames
    ss::FrontArgs a = frame_stream_front_args(cfg, out_kind, d_x, norm_frames, out0, out1);
    a.ld = ld;
    a.n_samples = static_cast<uint32_t>(n);
    a.batch = static_cast<uint32_t>(n_streams);
    a.n_frames = static_cast<uint32_t>(R);
    ss::FrameStreamArgs fsa{d_state, static_cast<uint32_t>(S), static_cast<int32_t>(h.d.flen) - static_cast<int32_t>(h.d.step)};
    ss::LaunchInfo info{};
    Step s{Tried::declined, SS_OK};
    if (frame_stream_fast_candidate(cfg, a)) {
        const ss::Fast512Args f = ss::fast512_args(cfg->fast, cfg->d_fast_tab, a);
        // declined: the configuration has no streaming build of this kernel -> the generic build
        s = tried(ss::launch_mfcc_c256_stream(f, fsa, stream, cfg->num_cus, &info), "launch_mfcc_c256_stream", info);
    }
    if (!s.done())
        s = tried(ss::launch_front_generic_frame_stream(a, fsa, h.d.log2c, stream, cfg->num_cus, &info), "launch_front_generic_frame_stream", info, true);
    if (s.rc) return s.rc;
    const hipError_t e = ss::launch_stream_advance(d_state, static_cast<uint32_t>(S), d_x, ld, a.n_samples, a.n_samples, a.batch, stream);
    if (e != hipSuccess) return hip_fail(e, "launch_stream_advance");
    return SS_OK;
}

// Host-pointer form, as stream_host: one upload of x and the state, the device call, one download of the outputs and the state on
// the config's first host-pipeline stream.  The caller's state is written only once everything before it succeeded.
int frame_stream_host(const ss_config *cfg, int out_kind, const float *x, size_t n_streams, size_t n, size_t ld, uint32_t norm_frames,
                      float *state, float *out0, float *out1)
{
    if (!cfg) return ss::fail(SS_ERR_ARG, "null config");
    if (n_streams == 0) return SS_OK;
    const ss::HostTables &h = cfg->host;
    size_t S = 0, R = 0;
    int rc = ss_frame_stream_state_len(&h.params, &S);
    if (rc) return rc;
    if (!x || !out0 || (out_kind == ss::OUT_MFE && !out1) || (S > 0 && !state)) return ss::fail(SS_ERR_ARG, "null buffer");
    if (ld < n) return ss::fail(SS_ERR_ARG, "leading dimension smaller than n_samples");
    if (n == 0 || n > 0x7fffffffull || n_streams > 0x7fffffffull) return ss::fail(SS_ERR_ARG, "bad chunk length / stream count");
    if ((rc = ss_frame_stream_rows(&h.params, n, &R))) return rc;
    const size_t cols = out_kind == ss::OUT_MFCC ? h.params.num_cepstral : h.params.num_filters;
    const size_t out0_floats = n_streams * R * cols, out1_floats = out1 ? n_streams * R : 0;
    const size_t in_floats = (n_streams - 1) * ld + n;
    const size_t sbytes = n_streams * S * sizeof(float);
    if (S > 0 && (ranges_overlap(state, sbytes, x, in_floats * sizeof(float)) || ranges_overlap(state, sbytes, out0, out0_floats * sizeof(float)) ||
                  (out1 && ranges_overlap(state, sbytes, out1, out1_floats * sizeof(float)))))
        return ss::fail(SS_ERR_ARG, "the state buffer overlaps the input or an output");
    if ((rc = check_device(cfg))) return rc;
    ss_config::HostPipe &hp = cfg->pipe;
    std::lock_guard<std::mutex> lock(hp.mu);
    if (!hp.stream[0]) {
        SS_HIP(hipStreamCreateWithFlags(&hp.stream[0], hipStreamNonBlocking));
        SS_HIP(hipEventCreateWithFlags(&hp.done[0], hipEventDisableTiming));
    }
    hipStream_t st = hp.stream[0];
    DeviceBuf dx, ds, d0, d1;
    if ((rc = dx.alloc(in_floats * sizeof(float))) || (S > 0 && (rc = ds.alloc(sbytes))) || (rc = d0.alloc(out0_floats * sizeof(float))) ||
        (out1 && (rc = d1.alloc(out1_floats * sizeof(float)))))
        return rc;
    hipError_t e = hipMemcpyAsync(dx.p, x, in_floats * sizeof(float), hipMemcpyHostToDevice, st);
    if (e == hipSuccess && S > 0) e = hipMemcpyAsync(ds.p, state, sbytes, hipMemcpyHostToDevice, st);
    if (e != hipSuccess) rc = hip_fail(e, "hipMemcpyAsync (H2D)");
    if (rc == SS_OK)
        rc = launch_frame_stream(cfg, out_kind, dx.as<const float>(), n_streams, n, ld, norm_frames, S > 0 ? ds.as<float>() : nullptr,
                                 d0.as<float>(), out1 ? d1.as<float>() : nullptr, st);
    if (rc == SS_OK) {
        e = hipMemcpyAsync(out0, d0.p, out0_floats * sizeof(float), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess && out1) e = hipMemcpyAsync(out1, d1.p, out1_floats * sizeof(float), hipMemcpyDeviceToHost, st);
        if (e != hipSuccess) rc = hip_fail(e, "hipMemcpyAsync (D2H)");
    }
    // the copies may still touch the caller's buffers and ours: synchronise whatever happened
    e = hipStreamSynchronize(st);
    if (e != hipSuccess && rc == SS_OK) rc = hip_fail(e, "frame stream host call");
    if (rc == SS_OK) rc = pending_device_error(cfg);
    if (rc == SS_OK && S > 0) {
        e = hipMemcpyAsync(state, ds.p, sbytes, hipMemcpyDeviceToHost, st);
        const hipError_t es = hipStreamSynchronize(st);
        if (e != hipSuccess || es != hipSuccess) rc = hip_fail(e != hipSuccess ? e : es, "hipMemcpyAsync (state D2H)");
    }
    return rc;
}

// Ragged streaming MFCC / mfe over a pool of stream states (ss_mfcc_stream_packed_device / ss_mfe_stream_packed_device): the rows of
// n_active entries of different hop counts, each over the pool row its slot names, then the advance of the named rows -- a linear
// chain of two kernels on `stream` (none for the advance where S == 0).  The tables are device arrays read by the kernels only
// (FrameStreamPackedArgs, ss_device.h); the grids come from n_active and total_rows.  Candidate order as launch_frame_stream.
int launch_frame_stream_packed(const ss_config *cfg, int out_kind, const PoolChunks &x, size_t n_active, const int64_t *d_so, const int64_t *d_ro,
                               size_t total_rows, const int32_t *d_slots, size_t pool_streams, uint32_t norm_frames, float *d_pool,
                               float *out0, float *out1, hipStream_t stream)
{
    if (!cfg) return ss::fail(SS_ERR_ARG, "null config");
    if (n_active == 0) return SS_OK;
    const ss::HostTables &h = cfg->host;
    size_t S = 0;
    int rc = ss_frame_stream_state_len(&h.params, &S);
    if (rc) return rc;
    if (!x.ptr() || !d_so || !d_ro || !d_slots || !out0 || (out_kind == ss::OUT_MFE && !out1) || (S > 0 && !d_pool))
        return ss::fail(SS_ERR_ARG, "null buffer");
    if (x.is_pcm && (rc = check_pcm_scale(x.scale))) return rc;
    if (x.is_pcm && (reinterpret_cast<uintptr_t>(x.pcm) & 3u)) return ss::fail(SS_ERR_ARG, "the PCM buffer must be 4-byte aligned");
    if (n_active >= 0x80000000ull || pool_streams >= 0x80000000ull || total_rows >= 0x80000000ull)
        return ss::fail(SS_ERR_ARG, "n_active, pool_streams and total_rows must be below 2^31");
    if (pool_streams == 0) return ss::fail(SS_ERR_ARG, "the pool has no rows");
    if (out_kind == ss::OUT_MFCC && h.params.dct_norm != SS_DCT_ORTHO && norm_frames == 0)
        return ss::fail(SS_ERR_ARG, "norm_frames must be >= 1: the reference DCT scaling needs a frame count");
    const size_t cols = out_kind == ss::OUT_MFCC ? h.params.num_cepstral : h.params.num_filters;
    const size_t pbytes = pool_streams * S * sizeof(float);
    if (S > 0 && (ranges_overlap(d_pool, pbytes, out0, total_rows * cols * sizeof(float)) ||
                  (out1 && ranges_overlap(d_pool, pbytes, out1, total_rows * sizeof(float)))))
        return ss::fail(SS_ERR_ARG, "the pool overlaps an output");
    if ((rc = device_ready(cfg))) return rc;  // see launch_frames
    const ss::FrontArgs a = frame_stream_front_args(cfg, out_kind, x.f, norm_frames, out0, out1);
    const ss::FrameStreamPackedArgs fsp = stream_packed_args(cfg, S, static_cast<int32_t>(h.d.flen) - static_cast<int32_t>(h.d.step), h.d.step, d_so,
                                                             d_ro, d_slots, n_active, pool_streams, total_rows, d_pool);
    const ss::FrameStreamPackedPcmArgs pcm{fsp, x.pcm, x.scale};
    ss::LaunchInfo info{};
    Step s{Tried::declined, SS_OK};
    if (frame_stream_fast_candidate(cfg, a)) {
        const ss::Fast512Args f = ss::fast512_args(cfg->fast, cfg->d_fast_tab, a);
        // declined: the configuration has no ragged streaming build of this kernel -> the generic build
        s = tried(x.is_pcm ? ss::launch_mfcc_c256_stream_packed(f, pcm, stream, cfg->num_cus, &info)
                           : ss::launch_mfcc_c256_stream_packed(f, fsp, stream, cfg->num_cus, &info),
                  "launch_mfcc_c256_stream_packed", info);
    }
    if (!s.done())
        s = tried(x.is_pcm ? ss::launch_front_generic_frame_stream_packed(a, pcm, h.d.log2c, stream, cfg->num_cus, &info)
                           : ss::launch_front_generic_frame_stream_packed(a, fsp, h.d.log2c, stream, cfg->num_cus, &info),
                  "launch_front_generic_frame_stream_packed", info, true);
    if (s.rc) return s.rc;
    const hipError_t e = x.is_pcm ? ss::launch_stream_advance_packed(pcm, stream) : ss::launch_stream_advance_packed(fsp, x.f, stream);
    if (e != hipSuccess) return hip_fail(e, "launch_stream_advance_packed");
    return SS_OK;
}

// Host-pointer form: the tables are checked here, before anything touches the device; then x, the tables and the n_active named
// pool rows (gathered into a compact block whose row i is entry i's: the device call runs on slots 0 .. n_active - 1) go up, the
// outputs and the named rows come down on the config's first host-pipeline stream.  The caller's pool is written only once
// everything before it succeeded.
int frame_stream_packed_host(const ss_config *cfg, int out_kind, const PoolChunks &x, size_t n_active, const int64_t *so, const int32_t *slots,
                             size_t pool_streams, uint32_t norm_frames, float *pool, float *out0, float *out1)
{
    if (!cfg) return ss::fail(SS_ERR_ARG, "null config");
    if (n_active == 0) return SS_OK;
    const ss::HostTables &h = cfg->host;
    size_t S = 0;
    int rc = ss_frame_stream_state_len(&h.params, &S);
    if (rc) return rc;
    if (!x.ptr() || !so || !slots || !out0 || (out_kind == ss::OUT_MFE && !out1) || (S > 0 && !pool)) return ss::fail(SS_ERR_ARG, "null buffer");
    if (x.is_pcm && (rc = check_pcm_scale(x.scale))) return rc;
    if (n_active >= 0x80000000ull || pool_streams >= 0x80000000ull)
        return ss::fail(SS_ERR_ARG, "n_active, pool_streams and total_rows must be below 2^31");
    if (out_kind == ss::OUT_MFCC && h.params.dct_norm != SS_DCT_ORTHO && norm_frames == 0)
        return ss::fail(SS_ERR_ARG, "norm_frames must be >= 1: the reference DCT scaling needs a frame count");
    std::vector<int64_t> ro(n_active + 1);
    if ((rc = ss_frame_stream_packed_row_offsets(&h.params, n_active, so, ro.data()))) return rc;
    if ((rc = ss::check_slots(slots, n_active, pool_streams))) return rc;
    const size_t rows = static_cast<size_t>(ro[n_active]), samples = static_cast<size_t>(so[n_active]);
    if (rows >= 0x80000000ull) return ss::fail(SS_ERR_ARG, "n_active, pool_streams and total_rows must be below 2^31");
    const size_t cols = out_kind == ss::OUT_MFCC ? h.params.num_cepstral : h.params.num_filters;
    if ((rc = check_device(cfg))) return rc;
    ss::PoolRows named;  // the named pool rows, row i = entry i's
    named.gather(pool, slots, n_active, S);
    ss_config::HostPipe &hp = cfg->pipe;
    std::lock_guard<std::mutex> lock(hp.mu);
    if (!hp.stream[0]) {
        SS_HIP(hipStreamCreateWithFlags(&hp.stream[0], hipStreamNonBlocking));
        SS_HIP(hipEventCreateWithFlags(&hp.done[0], hipEventDisableTiming));
    }
    hipStream_t st = hp.stream[0];
    const size_t tbytes = (n_active + 1) * sizeof(int64_t), sbytes = n_active * S * sizeof(float);
    DeviceBuf dx, dso, dro, dsl, dp, d0, d1;
    if ((rc = dx.alloc(samples * x.sample_bytes())) || (rc = dso.alloc(tbytes)) || (rc = dro.alloc(tbytes)) ||
        (rc = dsl.alloc(n_active * sizeof(int32_t))) || (S > 0 && (rc = dp.alloc(sbytes))) || (rc = d0.alloc(rows * cols * sizeof(float))) ||
        (out1 && (rc = d1.alloc(rows * sizeof(float)))))
        return rc;
    hipError_t e = samples ? hipMemcpyAsync(dx.p, x.ptr(), samples * x.sample_bytes(), hipMemcpyHostToDevice, st) : hipSuccess;
    if (e == hipSuccess) e = hipMemcpyAsync(dso.p, so, tbytes, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(dro.p, ro.data(), tbytes, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(dsl.p, named.iota.data(), n_active * sizeof(int32_t), hipMemcpyHostToDevice, st);
    if (e == hipSuccess && S > 0) e = hipMemcpyAsync(dp.p, named.rows_host.data(), sbytes, hipMemcpyHostToDevice, st);
    if (e != hipSuccess) rc = hip_fail(e, "hipMemcpyAsync (H2D)");
    if (rc == SS_OK)
        rc = launch_frame_stream_packed(cfg, out_kind, x.is_pcm ? PoolChunks(dx.as<const int16_t>(), x.scale) : PoolChunks(dx.as<const float>()),
                                        n_active, dso.as<const int64_t>(), dro.as<const int64_t>(), rows,
                                        dsl.as<const int32_t>(), n_active, norm_frames, S > 0 ? dp.as<float>() : nullptr, d0.as<float>(),
                                        out1 ? d1.as<float>() : nullptr, st);
    if (rc == SS_OK && rows > 0) {
        e = hipMemcpyAsync(out0, d0.p, rows * cols * sizeof(float), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess && out1) e = hipMemcpyAsync(out1, d1.p, rows * sizeof(float), hipMemcpyDeviceToHost, st);
        if (e != hipSuccess) rc = hip_fail(e, "hipMemcpyAsync (D2H)");
    }
    // the copies may still touch the caller's buffers and ours: synchronise whatever happened
    e = hipStreamSynchronize(st);
    if (e != hipSuccess && rc == SS_OK) rc = hip_fail(e, "frame stream pool host call");
    if (rc == SS_OK) rc = pending_device_error(cfg);
    if (rc == SS_OK && S > 0) {
        e = hipMemcpyAsync(named.rows_host.data(), dp.p, sbytes, hipMemcpyDeviceToHost, st);
        const hipError_t es = hipStreamSynchronize(st);
        if (e != hipSuccess || es != hipSuccess) rc = hip_fail(e != hipSuccess ? e : es, "hipMemcpyAsync (pool rows D2H)");
        if (rc == SS_OK) named.scatter(pool, slots);
    }
    return rc;
}

// Ragged streaming STFT / mel spectrogram over a pool of stream states (ss_mel_spectrogram_stream_packed_device /
// ss_stft_stream_packed_device), continuous mode: the rows of n_active entries of different hop counts, each over the pool row its
// slot names, then the advance of the named rows -- a linear chain of two kernels on `stream`.  The tables are device arrays read by
// the kernels only (StftStreamPackedArgs, ss_device.h); the grids come from n_active and total_rows.  Candidate order as
// launch_stft_stream: the ragged streaming build of the 2048-point mel kernel where mel2048.ok, else that of the generic kernel.
// x: the packed chunks, floats or 16-bit PCM (the _i16 entry points: both kernels have a PCM build, and the advance is the frame
// pool's ss_stream_advance_packed_i16 -- the pool rows stay float either way).
int launch_stft_stream_packed(const ss_config *cfg, int out_kind, const PoolChunks &x, size_t n_active, const int64_t *d_so, const int64_t *d_ro,
                              size_t total_rows, const int32_t *d_slots, size_t pool_streams, float *d_pool, float *out0, hipStream_t stream)
{
    if (!cfg) return ss::fail(SS_ERR_ARG, "null config");
    if (n_active == 0) return SS_OK;
    const ss::HostTables &h = cfg->host;
    if (!h.d.stft_ok) return ss::fail(SS_ERR_BAD_CONFIG, "STFT path needs fft_points >= 2 * frame_size (functions.rs:136)");
    const float *d_x = x.f;
    if (!x.ptr() || !d_so || !d_ro || !d_slots || !d_pool || !out0) return ss::fail(SS_ERR_ARG, "null buffer");
    if (x.is_pcm) {
        const int src = check_pcm_scale(x.scale);
        if (src) return src;
        if (reinterpret_cast<uintptr_t>(x.pcm) & 3u) return ss::fail(SS_ERR_ARG, "the PCM buffer must be 4-byte aligned");
    }
    if (n_active >= 0x80000000ull || pool_streams >= 0x80000000ull || total_rows >= 0x80000000ull)
        return ss::fail(SS_ERR_ARG, "n_active, pool_streams and total_rows must be below 2^31");
    if (pool_streams == 0) return ss::fail(SS_ERR_ARG, "the pool has no rows");
    const size_t S = h.params.fft_points - h.d.hop;  // >= hop >= 1
    const size_t F = h.params.fft_points / 2 + 1;
    const size_t out_floats = total_rows * (out_kind == ss::OUT_STFT ? 2 * F : h.params.num_filters);
    const size_t pbytes = pool_streams * S * sizeof(float);
    // (how far x reaches is in the device tables: its first sample stands for it here, the host form checks the whole range)
    if (ranges_overlap(d_pool, pbytes, out0, out_floats * sizeof(float)) || ranges_overlap(d_pool, pbytes, x.ptr(), x.sample_bytes()))
        return ss::fail(SS_ERR_ARG, "the pool overlaps the input or the output");
    const int drc = device_ready(cfg);  // see launch_frames
    if (drc) return drc;
    ss::FrontArgs a = stft_front_args(cfg, out_kind, out0);
    a.x = d_x;
    a.n_pad = 0u;  // continuous mode: every row is real
    const ss::StftStreamPackedArgs sp{stream_packed_args(cfg, S, 0, h.d.hop, d_so, d_ro, d_slots, n_active, pool_streams, total_rows, d_pool)};
    const ss::BatchPcmArgs pcm{x.pcm, x.scale};
    ss::LaunchInfo info{};
    Step s{Tried::declined, SS_OK};
    if (!ss::dbg_force_generic() && out_kind == ss::OUT_MEL && cfg->mel2048.ok) {
        ss::Mel2048Args m = ss::mel2048_args(ss::mel_view(cfg->mel2048, cfg->d_mel2048_tab), a);
        m.ctl = cfg->d_err;
        // declined: the configuration does not fit this kernel -> the generic build
        s = tried(x.is_pcm ? ss::launch_mel_c1024_stream_packed(m, sp, pcm, stream, cfg->num_cus, &info)
                           : ss::launch_mel_c1024_stream_packed(m, sp, stream, cfg->num_cus, &info),
                  "launch_mel_c1024_stream_packed", info);
    }
    if (!s.done())
        s = tried(x.is_pcm ? ss::launch_front_generic_stream_packed(a, sp, pcm, h.d.log2c, stream, cfg->num_cus, &info)
                           : ss::launch_front_generic_stream_packed(a, sp, h.d.log2c, stream, cfg->num_cus, &info),
                  "launch_front_generic_stream_packed", info, true);
    if (s.rc) return s.rc;
    const hipError_t e = x.is_pcm ? ss::launch_stream_advance_packed(ss::FrameStreamPackedPcmArgs{sp.e, x.pcm, x.scale}, stream)
                                  : ss::launch_stream_advance_packed(sp.e, d_x, stream);
    if (e != hipSuccess) return hip_fail(e, "launch_stream_advance_packed");
    return SS_OK;
}

// Host-pointer form, as frame_stream_packed_host: the tables are checked here, before anything touches the device; then x, the
// tables and the n_active named pool rows (a compact block whose row i is entry i's) go up, the output and the named rows come down
// on the config's first host-pipeline stream.  The caller's pool is written only once everything before it succeeded.
// x: floats or 16-bit PCM; the chunks go up as they are (2 B per sample for PCM) and the device call converts on load.
int stft_stream_packed_host(const ss_config *cfg, int out_kind, const PoolChunks &x, size_t n_active, const int64_t *so, const int32_t *slots,
                            size_t pool_streams, float *pool, float *out0)
{
    if (!cfg) return ss::fail(SS_ERR_ARG, "null config");
    if (n_active == 0) return SS_OK;
    const ss::HostTables &h = cfg->host;
    if (!h.d.stft_ok) return ss::fail(SS_ERR_BAD_CONFIG, "STFT path needs fft_points >= 2 * frame_size (functions.rs:136)");
    if (!x.ptr() || !so || !slots || !pool || !out0) return ss::fail(SS_ERR_ARG, "null buffer");
    int rc = x.is_pcm ? check_pcm_scale(x.scale) : SS_OK;
    if (rc) return rc;
    if (n_active >= 0x80000000ull || pool_streams >= 0x80000000ull)
        return ss::fail(SS_ERR_ARG, "n_active, pool_streams and total_rows must be below 2^31");
    if (pool_streams == 0) return ss::fail(SS_ERR_ARG, "the pool has no rows");
    std::vector<int64_t> ro(n_active + 1);
    rc = ss_stream_packed_row_offsets(&h.params, n_active, so, ro.data());
    if (rc || (rc = ss::check_slots(slots, n_active, pool_streams))) return rc;
    const size_t rows = static_cast<size_t>(ro[n_active]), samples = static_cast<size_t>(so[n_active]);
    if (rows >= 0x80000000ull) return ss::fail(SS_ERR_ARG, "n_active, pool_streams and total_rows must be below 2^31");
    const size_t S = h.params.fft_points - h.d.hop;
    const size_t out_floats = rows * (out_kind == ss::OUT_STFT ? 2 * (h.params.fft_points / 2 + 1) : h.params.num_filters);
    const size_t pbytes = pool_streams * S * sizeof(float);
    if (ranges_overlap(pool, pbytes, x.ptr(), samples * x.sample_bytes()) || ranges_overlap(pool, pbytes, out0, out_floats * sizeof(float)))
        return ss::fail(SS_ERR_ARG, "the pool overlaps the input or the output");
    if ((rc = check_device(cfg))) return rc;
    ss::PoolRows named;  // the named pool rows, row i = entry i's
    named.gather(pool, slots, n_active, S);
    ss_config::HostPipe &hp = cfg->pipe;
    std::lock_guard<std::mutex> lock(hp.mu);
    if (!hp.stream[0]) {
        SS_HIP(hipStreamCreateWithFlags(&hp.stream[0], hipStreamNonBlocking));
        SS_HIP(hipEventCreateWithFlags(&hp.done[0], hipEventDisableTiming));
    }
    hipStream_t st = hp.stream[0];
    const size_t tbytes = (n_active + 1) * sizeof(int64_t), sbytes = n_active * S * sizeof(float);
    DeviceBuf dx, dso, dro, dsl, dp, d0;
    // (x and the output keep one sample / float where the call has none: the device form takes no null buffer)
    if ((rc = dx.alloc((samples ? samples : 1) * x.sample_bytes())) || (rc = dso.alloc(tbytes)) || (rc = dro.alloc(tbytes)) ||
        (rc = dsl.alloc(n_active * sizeof(int32_t))) || (rc = dp.alloc(sbytes)) || (rc = d0.alloc((out_floats ? out_floats : 1) * sizeof(float))))
        return rc;
    hipError_t e = samples ? hipMemcpyAsync(dx.p, x.ptr(), samples * x.sample_bytes(), hipMemcpyHostToDevice, st) : hipSuccess;
    if (e == hipSuccess) e = hipMemcpyAsync(dso.p, so, tbytes, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(dro.p, ro.data(), tbytes, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(dsl.p, named.iota.data(), n_active * sizeof(int32_t), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(dp.p, named.rows_host.data(), sbytes, hipMemcpyHostToDevice, st);
    if (e != hipSuccess) rc = hip_fail(e, "hipMemcpyAsync (H2D)");
    if (rc == SS_OK)
        rc = launch_stft_stream_packed(cfg, out_kind, x.is_pcm ? PoolChunks(dx.as<const int16_t>(), x.scale) : PoolChunks(dx.as<const float>()), n_active, dso.as<const int64_t>(), dro.as<const int64_t>(), rows,
                                       dsl.as<const int32_t>(), n_active, dp.as<float>(), d0.as<float>(), st);
    if (rc == SS_OK && out_floats > 0) {
        e = hipMemcpyAsync(out0, d0.p, out_floats * sizeof(float), hipMemcpyDeviceToHost, st);
        if (e != hipSuccess) rc = hip_fail(e, "hipMemcpyAsync (D2H)");
    }
    // the copies may still touch the caller's buffers and ours: synchronise whatever happened
    e = hipStreamSynchronize(st);
    if (e != hipSuccess && rc == SS_OK) rc = hip_fail(e, "stream pool host call");
    if (rc == SS_OK) rc = pending_device_error(cfg);
    if (rc == SS_OK) {
        e = hipMemcpyAsync(named.rows_host.data(), dp.p, sbytes, hipMemcpyDeviceToHost, st);
        const hipError_t es = hipStreamSynchronize(st);
        if (e != hipSuccess || es != hipSuccess) rc = hip_fail(e != hipSuccess ? e : es, "hipMemcpyAsync (pool rows D2H)");
        if (rc == SS_OK) named.scatter(pool, slots);
    }
    return rc;
}

// stack_frames (processing.rs:65-129): frames[clip][t][i] = x[clip][t * step + i] (* window[i]); one thread per element,
// neighbouring threads on neighbouring samples of a frame.  frame_mode as in the fused kernels' loaders: contract framing,
// zero_padding = true (zeros past the signal), the literal exact_chunks copy (all-zero rows for > 2 frames, x[0 .. flen & ~1]
// in every row otherwise), librosa's centred frames.
__global__ __launch_bounds__(256) void ss_stack_frames_kernel(const float *__restrict__ x, unsigned long long ld, unsigned n_samples, unsigned flen,
                                                             unsigned step, unsigned n_frames, int frame_mode, int pad_reflect,
                                                             const float *__restrict__ window, float *__restrict__ frames, unsigned long long total)
{
    const unsigned long long g = static_cast<unsigned long long>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (g >= total) return;
    const unsigned i = static_cast<unsigned>(g % flen);
    const unsigned long long row = g / flen;
    const unsigned t = static_cast<unsigned>(row % n_frames);
    const float *xc = x + (row / n_frames) * ld;
    float v = 0.0f;
    if (frame_mode == ss::FRAME_NORMAL) {
        v = xc[t * step + i];
    } else if (frame_mode == ss::FRAME_PADDED) {
        const unsigned idx = t * step + i;
        v = idx < n_samples ? xc[idx] : 0.0f;
    } else if (frame_mode == ss::FRAME_FIRST) {
        v = i < (flen & ~1u) ? xc[i] : 0.0f;
    } else if (frame_mode == ss::FRAME_CENTER) {
        long long pos = static_cast<long long>(t) * step + i - flen / 2;
        const long long ns = n_samples;
        bool inside = true;
        if (pos < 0 || pos >= ns) {
            if (pad_reflect) pos = pos < 0 ? -pos : 2 * (ns - 1) - pos;
            else inside = false;
        }
        v = inside ? xc[pos] : 0.0f;
    }  // FRAME_ZERO: zeros
    if (window) v *= window[i];
    frames[g] = v;
}

// The same for the common case -- contract framing, frame length, step and leading dimension multiples of four samples, 16-byte
// aligned buffers: a wave copies rows as float4s (one scalar division per row instead of two 64-bit ones per element).
__global__ __launch_bounds__(64) void ss_stack_frames_rows4(const float *__restrict__ x, unsigned long long ld, unsigned flen4, unsigned step,
                                                            unsigned n_frames, const float *__restrict__ window, float *__restrict__ frames,
                                                            unsigned long long rows, unsigned rows_per_block)
{
    const unsigned long long r0 = static_cast<unsigned long long>(blockIdx.x) * rows_per_block;
    for (unsigned k = 0; k < rows_per_block && r0 + k < rows; ++k) {
        const unsigned long long row = r0 + k;
        const unsigned long long clip = row / n_frames;
        const unsigned t = static_cast<unsigned>(row - clip * n_frames);
        const float4 *src = reinterpret_cast<const float4 *>(x + clip * ld + static_cast<unsigned long long>(t) * step);
        float4 *dst = reinterpret_cast<float4 *>(frames) + row * flen4;
        for (unsigned i = threadIdx.x; i < flen4; i += 64) {
            float4 v = src[i];
            if (window) {
                const float4 w = reinterpret_cast<const float4 *>(window)[i];
                v = make_float4(v.x * w.x, v.y * w.y, v.z * w.z, v.w * w.w);
            }
            dst[i] = v;
        }
    }
}

int check_device(const ss_config *cfg)
{
    int dev = -1;
    SS_HIP(hipGetDevice(&dev));
    if (dev != cfg->device) return ss::fail(SS_ERR_ARG, "config was created on a different HIP device than the current one");
    return SS_OK;
}

// ---- host-pointer pipeline ---------------------------------------------------------------------
// The reference's callers hand over host arrays (feature.rs:99 takes an ArrayView1, py lib.rs:167-177 a numpy array).
// `units` rows of `n` samples (row stride `ld`) are cut into chunks of a few MB; chunk k uses buffer set k % 2 on its own
// stream: H2D copy, kernel launch, D2H copy, all asynchronous, so the copy of chunk k + 1 runs while chunk k computes and
// returns (PCIe is full duplex).  Pinned caller memory (hipHostMalloc / hipHostRegister / torch pin_memory) is DMA'd directly;
// for pageable memory the runtime stages the copy and hipMemcpyAsync returns once the staging is done.
// launch(d_x, units_in_chunk, d_out0, d_out1, stream) issues the kernels for one chunk.
// T: the sample type -- float, or int16_t for the _i16 host forms, whose samples cross the link (and the mapped staging) as int16;
// the chunk size and the small-call threshold are in bytes either way.
template <typename T, typename Launch>
int host_pipeline(const ss_config *cfg, const T *x, size_t units, size_t n, size_t ld, float *out0, size_t out0_per_unit,
                  float *out1, size_t out1_per_unit, Launch launch)
{
    ss_config::HostPipe &hp = cfg->pipe;
    std::lock_guard<std::mutex> lock(hp.mu);
#if SS_LAB
    static const size_t chunk_bytes = [] {
        const char *e = std::getenv("SS_HOST_CHUNK_MB");  // A/B knob (lab build)
        const long mb = e ? std::atol(e) : 16;
        return static_cast<size_t>(mb > 0 ? mb : 16) << 20;
    }();
#else
    constexpr size_t chunk_bytes = size_t(16) << 20;
#endif
    for (int b = 0; b < 2; ++b) {
        if (!hp.stream[b]) {
            SS_HIP(hipStreamCreateWithFlags(&hp.stream[b], hipStreamNonBlocking));
            SS_HIP(hipEventCreateWithFlags(&hp.done[b], hipEventDisableTiming));
        }
    }
    // Small calls -- a single utterance, the reference's mfcc(signal) -- are latency-bound: two copy commands and their
    // completion signals cost more than moving the bytes.  Up to SS_HOST_SMALL_KB (default 1024; measured crossover between
    // 1 and 2 MB of samples, tools/latency.py) of input and of output
    // the samples are copied into pinned, device-mapped memory by the CPU, the kernel reads them and writes its results
    // through the mapping, and the only stream operations are the launch and one synchronise.
#if SS_LAB
    static const size_t small_bytes = [] {
        const char *e = std::getenv("SS_HOST_SMALL_KB");  // A/B knob (lab build)
        const long kb = e ? std::atol(e) : 1024;
        return static_cast<size_t>(kb > 0 ? kb : 0) << 10;
    }();
#else
    constexpr size_t small_bytes = size_t(1024) << 10;
#endif
    const size_t in_all = ((units - 1) * ld + n) * sizeof(T), o0_all = units * out0_per_unit * sizeof(float),
                 o1_all = out1 ? units * out1_per_unit * sizeof(float) : 0;
    if (units > 0 && in_all <= small_bytes && o0_all <= small_bytes && o1_all <= small_bytes) {
        const size_t need[3] = {in_all, o0_all, o1_all};
        for (int i = 0; i < 3; ++i) {
            if (need[i] <= hp.cap_small[i]) continue;
            SS_HIP(hipStreamSynchronize(hp.stream[0]));
            if (hp.h_small[i]) (void)hipHostFree(hp.h_small[i]);
            hp.h_small[i] = hp.d_small[i] = nullptr;
            hp.cap_small[i] = 0;
            const size_t cap = std::max<size_t>(need[i], 64 << 10);
            SS_HIP(hipHostMalloc(&hp.h_small[i], cap, hipHostMallocMapped));
            SS_HIP(hipHostGetDevicePointer(&hp.d_small[i], hp.h_small[i], 0));
            hp.cap_small[i] = cap;
        }
        std::memcpy(hp.h_small[0], x, in_all);
        int rc = launch(static_cast<const T *>(hp.d_small[0]), units, static_cast<float *>(hp.d_small[1]), static_cast<float *>(hp.d_small[2]), hp.stream[0]);
        const hipError_t e = hipStreamSynchronize(hp.stream[0]);
        if (e != hipSuccess && rc == SS_OK) rc = hip_fail(e, "host call (mapped staging)");
        if (rc == SS_OK) rc = pending_device_error(cfg);
        if (rc == SS_OK) {
            std::memcpy(out0, hp.h_small[1], o0_all);
            if (out1) std::memcpy(out1, hp.h_small[2], o1_all);
        }
        return rc;
    }
    size_t cu = chunk_bytes / (ld * sizeof(T));
    if (cu == 0) cu = 1;
    if (cu > units) cu = units;
    const size_t in_cap = ((cu - 1) * ld + n) * sizeof(T), o0_cap = cu * out0_per_unit * sizeof(float), o1_cap = cu * out1_per_unit * sizeof(float);
    auto grow = [&](void *(&buf)[2], size_t &cap, size_t need) -> int {
        if (need <= cap) return SS_OK;
        // the capacity is void until BOTH new buffers exist: a failed hipMalloc must not leave a non-zero cap beside a
        // freed pointer (every later call with need <= cap would launch on a null buffer)
        cap = 0;
        for (int b = 0; b < 2; ++b) {
            SS_HIP(hipStreamSynchronize(hp.stream[b]));
            if (buf[b]) (void)hipFree(buf[b]);
            buf[b] = nullptr;
        }
        for (int b = 0; b < 2; ++b) {
            const hipError_t e = hipMalloc(&buf[b], need);
            if (e != hipSuccess) {
                buf[b] = nullptr;
                if (buf[0]) (void)hipFree(buf[0]);
                buf[0] = buf[1] = nullptr;
                return hip_fail(e, "hipMalloc (host pipeline buffers)");
            }
        }
        cap = need;
        return SS_OK;
    };
    int rc;
    if ((rc = grow(hp.d_in, hp.cap_in, in_cap)) || (rc = grow(hp.d_out0, hp.cap_out0, o0_cap))) return rc;
    if (out1 && (rc = grow(hp.d_out1, hp.cap_out1, o1_cap))) return rc;
    size_t k = 0;
    for (size_t u0 = 0; u0 < units; u0 += cu, ++k) {
        const int b = static_cast<int>(k & 1);
        const size_t c = std::min(cu, units - u0);
        hipStream_t st = hp.stream[b];
        // the stream orders this chunk behind the previous use of the same buffer set.  A failure only breaks out of the
        // loop: earlier chunks may still have copies in flight that touch the caller's x / out buffers, so both streams are
        // synchronised below before this function returns, whatever happened.
        hipError_t e = hipMemcpyAsync(hp.d_in[b], x + u0 * ld, ((c - 1) * ld + n) * sizeof(T), hipMemcpyHostToDevice, st);
        if (e != hipSuccess) { rc = hip_fail(e, "hipMemcpyAsync (H2D)"); break; }
        rc = launch(static_cast<const T *>(hp.d_in[b]), c, static_cast<float *>(hp.d_out0[b]), static_cast<float *>(hp.d_out1[b]), st);
        if (rc) break;
        e = hipMemcpyAsync(out0 + u0 * out0_per_unit, hp.d_out0[b], c * out0_per_unit * sizeof(float), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess && out1) e = hipMemcpyAsync(out1 + u0 * out1_per_unit, hp.d_out1[b], c * out1_per_unit * sizeof(float), hipMemcpyDeviceToHost, st);
        if (e != hipSuccess) { rc = hip_fail(e, "hipMemcpyAsync (D2H)"); break; }
    }
    for (int b = 0; b < 2; ++b) {
        const hipError_t e = hipStreamSynchronize(hp.stream[b]);
        if (e != hipSuccess && rc == SS_OK) rc = hip_fail(e, "host pipeline");
    }
    if (rc == SS_OK) rc = pending_device_error(cfg);
    return rc;
}

// ---- packed variable-length clips (ss_*_packed*) ---------------------------------------------------
// Clip b is d_x[so[b] : so[b+1]], its features rows fo[b] .. fo[b+1] of out0 (and out1); the offset tables are device arrays, read
// by the kernel only (nothing of them passes through the host here: the launch is graph-capturable).  One launch over every
// clip's frames; the kernel checks the tables against each other (VarlenArgs, ss_device.h).
// x: the packed samples, floats or 16-bit PCM (the _i16 entry points: both kernels have a PCM build, so no call converts first).
int launch_packed(const ss_config *cfg, int out_kind, const PoolChunks &x, size_t n_clips, const int64_t *d_so, const int64_t *d_fo,
                  size_t total_frames, float *out0, float *out1, hipStream_t stream)
{
    if (!cfg) return ss::fail(SS_ERR_ARG, "null config");
    if (x.is_pcm) {
        const int src = check_pcm_scale(x.scale);
        if (src) return src;
    }
    if (n_clips == 0) return SS_OK;
    const float *d_x = x.f;
    if (!x.ptr() || !d_so || !d_fo || !out0 || (out_kind == ss::OUT_MFE && !out1)) return ss::fail(SS_ERR_ARG, "null buffer");
    if (n_clips > 0x7fffffffull) return ss::fail(SS_ERR_ARG, "too many clips");
    const int drc = device_ready(cfg);  // see launch_frames
    if (drc) return drc;
    const ss::HostTables &h = cfg->host;
    ss::FrontArgs a = mfcc_front_args(cfg, out_kind, out0, out1);
    a.x = d_x;
    // literal framing: the kernel picks FRAME_ZERO / FRAME_FIRST from each clip's frame count
    if (h.params.framing == SS_FRAMING_CENTER) a.frame_mode = ss::FRAME_CENTER;
    else if (h.params.framing == SS_FRAMING_PADDED) a.frame_mode = ss::FRAME_PADDED;
    else a.frame_mode = ss::FRAME_NORMAL;
    set_dct_scales(a, ss::dct_scales_per_clip(h.params));  // as launch_frames; the reference scaling is formed per clip on the device
    ss::VarlenArgs v{};
    v.so = reinterpret_cast<const long long *>(d_so);
    v.fo = reinterpret_cast<const long long *>(d_fo);
    v.total_frames = total_frames;
    v.n_clips = static_cast<uint32_t>(n_clips);
    v.framing = h.params.framing;
    v.pad_reflect = a.pad_reflect;
    v.dct_ortho = h.params.dct_norm == SS_DCT_ORTHO;
    v.dct2_gain = h.params.dct2_gain;
    v.err = cfg->d_err;
    const ss::VarlenPcmArgs vp{v, x.pcm, x.scale};
    ss::LaunchInfo info{};
    // the headline shape (512-point MFCC, default frame shape and bank): the varlen build of the dedicated kernel -- the same bits as
    // ss_mfcc_batch_device per clip; hipErrorInvalidValue before the launch for every other configuration
    if (cfg->fast.ok && !cfg->fast.fullp && out_kind == ss::OUT_MFCC && !ss::dbg_force_generic()) {
        const ss::Fast512Args f = ss::fast512_args(cfg->fast, cfg->d_fast_tab, a);
        const Step s = tried(x.is_pcm ? ss::launch_mfcc_c256_varlen(f, vp, stream, cfg->num_cus, &info)
                                      : ss::launch_mfcc_c256_varlen(f, v, stream, cfg->num_cus, &info),
                             "launch_mfcc_c256_varlen", info);
        if (s.done()) return s.rc;
    }
    return tried(x.is_pcm ? ss::launch_front_generic_varlen(a, vp, h.d.log2c, stream, cfg->num_cus, &info)
                          : ss::launch_front_generic_varlen(a, v, h.d.log2c, stream, cfg->num_cus, &info),
                 "launch_front_generic_varlen", info, true)
        .rc;
}

// Host-pointer form: the frame offsets from the host's sample offsets, one upload, one launch, one download on the config's
// first host-pipeline stream (the host calls of a config are serialised by its mutex).
// ln: lmfe -- the features go through the in-place ln on the device and the frame energies stay there (out1 is NULL).
// x: floats or 16-bit PCM; the samples go up as they are (2 B per sample for PCM) and the device call converts on load.
int packed_host(const ss_config *cfg, int out_kind, const PoolChunks &x, size_t n_clips, const int64_t *so, float *out0, float *out1,
                bool ln = false)
{
    if (!cfg) return ss::fail(SS_ERR_ARG, "null config");
    if (x.is_pcm) {
        const int src = check_pcm_scale(x.scale);
        if (src) return src;
    }
    if (n_clips == 0) return SS_OK;
    if (!x.ptr() || !so || !out0 || (out_kind == ss::OUT_MFE && !out1 && !ln)) return ss::fail(SS_ERR_ARG, "null buffer");
    std::vector<int64_t> fo(n_clips + 1);
    int rc = ss_packed_frame_offsets(&cfg->host.params, n_clips, so, fo.data());
    if (rc) return rc;
    if ((rc = check_device(cfg))) return rc;
    const size_t rows = static_cast<size_t>(fo[n_clips]), samples = static_cast<size_t>(so[n_clips]);
    const size_t cols = out_kind == ss::OUT_MFCC ? cfg->host.params.num_cepstral : cfg->host.params.num_filters;
    ss_config::HostPipe &hp = cfg->pipe;
    std::lock_guard<std::mutex> lock(hp.mu);
    if (!hp.stream[0]) {
        SS_HIP(hipStreamCreateWithFlags(&hp.stream[0], hipStreamNonBlocking));
        SS_HIP(hipEventCreateWithFlags(&hp.done[0], hipEventDisableTiming));
    }
    hipStream_t st = hp.stream[0];
    DeviceBuf dx, dso, dfo, d0, d1;
    if ((rc = dx.alloc(samples * x.sample_bytes())) || (rc = dso.alloc((n_clips + 1) * sizeof(int64_t))) ||
        (rc = dfo.alloc((n_clips + 1) * sizeof(int64_t))) || (rc = d0.alloc(rows * cols * sizeof(float))) ||
        ((out1 || ln) && (rc = d1.alloc(rows * sizeof(float)))))
        return rc;
    hipError_t e = hipMemcpyAsync(dx.p, x.ptr(), samples * x.sample_bytes(), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(dso.p, so, (n_clips + 1) * sizeof(int64_t), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(dfo.p, fo.data(), (n_clips + 1) * sizeof(int64_t), hipMemcpyHostToDevice, st);
    if (e != hipSuccess) rc = hip_fail(e, "hipMemcpyAsync (H2D)");
    if (rc == SS_OK)
        rc = launch_packed(cfg, out_kind, x.is_pcm ? PoolChunks(dx.as<const int16_t>(), x.scale) : PoolChunks(dx.as<const float>()), n_clips,
                           dso.as<const int64_t>(), dfo.as<const int64_t>(), rows, d0.as<float>(), (out1 || ln) ? d1.as<float>() : nullptr, st);
    if (rc == SS_OK && ln) rc = ss_ln_device(d0.as<float>(), rows * cols, st);
    if (rc == SS_OK) {
        e = hipMemcpyAsync(out0, d0.p, rows * cols * sizeof(float), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess && out1) e = hipMemcpyAsync(out1, d1.p, rows * sizeof(float), hipMemcpyDeviceToHost, st);
        if (e != hipSuccess) rc = hip_fail(e, "hipMemcpyAsync (D2H)");
    }
    // the copies may still touch the caller's buffers and ours: synchronise whatever happened
    e = hipStreamSynchronize(st);
    if (e != hipSuccess && rc == SS_OK) rc = hip_fail(e, "packed host call");
    if (rc == SS_OK) rc = pending_device_error(cfg);
    return rc;
}


// ---- packed variable-length clips on the STFT path (ss_mel_spectrogram_packed* / ss_stft_packed*) ------------------------------
// Clip b is d_x[so[b] : so[b+1]], its rows ro[b] .. ro[b+1] of the packed row space; the offset tables are device arrays, read by the
// kernel only (the launch is graph-capturable).  One launch over every clip's rows; the kernel checks the tables against each other
// (VarRowsArgs, ss_device.h).
// x: the packed samples, floats or 16-bit PCM (the _i16 entry points: both kernels have a PCM build, so no call converts first).
// `dbs` (the ss_log_mel_spectrogram_packed* entry points, OUT_MEL): the dB builds of the same two kernels, and behind them -- with a
// top_db floor -- the floor pass over the clips the kernel's table check accepts.
int launch_packed_stft(const ss_config *cfg, int out_kind, const PoolChunks &x, size_t n_clips, const int64_t *d_so, const int64_t *d_ro,
                       size_t total_rows, float *out0, hipStream_t stream, DbStep *dbs = nullptr)
{
    if (!cfg) return ss::fail(SS_ERR_ARG, "null config");
    const ss::HostTables &h = cfg->host;
    if (!h.d.stft_ok) return ss::fail(SS_ERR_BAD_CONFIG, "STFT path needs fft_points >= 2 * frame_size (functions.rs:136)");
    if (x.is_pcm) {
        const int src = check_pcm_scale(x.scale);
        if (src) return src;
    }
    if (n_clips == 0) return SS_OK;
    const float *d_x = x.f;
    if (!x.ptr() || !d_so || !d_ro || !out0) return ss::fail(SS_ERR_ARG, "null buffer");
    if (n_clips > 0x7fffffffull) return ss::fail(SS_ERR_ARG, "too many clips");
    const int drc = device_ready(cfg);  // see launch_frames
    if (drc) return drc;
    ss::FrontArgs a = stft_front_args(cfg, out_kind, out0);
    a.x = d_x;
    ss::VarRowsArgs v{};
    v.so = reinterpret_cast<const long long *>(d_so);
    v.ro = reinterpret_cast<const long long *>(d_ro);
    v.total_rows = total_rows;
    v.n_clips = static_cast<uint32_t>(n_clips);
    v.hop = h.d.hop;
    v.err = cfg->d_err;
    const ss::BatchPcmArgs pcm{x.pcm, x.scale};
    ss::LaunchInfo own{};
    ss::LaunchInfo &info = dbs ? dbs->ran : own;
    int rc = dbs ? dbs->prepare(n_clips, stream) : SS_OK;
    if (rc) return rc;
    const ss::DbArgs *db = dbs ? &dbs->args : nullptr;
    // the floor pass behind a dB build (every packed mel launch is one)
    const auto floored = [&](int launched) {
        if (launched != SS_OK || !db || !db->max_key || !info.db_fused) return launched;
        const hipError_t e = ss::launch_db_floor_varrows(out0, v, a.n_filters, dbs->top_db, db->max_key, stream);
        return e == hipSuccess ? SS_OK : hip_fail(e, "launch_db_floor_varrows");
    };
    // the 2048-point mel shape (bank within bins 0..512): the packed build of the twelve-wave kernel -- per clip the bits of
    // ss_mel_spectrogram_device's twelve-wave build; hipErrorInvalidValue before the launch for every other configuration
    if (!ss::dbg_force_generic() && out_kind == ss::OUT_MEL && cfg->mel2048.ok && !cfg->mel2048.fullp) {
        ss::Mel2048Args m = ss::mel2048_args(ss::mel_view(cfg->mel2048, cfg->d_mel2048_tab), a);
        m.ctl = cfg->d_err;
        const Step s = tried(x.is_pcm ? ss::launch_mel_c1024_varlen(m, v, pcm, stream, cfg->num_cus, &info, db)
                                      : ss::launch_mel_c1024_varlen(m, v, stream, cfg->num_cus, &info, db),
                             "launch_mel_c1024_varlen", info);
        if (s.done()) return floored(s.rc);
    }
    return floored(tried(x.is_pcm ? ss::launch_front_generic_varrows(a, v, pcm, h.d.log2c, stream, cfg->num_cus, &info, db)
                                  : ss::launch_front_generic_varrows(a, v, h.d.log2c, stream, cfg->num_cus, &info, db),
                         "launch_front_generic_varrows", info, true)
                       .rc);
}

// Host-pointer form: the row offsets from the host's sample offsets, one upload, one launch, one download on the config's first
// host-pipeline stream (the host calls of a config are serialised by its mutex).
// x: floats or 16-bit PCM; the samples go up as they are (2 B per sample for PCM) and the device call converts on load.
// dbc (ss_log_mel_spectrogram_packed*): the device call is the log-mel one.
int packed_stft_host(const ss_config *cfg, int out_kind, const PoolChunks &x, size_t n_clips, const int64_t *so, float *out0,
                     const DbCall *dbc = nullptr)
{
    if (!cfg) return ss::fail(SS_ERR_ARG, "null config");
    if (!cfg->host.d.stft_ok) return ss::fail(SS_ERR_BAD_CONFIG, "STFT path needs fft_points >= 2 * frame_size (functions.rs:136)");
    int rc = x.is_pcm ? check_pcm_scale(x.scale) : SS_OK;
    if (rc) return rc;
    DbStep dbs;
    if (dbc && (rc = dbs.init(*dbc))) return rc;
    if (n_clips == 0) return SS_OK;
    if (!x.ptr() || !so || !out0) return ss::fail(SS_ERR_ARG, "null buffer");
    std::vector<int64_t> ro(n_clips + 1);
    rc = ss_packed_row_offsets(&cfg->host.params, n_clips, so, ro.data());
    if (rc) return rc;
    if ((rc = check_device(cfg))) return rc;
    const size_t rows = static_cast<size_t>(ro[n_clips]), samples = static_cast<size_t>(so[n_clips]);
    const size_t cols = out_kind == ss::OUT_MEL ? cfg->host.params.num_filters : 2 * (cfg->host.params.fft_points / 2 + 1);
    ss_config::HostPipe &hp = cfg->pipe;
    std::lock_guard<std::mutex> lock(hp.mu);
    if (!hp.stream[0]) {
        SS_HIP(hipStreamCreateWithFlags(&hp.stream[0], hipStreamNonBlocking));
        SS_HIP(hipEventCreateWithFlags(&hp.done[0], hipEventDisableTiming));
    }
    hipStream_t st = hp.stream[0];
    DeviceBuf dx, dso, dro, d0;
    if ((rc = dx.alloc(samples * x.sample_bytes())) || (rc = dso.alloc((n_clips + 1) * sizeof(int64_t))) ||
        (rc = dro.alloc((n_clips + 1) * sizeof(int64_t))) || (rc = d0.alloc(rows * cols * sizeof(float))))
        return rc;
    hipError_t e = hipMemcpyAsync(dx.p, x.ptr(), samples * x.sample_bytes(), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(dso.p, so, (n_clips + 1) * sizeof(int64_t), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(dro.p, ro.data(), (n_clips + 1) * sizeof(int64_t), hipMemcpyHostToDevice, st);
    if (e != hipSuccess) rc = hip_fail(e, "hipMemcpyAsync (H2D)");
    if (rc == SS_OK)
        rc = launch_packed_stft(cfg, out_kind, x.is_pcm ? PoolChunks(dx.as<const int16_t>(), x.scale) : PoolChunks(dx.as<const float>()), n_clips, dso.as<const int64_t>(), dro.as<const int64_t>(), rows,
                                d0.as<float>(), st, dbc ? &dbs : nullptr);
    if (rc == SS_OK) {
        e = hipMemcpyAsync(out0, d0.p, rows * cols * sizeof(float), hipMemcpyDeviceToHost, st);
        if (e != hipSuccess) rc = hip_fail(e, "hipMemcpyAsync (D2H)");
    }
    // the copies may still touch the caller's buffers and ours: synchronise whatever happened
    e = hipStreamSynchronize(st);
    if (e != hipSuccess && rc == SS_OK) rc = hip_fail(e, "packed host call");
    if (rc == SS_OK) rc = pending_device_error(cfg);
    return rc;
}

// The equal-length log-mel call (ss_log_mel_spectrogram*_device): launch_stft's mel launch with the dB step around it.  On a dB build
// that is the whole conversion; behind a kernel without one (the eight-wave 2048-point builds, the 512 / 1024 / 4096-point mel
// kernels) the in-place pass over the block follows -- the same element arithmetic, the same maxima -- and the name reported is the
// mel kernel's + "+db".  With a top_db floor the equal-segment floor pass is the last launch.  A linear chain on `stream`.
int log_mel_dense(const ss_config *cfg, const float *d_x, const ss::BatchPcmArgs *pcm, size_t channels, size_t n, size_t ld, const DbCall &c,
                  float *d_out, hipStream_t stream)
{
    DbStep dbs;
    int rc = dbs.init(c);
    if (rc) return rc;
    rc = launch_stft(cfg, ss::OUT_MEL, d_x, channels, n, ld, d_out, stream, nullptr, pcm, &dbs);
    if (rc || !dbs.ran.kernel_name) return rc;
    size_t R = 0, Rreal = 0;
    if ((rc = ss::stft_rows(cfg->host.params, n, R, Rreal))) return rc;
    const size_t seg = R * cfg->host.params.num_filters;
    if (!dbs.ran.db_fused) {
        const hipError_t e = ss::launch_power_to_db_equal(d_out, channels, seg, dbs.args, stream);
        if (e != hipSuccess) return hip_fail(e, "launch_power_to_db_equal");
        g_last_kernel = plus_db_name(dbs.ran.kernel_name);
    }
    if (dbs.args.max_key) {
        const hipError_t e = ss::launch_db_floor_equal(d_out, channels, seg, c.top_db, dbs.args.max_key, stream);
        if (e != hipSuccess) return hip_fail(e, "launch_db_floor_equal");
    }
    return SS_OK;
}

int log_mel_packed(const ss_config *cfg, const PoolChunks &x, size_t n_clips, const int64_t *d_so, const int64_t *d_ro, size_t total_rows,
                   const DbCall &c, float *d_out, hipStream_t stream)
{
    DbStep dbs;
    const int rc = dbs.init(c);
    return rc ? rc : launch_packed_stft(cfg, ss::OUT_MEL, x, n_clips, d_so, d_ro, total_rows, d_out, stream, &dbs);
}

// Host-pointer form of the equal-length STFT-path calls (ss_stft / ss_mel_spectrogram and their _i16 forms): T = float, or int16_t
// with pcm_scale -- the samples then cross the link as int16 (host_pipeline<int16_t>) and the device call converts.
// dbc (ss_log_mel_spectrogram / _i16, mel output): every piece of the pipeline is a log-mel device call (a clip's maximum is its own).
template <typename T>
int stft_host(const ss_config *cfg, int out_kind, const T *x, size_t channels, size_t n_samples, float pcm_scale, float *out,
              const DbCall *dbc = nullptr)
{
    constexpr bool kPcm = std::is_same_v<T, int16_t>;
    if (!cfg || !x || !out) return ss::fail(SS_ERR_ARG, "null argument");
    int rc = kPcm ? check_pcm_scale(pcm_scale) : SS_OK;
    if (rc) return rc;
    if (dbc && (rc = check_db(*dbc))) return rc;
    size_t R = 0, Rreal = 0;
    rc = ss::stft_rows(cfg->host.params, n_samples, R, Rreal);
    if (rc) return rc;
    if (channels == 0) return SS_OK;
    if (n_samples == 0) return ss::fail(SS_ERR_ARG, "empty signal");
    rc = check_device(cfg);
    if (rc) return rc;
    const size_t per_channel = out_kind == ss::OUT_STFT ? R * (cfg->host.params.fft_points / 2 + 1) * 2 : cfg->host.params.num_filters * R;
    return host_pipeline(cfg, x, channels, n_samples, n_samples, out, per_channel, nullptr, 0,
                         [&](const T *d_x, size_t c, float *d_o0, float *, hipStream_t st) {
                             if constexpr (kPcm) {
                                 const ss::BatchPcmArgs pcm{d_x, pcm_scale};
                                 if (dbc) return log_mel_dense(cfg, nullptr, &pcm, c, n_samples, n_samples, *dbc, d_o0, st);
                                 return launch_stft(cfg, out_kind, nullptr, c, n_samples, n_samples, d_o0, st, nullptr, &pcm);
                             } else {
                                 if (dbc) return log_mel_dense(cfg, d_x, nullptr, c, n_samples, n_samples, *dbc, d_o0, st);
                                 return launch_stft(cfg, out_kind, d_x, c, n_samples, n_samples, d_o0, st);
                             }
                         });
}

}  // namespace

namespace ss {
void note_kernel(const char *name) { g_last_kernel = name; }
}  // namespace ss

extern "C" {

int ss_device_count(int *count)
{
    if (!count) return ss::fail(SS_ERR_ARG, "null argument");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) {
        *count = 0;
        return hip_fail(e, "hipGetDeviceCount");
    }
    *count = n;
    return SS_OK;
}

int ss_set_device(int device)
{
    SS_HIP(hipSetDevice(device));
    return SS_OK;
}

int ss_config_create(const ss_params *p, ss_config **out)
{
    if (!p || !out) return ss::fail(SS_ERR_ARG, "null argument");
    *out = nullptr;
    std::unique_ptr<ss_config> cfg(new ss_config());
    int rc = ss::build_tables(*p, cfg->host);
    if (rc) return rc;
    if (!ss::have_device()) return ss::no_device("hot path");
    SS_HIP(hipGetDevice(&cfg->device));
    hipDeviceProp_t prop;
    SS_HIP(hipGetDeviceProperties(&prop, cfg->device));
    cfg->num_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    const ss::HostTables &h = cfg->host;
    ss_config *c = cfg.get();
#define SS_UP(field, vec)                                                              \
    do {                                                                               \
        rc = upload(&c->field, (vec).data(), (vec).size() * sizeof((vec)[0]));         \
        if (rc) { ss_config_destroy(cfg.release()); return rc; }                       \
    } while (0)
    SS_UP(d_window_mfcc, h.window_mfcc);
    SS_UP(d_window_stft, h.window_stft);
    SS_UP(d_tw_c, h.tw_c);
    SS_UP(d_tw_n, h.tw_n);
    if (h.d.bluestein) {
        SS_UP(d_blu_c, h.blu_c);
        SS_UP(d_blu_b, h.blu_b);
    }
    SS_UP(d_f_start, h.bank.start);
    SS_UP(d_f_len, h.bank.len);
    SS_UP(d_f_off, h.bank.off);
    SS_UP(d_f_w, h.bank.w);
    SS_UP(d_dct, h.dct);
    ss::build_fast512(h, c->fast);
    if (c->fast.ok) {
        SS_UP(d_fast_tab, c->fast.tab);
    }
    ss::build_mfcc4096(h, c->mfcc4096);
    if (c->mfcc4096.ok) SS_UP(d_mfcc4096_tab, c->mfcc4096.tab);
    ss::build_mfcc2048(h, c->mfcc2048);
    if (c->mfcc2048.ok) SS_UP(d_mfcc2048_tab, c->mfcc2048.tab);
    ss::build_mfcc1024(h, c->mfcc1024);
    if (c->mfcc1024.ok) SS_UP(d_mfcc1024_tab, c->mfcc1024.tab);
    ss::build_mfcc256(h, c->mfcc256);
    if (c->mfcc256.ok) SS_UP(d_mfcc256_tab, c->mfcc256.tab);
    // the wide-bank build also serves what the headline kernel's specialised builds leave out at 512 points (mfe / window /
    // centred frames at other than the default frame shape)
    ss::build_mfcc512w(h, c->mfcc512w);
    if (c->mfcc512w.ok) SS_UP(d_mfcc512w_tab, c->mfcc512w.tab);
    ss::build_mel512(h, c->mel512);
    if (c->mel512.ok || c->mel512.stft_only) SS_UP(d_mel512_tab, c->mel512.tab);
    ss::build_mel1024(h, c->mel1024);
    if (c->mel1024.ok || c->mel1024.stft_only) SS_UP(d_mel1024_tab, c->mel1024.tab);
    ss::build_mel4096(h, c->mel4096);
    if (c->mel4096.ok || c->mel4096.stft_only) SS_UP(d_mel4096_tab, c->mel4096.tab);
    ss::build_mel2048(h, c->mel2048);
    if (c->mel2048.ok || c->mel2048.stft_only) SS_UP(d_mel2048_tab, c->mel2048.tab);
#undef SS_UP
    {
        // device error word (see ss_config): pinned and device-mapped, so that a kernel's store is visible to the host without
        // a copy and costs nothing unless it happens
        void *hp = nullptr, *dp = nullptr;
        hipError_t e2 = hipHostMalloc(&hp, 64, hipHostMallocMapped);
        if (e2 == hipSuccess) e2 = hipHostGetDevicePointer(&dp, hp, 0);
        if (e2 != hipSuccess) {
            if (hp) (void)hipHostFree(hp);
            ss_config_destroy(cfg.release());
            return hip_fail(e2, "hipHostMalloc (device error word)");
        }
        std::memset(hp, 0, 64);
        c->h_err = static_cast<unsigned *>(hp);
        c->d_err = static_cast<unsigned *>(dp);
    }
    *out = cfg.release();
    return SS_OK;
}

void ss_config_destroy(ss_config *cfg)
{
    if (!cfg) return;
    void *ptrs[] = {cfg->d_window_mfcc, cfg->d_window_stft, cfg->d_tw_c, cfg->d_tw_n, cfg->d_blu_c, cfg->d_blu_b, cfg->d_f_start,
                    cfg->d_f_len,       cfg->d_f_off,       cfg->d_f_w,  cfg->d_dct,
                    cfg->d_fast_tab,    cfg->d_mel2048_tab, cfg->d_mfcc4096_tab, cfg->d_mfcc2048_tab, cfg->d_mfcc1024_tab, cfg->d_mfcc256_tab, cfg->d_mfcc512w_tab, cfg->d_mel512_tab, cfg->d_mel1024_tab, cfg->d_mel4096_tab};
    for (void *p : ptrs)
        if (p) (void)hipFree(p);
    for (int b = 0; b < 2; ++b) {
        if (cfg->pipe.stream[b]) (void)hipStreamSynchronize(cfg->pipe.stream[b]);
        for (void *p : {cfg->pipe.d_in[b], cfg->pipe.d_out0[b], cfg->pipe.d_out1[b]})
            if (p) (void)hipFree(p);
        if (cfg->pipe.done[b]) (void)hipEventDestroy(cfg->pipe.done[b]);
        if (cfg->pipe.stream[b]) (void)hipStreamDestroy(cfg->pipe.stream[b]);
    }
    for (void *p : cfg->pipe.h_small)
        if (p) (void)hipHostFree(p);
    if (cfg->h_err) (void)hipHostFree(cfg->h_err);
    delete cfg;
}

int ss_config_params(const ss_config *cfg, ss_params *out)
{
    if (!cfg || !out) return ss::fail(SS_ERR_ARG, "null argument");
    *out = cfg->host.params;
    return SS_OK;
}

int ss_config_device_status(const ss_config *cfg)
{
    if (!cfg) return ss::fail(SS_ERR_ARG, "null config");
    return pending_device_error(cfg);
}

// ---- device-pointer variants ---------------------------------------------------------------

int ss_mfcc_batch_device(const ss_config *cfg, const float *d_x, size_t batch, size_t n_samples, size_t ld,
                         float *d_out, void *stream)
{
    return launch_frames(cfg, ss::OUT_MFCC, d_x, batch, n_samples, ld, d_out, nullptr, static_cast<hipStream_t>(stream));
}

// Several independent batches of equal-length clips per call.  Where the configuration's kernel takes a batch table (the 512-point
// MFCC kernel's default build: ss_mfcc512.hip, MULTI) up to ss::kMaxLaunchBatches batches share ONE launch -- the persistent
// workgroups' work range is the concatenation of the batches' frame quads, so a launch's start-up and its one-unit tail are paid
// once per call instead of once per batch; every other configuration is served batch by batch on the same stream.  Either way the
// results are those of n_batches separate ss_mfcc_batch_device calls, bit for bit.
int ss_mfcc_batches_device(const ss_config *cfg, size_t n_batches, const float *const *d_x, const size_t *batch, size_t n_samples,
                           size_t ld, float *const *d_out, void *stream)
{
    if (!cfg) return ss::fail(SS_ERR_ARG, "null config");
    if (n_batches == 0) return SS_OK;
    if (!d_x || !batch || !d_out) return ss::fail(SS_ERR_ARG, "null batch table");
    if (ld < n_samples) return ss::fail(SS_ERR_ARG, "leading dimension smaller than n_samples");
    {
        size_t T = 0;  // the clip shape is checked before anything is launched (every batch has the same one)
        const int rc = ss::num_frames(cfg->host.params, n_samples, T);
        if (rc) return rc;
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    return launch_batches(n_batches, d_x, batch, d_out, "batch too large", [&](const float *x, size_t clips, float *out, const MultiBatches *mb) {
        return launch_frames(cfg, ss::OUT_MFCC, x, clips, n_samples, ld, out, nullptr, st, false, mb);
    });
}

int ss_mfe_batch_device(const ss_config *cfg, const float *d_x, size_t batch, size_t n_samples, size_t ld,
                        float *d_feat, float *d_energy, void *stream)
{
    if (!d_energy) return ss::fail(SS_ERR_ARG, "null buffer");
    return launch_frames(cfg, ss::OUT_MFE, d_x, batch, n_samples, ld, d_feat, d_energy, static_cast<hipStream_t>(stream));
}

int ss_mfcc_packed_device(const ss_config *cfg, const float *d_x, size_t n_clips, const int64_t *d_sample_offsets,
                          const int64_t *d_frame_offsets, size_t total_frames, float *d_out, void *stream)
{
    return launch_packed(cfg, ss::OUT_MFCC, d_x, n_clips, d_sample_offsets, d_frame_offsets, total_frames, d_out, nullptr,
                         static_cast<hipStream_t>(stream));
}

int ss_mfe_packed_device(const ss_config *cfg, const float *d_x, size_t n_clips, const int64_t *d_sample_offsets,
                         const int64_t *d_frame_offsets, size_t total_frames, float *d_feat, float *d_energy, void *stream)
{
    return launch_packed(cfg, ss::OUT_MFE, d_x, n_clips, d_sample_offsets, d_frame_offsets, total_frames, d_feat, d_energy,
                         static_cast<hipStream_t>(stream));
}

// ---- the one-shot calls fed signed 16-bit PCM: sample = (float)pcm * scale (speechsauce_amd.h) ----
int ss_mfcc_batch_i16_device(const ss_config *cfg, const int16_t *d_x, size_t batch, size_t n_samples, size_t ld, float scale,
                             float *d_out, void *stream)
{
    const ss::BatchPcmArgs pcm{d_x, scale};
    return launch_frames(cfg, ss::OUT_MFCC, nullptr, batch, n_samples, ld, d_out, nullptr, static_cast<hipStream_t>(stream), false, nullptr,
                         &pcm);
}

int ss_mfe_batch_i16_device(const ss_config *cfg, const int16_t *d_x, size_t batch, size_t n_samples, size_t ld, float scale,
                            float *d_feat, float *d_energy, void *stream)
{
    if (!d_energy) return ss::fail(SS_ERR_ARG, "null buffer");
    const ss::BatchPcmArgs pcm{d_x, scale};
    return launch_frames(cfg, ss::OUT_MFE, nullptr, batch, n_samples, ld, d_feat, d_energy, static_cast<hipStream_t>(stream), false, nullptr,
                         &pcm);
}

int ss_mfcc_packed_i16_device(const ss_config *cfg, const int16_t *d_x, size_t n_clips, const int64_t *d_sample_offsets, float scale,
                              const int64_t *d_frame_offsets, size_t total_frames, float *d_out, void *stream)
{
    return launch_packed(cfg, ss::OUT_MFCC, PoolChunks(d_x, scale), n_clips, d_sample_offsets, d_frame_offsets, total_frames, d_out, nullptr,
                         static_cast<hipStream_t>(stream));
}

int ss_mfe_packed_i16_device(const ss_config *cfg, const int16_t *d_x, size_t n_clips, const int64_t *d_sample_offsets, float scale,
                             const int64_t *d_frame_offsets, size_t total_frames, float *d_feat, float *d_energy, void *stream)
{
    return launch_packed(cfg, ss::OUT_MFE, PoolChunks(d_x, scale), n_clips, d_sample_offsets, d_frame_offsets, total_frames, d_feat, d_energy,
                         static_cast<hipStream_t>(stream));
}

int ss_mfcc_packed_i16(const ss_config *cfg, const int16_t *x, size_t n_clips, const int64_t *sample_offsets, float scale, float *out)
{
    return packed_host(cfg, ss::OUT_MFCC, PoolChunks(x, scale), n_clips, sample_offsets, out, nullptr);
}

int ss_mfe_packed_i16(const ss_config *cfg, const int16_t *x, size_t n_clips, const int64_t *sample_offsets, float scale, float *feat,
                      float *energy)
{
    return packed_host(cfg, ss::OUT_MFE, PoolChunks(x, scale), n_clips, sample_offsets, feat, energy);
}

int ss_mfcc_packed(const ss_config *cfg, const float *x, size_t n_clips, const int64_t *sample_offsets, float *out)
{
    return packed_host(cfg, ss::OUT_MFCC, x, n_clips, sample_offsets, out, nullptr);
}

int ss_mfe_packed(const ss_config *cfg, const float *x, size_t n_clips, const int64_t *sample_offsets, float *feat, float *energy)
{
    return packed_host(cfg, ss::OUT_MFE, x, n_clips, sample_offsets, feat, energy);
}

int ss_mel_spectrogram_packed_device(const ss_config *cfg, const float *d_x, size_t n_clips, const int64_t *d_sample_offsets,
                                     const int64_t *d_row_offsets, size_t total_rows, float *d_out, void *stream)
{
    return launch_packed_stft(cfg, ss::OUT_MEL, d_x, n_clips, d_sample_offsets, d_row_offsets, total_rows, d_out,
                              static_cast<hipStream_t>(stream));
}

int ss_stft_packed_device(const ss_config *cfg, const float *d_x, size_t n_clips, const int64_t *d_sample_offsets,
                          const int64_t *d_row_offsets, size_t total_rows, float *d_out, void *stream)
{
    return launch_packed_stft(cfg, ss::OUT_STFT, d_x, n_clips, d_sample_offsets, d_row_offsets, total_rows, d_out,
                              static_cast<hipStream_t>(stream));
}

int ss_mel_spectrogram_packed(const ss_config *cfg, const float *x, size_t n_clips, const int64_t *sample_offsets, float *out)
{
    return packed_stft_host(cfg, ss::OUT_MEL, x, n_clips, sample_offsets, out);
}

int ss_stft_packed(const ss_config *cfg, const float *x, size_t n_clips, const int64_t *sample_offsets, float *out)
{
    return packed_stft_host(cfg, ss::OUT_STFT, x, n_clips, sample_offsets, out);
}

// lmfe of packed clips: ss_mfe_packed_device, then the in-place ln over the block (two stream-ordered launches, a linear chain)
int ss_lmfe_packed_device(const ss_config *cfg, const float *d_x, size_t n_clips, const int64_t *d_sample_offsets,
                          const int64_t *d_frame_offsets, size_t total_frames, float *d_feat, float *d_energy, void *stream)
{
    if (!cfg) return ss::fail(SS_ERR_ARG, "null config");
    if (n_clips == 0) return SS_OK;
    if (!d_x || !d_sample_offsets || !d_frame_offsets || !d_feat) return ss::fail(SS_ERR_ARG, "null buffer");
    if (total_frames >= (1ull << 31)) return ss::fail(SS_ERR_ARG, "feature block too large");
    hipStream_t st = static_cast<hipStream_t>(stream);
    float *tmp = nullptr;
    if (!d_energy && total_frames) {
        SS_HIP(hipMallocAsync(reinterpret_cast<void **>(&tmp), total_frames * sizeof(float), st));
        d_energy = tmp;
    }
    int rc = launch_packed(cfg, ss::OUT_MFE, d_x, n_clips, d_sample_offsets, d_frame_offsets, total_frames, d_feat, d_energy, st);
    if (rc == SS_OK) rc = ss_ln_device(d_feat, total_frames * cfg->host.params.num_filters, stream);
    if (tmp) {
        const hipError_t e = hipFreeAsync(tmp, st);
        if (e != hipSuccess && rc == SS_OK) rc = hip_fail(e, "hipFreeAsync");
    }
    return rc;
}

int ss_lmfe_packed(const ss_config *cfg, const float *x, size_t n_clips, const int64_t *sample_offsets, float *feat)
{
    return packed_host(cfg, ss::OUT_MFE, x, n_clips, sample_offsets, feat, nullptr, true);
}

// lmfe (feature.rs:242-245): ln of mfe's zero-handled filterbank energies.  The frame energies mfe also returns are
// dropped, as in the reference; a caller that has room for them passes d_energy, otherwise a stream-ordered temporary is used.
int ss_lmfe_batch_device(const ss_config *cfg, const float *d_x, size_t batch, size_t n_samples, size_t ld,
                         float *d_feat, float *d_energy, void *stream)
{
    if (!cfg) return ss::fail(SS_ERR_ARG, "null config");
    if (batch == 0) return SS_OK;
    size_t T = 0;
    int rc = ss::num_frames(cfg->host.params, n_samples, T);
    if (rc) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    float *tmp = nullptr;
    if (!d_energy) {
        SS_HIP(hipMallocAsync(reinterpret_cast<void **>(&tmp), batch * T * sizeof(float), st));
        d_energy = tmp;
    }
    rc = launch_frames(cfg, ss::OUT_MFE, d_x, batch, n_samples, ld, d_feat, d_energy, st);
    if (rc == SS_OK) rc = ss_ln_device(d_feat, batch * T * cfg->host.params.num_filters, stream);
    if (tmp) {
        const hipError_t e = hipFreeAsync(tmp, st);
        if (e != hipSuccess && rc == SS_OK) rc = hip_fail(e, "hipFreeAsync");
    }
    return rc;
}

int ss_lmfe_batch(const ss_config *cfg, const float *x, size_t batch, size_t n_samples, size_t ld, float *feat)
{
    if (!cfg || !x || !feat) return ss::fail(SS_ERR_ARG, "null argument");
    if (ld < n_samples) return ss::fail(SS_ERR_ARG, "leading dimension smaller than n_samples");
    size_t T = 0;
    int rc = ss::num_frames(cfg->host.params, n_samples, T);
    if (rc) return rc;
    if (batch == 0) return SS_OK;
    rc = check_device(cfg);
    if (rc) return rc;
    return host_pipeline(cfg, x, batch, n_samples, ld, feat, T * cfg->host.params.num_filters, nullptr, 0,
                         [&](const float *d_x, size_t c, float *d_o0, float *, hipStream_t st) {
                             return ss_lmfe_batch_device(cfg, d_x, c, n_samples, ld, d_o0, nullptr, st);
                         });
}

int ss_lmfe(const ss_config *cfg, const float *x, size_t n_samples, float *feat)
{
    return ss_lmfe_batch(cfg, x, 1, n_samples, n_samples, feat);
}

int ss_shard_bounds(size_t n_items, int world, int rank, size_t *lo, size_t *hi)
{
    if (!lo || !hi || world <= 0 || rank < 0 || rank >= world) return ss::fail(SS_ERR_ARG, "bad world / rank");
    // contiguous block partition: ranks [0, n % world) get one extra item (speechsauce_amd.distributed.shard_bounds)
    const size_t w = static_cast<size_t>(world), r = static_cast<size_t>(rank), base = n_items / w, extra = n_items % w;
    *lo = r * base + std::min(r, extra);
    *hi = *lo + base + (r < extra ? 1 : 0);
    return SS_OK;
}

}  // extern "C" (reopened below, after the RCCL resolver)

// ---- RCCL, resolved at run time (nothing is linked at build time) ---------------------------------------------------------
// The communicator is the caller's, so the functions must come from the RCCL copy that created it.  Order: a library named
// with ss_rccl_library; a copy that is ALREADY mapped into the process (dlsym(RTLD_DEFAULT), then RTLD_NOLOAD on the usual
// sonames -- a Python process that imported torch has torch/lib/librccl.so mapped, and torch.distributed's communicators
// come from it); only then a fresh dlopen of librccl.so.1 / librccl.so.
namespace {

struct Rccl {
    using all_gather_fn = int (*)(const void *, void *, size_t, int, void *, hipStream_t);
    using send_fn = int (*)(const void *, size_t, int, int, void *, hipStream_t);
    using recv_fn = int (*)(void *, size_t, int, int, void *, hipStream_t);
    using group_fn = int (*)();
    all_gather_fn all_gather = nullptr;
    send_fn send = nullptr;
    recv_fn recv = nullptr;
    group_fn group_start = nullptr, group_end = nullptr;
    std::string origin;
    bool ok() const { return all_gather && send && recv && group_start && group_end; }
};

std::mutex g_rccl_mu;
std::string g_rccl_path;       // ss_rccl_library
std::unique_ptr<Rccl> g_rccl;  // set once a resolution has succeeded
std::string g_rccl_error;      // why the last attempt failed
bool g_rccl_absent = false;    // the auto-discovery found nothing: not repeated per call (ss_rccl_library resets it)

bool rccl_from(void *handle, const char *origin, Rccl &r)
{
    r.all_gather = reinterpret_cast<Rccl::all_gather_fn>(dlsym(handle, "ncclAllGather"));
    r.send = reinterpret_cast<Rccl::send_fn>(dlsym(handle, "ncclSend"));
    r.recv = reinterpret_cast<Rccl::recv_fn>(dlsym(handle, "ncclRecv"));
    r.group_start = reinterpret_cast<Rccl::group_fn>(dlsym(handle, "ncclGroupStart"));
    r.group_end = reinterpret_cast<Rccl::group_fn>(dlsym(handle, "ncclGroupEnd"));
    r.origin = origin;
    return r.ok();
}

// (why: the reason of a failed resolution, copied under the lock)
const Rccl *rccl(std::string *why = nullptr)
{
    std::lock_guard<std::mutex> lock(g_rccl_mu);
    struct Report {
        std::string *out;
        ~Report() { if (out) *out = g_rccl_error; }
    } report{why};
    if (g_rccl) {  // only a successful resolution is kept
        g_rccl_error.clear();  // (a stale reason of an earlier, corrected attempt must not reach `why` on success)
        return g_rccl.get();
    }
    std::unique_ptr<Rccl> r(new Rccl());
    auto keep = [&]() {
        g_rccl = std::move(r);
        g_rccl_error.clear();
        return g_rccl.get();
    };
    // a handle THIS function opened and that did not resolve is closed again (one reference would leak per call)
    auto from_opened = [&](void *h, const char *origin) {
        if (!h) return false;
        if (rccl_from(h, origin, *r)) return true;
        (void)dlclose(h);
        return false;
    };
    if (!g_rccl_path.empty()) {
        void *h = dlopen(g_rccl_path.c_str(), RTLD_NOW | RTLD_LOCAL);
        const char *de = h ? nullptr : dlerror();
        if (from_opened(h, g_rccl_path.c_str())) return keep();
        // an explicit path that does not load is an error, not a reason to guess; nothing is cached, so a corrected
        // ss_rccl_library call is accepted and tried again
        g_rccl_error = g_rccl_path + (h ? ": ncclAllGather / ncclSend / ncclRecv / ncclGroupStart / ncclGroupEnd not all found" : std::string(": ") + (de ? de : "dlopen failed"));
        return nullptr;
    }
    g_rccl_error = "no mapped copy, librccl.so.1 / librccl.so not loadable";
    if (g_rccl_absent) return nullptr;  // looked already: the lookups, the /proc scan and four dlopen attempts are not repeated per call
    if (rccl_from(RTLD_DEFAULT, "already in the global symbol scope", *r)) return keep();
    for (const char *name : {"librccl.so.1", "librccl.so"}) {
        void *h = dlopen(name, RTLD_NOW | RTLD_NOLOAD);
        if (from_opened(h, "already mapped (RTLD_NOLOAD)")) return keep();
    }
    {
        // a copy mapped under another name (torch/lib/librccl.so is loaded by path): look through the process's objects
        struct Ctx { std::string path; } ctx;
        if (FILE *fp = std::fopen("/proc/self/maps", "r")) {
            char line[1024];
            while (std::fgets(line, sizeof line, fp)) {
                const char *sl = std::strchr(line, '/');
                if (sl && std::strstr(sl, "librccl.so")) {
                    ctx.path.assign(sl, std::strcspn(sl, "\n"));
                    break;
                }
            }
            std::fclose(fp);
        }
        if (!ctx.path.empty()) {
            void *h = dlopen(ctx.path.c_str(), RTLD_NOW | RTLD_NOLOAD);
            if (from_opened(h, ctx.path.c_str())) return keep();
        }
    }
    for (const char *name : {"librccl.so.1", "librccl.so"}) {
        void *h = dlopen(name, RTLD_NOW | RTLD_LOCAL);
        if (from_opened(h, name)) return keep();
    }
    g_rccl_absent = true;  // (a later ss_rccl_library call, e.g. after the caller has loaded RCCL, asks again)
    return nullptr;
}

int rccl_fail(const char *what, int rc)
{
    return ss::fail(SS_ERR_HIP, std::string(what) + " failed with ncclResult_t " + std::to_string(rc));
}

constexpr int kNcclFloat32 = 7;  // rccl.h: ncclFloat32

}  // namespace

extern "C" {

int ss_rccl_library(const char *path)
{
    std::lock_guard<std::mutex> lock(g_rccl_mu);
    if (g_rccl) return ss::fail(SS_ERR_ARG, "RCCL was already resolved (" + g_rccl->origin + "): ss_rccl_library must precede the first collective");
    g_rccl_path = path ? path : "";
    g_rccl_absent = false;
    return SS_OK;
}

int ss_all_gather_features(void *nccl_comm, const float *d_block, size_t elems_per_rank, float *d_out, void *stream)
{
    if (!nccl_comm || !d_block || !d_out) return ss::fail(SS_ERR_ARG, "null argument");
    if (elems_per_rank == 0) return SS_OK;
    std::string why;
    const Rccl *r = rccl(&why);
    if (!r) return ss::fail(SS_ERR_UNSUPPORTED, "RCCL could not be resolved (" + why + ")");
    // ncclAllGather(sendbuff, recvbuff, sendcount, datatype, comm, stream)
    const int rc = r->all_gather(d_block, d_out, elems_per_rank, kNcclFloat32, nccl_comm, static_cast<hipStream_t>(stream));
    if (rc != 0) return rccl_fail("ncclAllGather", rc);
    return SS_OK;
}

int ss_gather_features(void *nccl_comm, const float *d_block, size_t elems_per_rank, float *d_out, int root, int rank, int world,
                       void *stream)
{
    if (!nccl_comm || !d_block) return ss::fail(SS_ERR_ARG, "null argument");
    if (world <= 0 || rank < 0 || rank >= world || root < 0 || root >= world) return ss::fail(SS_ERR_ARG, "bad world / rank / root");
    if (rank == root && !d_out) return ss::fail(SS_ERR_ARG, "the root needs an output buffer");
    if (elems_per_rank == 0) return SS_OK;
    std::string why;
    const Rccl *r = rccl(&why);
    if (!r) return ss::fail(SS_ERR_UNSUPPORTED, "RCCL could not be resolved (" + why + ")");
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (rank != root) {
        const int rc = r->send(d_block, elems_per_rank, kNcclFloat32, root, nccl_comm, st);
        return rc ? rccl_fail("ncclSend", rc) : SS_OK;
    }
    // root: its own block is a device copy; one receive per peer inside a group, so that all of them progress together
    // (every peer has a direct xGMI link to the root)
    SS_HIP(hipMemcpyAsync(d_out + static_cast<size_t>(root) * elems_per_rank, d_block, elems_per_rank * sizeof(float), hipMemcpyDeviceToDevice, st));
    int rc = r->group_start();
    if (rc) return rccl_fail("ncclGroupStart", rc);
    int first_err = 0;
    for (int p = 0; p < world; ++p) {
        if (p == root) continue;
        const int e = r->recv(d_out + static_cast<size_t>(p) * elems_per_rank, elems_per_rank, kNcclFloat32, p, nccl_comm, st);
        if (e && !first_err) first_err = e;
    }
    rc = r->group_end();  // always closed, also after a failed ncclRecv
    if (first_err) return rccl_fail("ncclRecv", first_err);
    if (rc) return rccl_fail("ncclGroupEnd", rc);
    return SS_OK;
}

int ss_power_spectrum_batch_device(const ss_config *cfg, const float *d_x, size_t batch, size_t n_samples,
                                   size_t ld, float *d_P, void *stream)
{
    return launch_frames(cfg, ss::OUT_POWER, d_x, batch, n_samples, ld, d_P, nullptr, static_cast<hipStream_t>(stream));
}

int ss_power_spectrum_frames_device(const ss_config *cfg, const float *d_frames, size_t rows, size_t cols, size_t ld, float *d_P,
                                    void *stream)
{
    return launch_frames(cfg, ss::OUT_POWER, d_frames, rows, cols, ld, d_P, nullptr, static_cast<hipStream_t>(stream), true);
}

// Host-pointer forms of the stage outputs the reference exposes as pub fns (processing.rs:179-181, functions.rs:86-123,
// :199-233, processing.rs:65-129): same chunked two-stream pipeline / mapped small-call staging as ss_mfcc_batch.
int ss_power_spectrum_batch(const ss_config *cfg, const float *x, size_t batch, size_t n_samples, size_t ld, float *P)
{
    if (!cfg || !x || !P) return ss::fail(SS_ERR_ARG, "null argument");
    if (ld < n_samples) return ss::fail(SS_ERR_ARG, "leading dimension smaller than n_samples");
    size_t T = 0;
    int rc = ss::num_frames(cfg->host.params, n_samples, T);
    if (rc) return rc;
    if (batch == 0) return SS_OK;
    rc = check_device(cfg);
    if (rc) return rc;
    return host_pipeline(cfg, x, batch, n_samples, ld, P, T * (cfg->host.params.fft_points / 2 + 1), nullptr, 0,
                         [&](const float *d_x, size_t c, float *d_o0, float *, hipStream_t st) {
                             return ss_power_spectrum_batch_device(cfg, d_x, c, n_samples, ld, d_o0, st);
                         });
}

int ss_power_spectrum(const ss_config *cfg, const float *x, size_t n_samples, float *P)
{
    return ss_power_spectrum_batch(cfg, x, 1, n_samples, n_samples, P);
}

int ss_power_spectrum_frames(const ss_config *cfg, const float *frames, size_t rows, size_t cols, float *P)
{
    if (!cfg || !frames || !P) return ss::fail(SS_ERR_ARG, "null argument");
    if (cols == 0 || cols > cfg->host.params.fft_points) return ss::fail(SS_ERR_ARG, "frame length must be in [1, fft_points]");
    if (rows == 0) return SS_OK;
    const int rc = check_device(cfg);
    if (rc) return rc;
    return host_pipeline(cfg, frames, rows, cols, cols, P, cfg->host.params.fft_points / 2 + 1, nullptr, 0,
                         [&](const float *d_x, size_t c, float *d_o0, float *, hipStream_t st) {
                             return ss_power_spectrum_frames_device(cfg, d_x, c, cols, cols, d_o0, st);
                         });
}

}  // extern "C"

namespace {

// The framing kernels for `batch` clips of n_samples (row stride ld): frames [batch x T x flen]; d_window: flen floats or null.
int launch_stack_frames(const float *d_x, size_t batch, size_t n_samples, size_t ld, uint32_t flen, uint32_t step, size_t T, int mode,
                        int pad_reflect, const float *d_window, float *d_frames, hipStream_t stream)
{
    if (n_samples > 0x7fffffffull || static_cast<unsigned long long>(T) * step + flen > 0xffffffffull) return ss::fail(SS_ERR_ARG, "clip too long");
    const unsigned long long total = static_cast<unsigned long long>(batch) * T * flen;
    const bool aligned4 = mode == ss::FRAME_NORMAL && flen % 4 == 0 && step % 4 == 0 && ld % 4 == 0 &&
                          reinterpret_cast<uintptr_t>(d_x) % 16 == 0 && reinterpret_cast<uintptr_t>(d_frames) % 16 == 0 &&
                          (!d_window || reinterpret_cast<uintptr_t>(d_window) % 16 == 0);
    if (aligned4) {
        const unsigned long long rows = static_cast<unsigned long long>(batch) * T;
        const unsigned rpb = 4;
        const unsigned long long nb = (rows + rpb - 1) / rpb;
        if (nb > 0x7fffffffull) return ss::fail(SS_ERR_ARG, "batch too large");
        hipLaunchKernelGGL(ss_stack_frames_rows4, dim3(static_cast<unsigned>(nb)), dim3(64), 0, stream, d_x, static_cast<unsigned long long>(ld),
                           flen / 4, step, static_cast<unsigned>(T), d_window, d_frames, rows, rpb);
        const hipError_t e4 = hipGetLastError();
        if (e4 != hipSuccess) return hip_fail(e4, "ss_stack_frames_rows4");
        g_last_kernel = "ss_stack_frames_rows4";
        return SS_OK;
    }
    const unsigned long long blocks = (total + 255) / 256;
    if (blocks > 0x7fffffffull) return ss::fail(SS_ERR_ARG, "batch too large");
    hipLaunchKernelGGL(ss_stack_frames_kernel, dim3(static_cast<unsigned>(blocks)), dim3(256), 0, stream, d_x, static_cast<unsigned long long>(ld),
                       static_cast<unsigned>(n_samples), flen, step, static_cast<unsigned>(T), mode, pad_reflect, d_window, d_frames, total);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "ss_stack_frames_kernel");
    g_last_kernel = "ss_stack_frames_kernel";
    return SS_OK;
}

// processing.rs:77-78, :91-92, :101: frame sizes and count from the reference's own loose arguments (no SpeechConfig, no FFT length)
int frames_shape(size_t n_samples, uint32_t sample_rate, float frame_length, float frame_stride, int zero_padding, size_t &T, uint32_t &flen,
                 uint32_t &step)
{
    ss_params p{};
    int rc = ss_params_default(&p, sample_rate ? sample_rate : 1u);
    if (rc) return rc;
    if (sample_rate == 0) return ss::fail(SS_ERR_BAD_CONFIG, "sample_rate must be > 0");
    p.frame_length = frame_length;
    p.frame_stride = frame_stride;
    p.framing = zero_padding ? SS_FRAMING_PADDED : SS_FRAMING_CONTRACT;
    ss::Derived d;
    rc = ss::derive(p, d);
    if (rc) return rc;
    rc = ss::num_frames(p, n_samples, T);
    if (rc) return rc;
    flen = d.flen;
    step = d.step;
    return SS_OK;
}

}  // namespace

extern "C" {

int ss_stack_frames_device(const ss_config *cfg, const float *d_x, size_t batch, size_t n_samples, size_t ld, float *d_frames,
                           void *stream)
{
    if (!cfg) return ss::fail(SS_ERR_ARG, "null config");
    if (ld < n_samples) return ss::fail(SS_ERR_ARG, "leading dimension smaller than n_samples");
    const ss::HostTables &h = cfg->host;
    size_t T = 0;
    int rc = ss::num_frames(h.params, n_samples, T);
    if (rc) return rc;
    if (batch == 0) return SS_OK;
    if (!d_x || !d_frames) return ss::fail(SS_ERR_ARG, "null buffer");
    rc = check_device(cfg);
    if (rc) return rc;
    int mode = ss::FRAME_NORMAL;
    if (h.params.framing == SS_FRAMING_LITERAL) mode = T > 2 ? ss::FRAME_ZERO : ss::FRAME_FIRST;
    else if (h.params.framing == SS_FRAMING_CENTER) mode = ss::FRAME_CENTER;
    else if (h.params.framing == SS_FRAMING_PADDED) mode = ss::FRAME_PADDED;
    return launch_stack_frames(d_x, batch, n_samples, ld, h.d.flen, h.d.step, T, mode, h.params.pad_mode == SS_PAD_REFLECT ? 1 : 0,
                               cfg->d_window_mfcc, d_frames, static_cast<hipStream_t>(stream));
}

// ---- stack_frames with the reference's own argument list (processing.rs:65-76): no SpeechConfig, no FFT length ----

int ss_stack_frames_shape(size_t n_samples, uint32_t sample_rate, float frame_length, float frame_stride, int zero_padding,
                          size_t *num_frames, size_t *frame_len)
{
    if (!num_frames || !frame_len) return ss::fail(SS_ERR_ARG, "null argument");
    size_t T = 0;
    uint32_t flen = 0, step = 0;
    const int rc = frames_shape(n_samples, sample_rate, frame_length, frame_stride, zero_padding, T, flen, step);
    if (rc) return rc;
    *num_frames = T;
    *frame_len = flen;
    return SS_OK;
}

int ss_stack_frames_signal_device(const float *d_x, size_t n_samples, uint32_t sample_rate, float frame_length, float frame_stride,
                                  const float *d_window, int zero_padding, float *d_frames, void *stream)
{
    size_t T = 0;
    uint32_t flen = 0, step = 0;
    const int rc = frames_shape(n_samples, sample_rate, frame_length, frame_stride, zero_padding, T, flen, step);
    if (rc) return rc;
    if (!d_x || !d_frames) return ss::fail(SS_ERR_ARG, "null buffer");
    return launch_stack_frames(d_x, 1, n_samples, n_samples, flen, step, T, zero_padding ? ss::FRAME_PADDED : ss::FRAME_NORMAL, 0, d_window,
                               d_frames, static_cast<hipStream_t>(stream));
}

int ss_stack_frames_signal(const float *x, size_t n_samples, uint32_t sample_rate, float frame_length, float frame_stride,
                           const float *window, int zero_padding, float *frames)
{
    size_t T = 0;
    uint32_t flen = 0, step = 0;
    int rc = frames_shape(n_samples, sample_rate, frame_length, frame_stride, zero_padding, T, flen, step);
    if (rc) return rc;
    if (!x || !frames) return ss::fail(SS_ERR_ARG, "null argument");
    if (!ss::have_device()) return ss::no_device("hot path");
    // a cold path (no config, so no staging pipeline to reuse): plain allocations and synchronous copies
    DeviceBuf dx, dw, df;
    const size_t out_bytes = T * static_cast<size_t>(flen) * sizeof(float);
    if ((rc = dx.alloc(n_samples * sizeof(float))) || (rc = df.alloc(out_bytes))) return rc;
    if (window && (rc = dw.alloc(flen * sizeof(float)))) return rc;
    SS_HIP(hipMemcpy(dx.p, x, n_samples * sizeof(float), hipMemcpyHostToDevice));
    if (window) SS_HIP(hipMemcpy(dw.p, window, flen * sizeof(float), hipMemcpyHostToDevice));
    rc = ss_stack_frames_signal_device(dx.as<float>(), n_samples, sample_rate, frame_length, frame_stride, window ? dw.as<float>() : nullptr,
                                       zero_padding, df.as<float>(), nullptr);
    if (rc) return rc;
    SS_HIP(hipMemcpy(frames, df.p, out_bytes, hipMemcpyDeviceToHost));
    return SS_OK;
}

int ss_stack_frames(const ss_config *cfg, const float *x, size_t n_samples, float *frames)
{
    if (!cfg || !x || !frames) return ss::fail(SS_ERR_ARG, "null argument");
    size_t T = 0;
    int rc = ss::num_frames(cfg->host.params, n_samples, T);
    if (rc) return rc;
    rc = check_device(cfg);
    if (rc) return rc;
    return host_pipeline(cfg, x, 1, n_samples, n_samples, frames, T * cfg->host.d.flen, nullptr, 0,
                         [&](const float *d_x, size_t c, float *d_o0, float *, hipStream_t st) {
                             return ss_stack_frames_device(cfg, d_x, c, n_samples, n_samples, d_o0, st);
                         });
}

int ss_stft(const ss_config *cfg, const float *x, size_t channels, size_t n_samples, float *out)
{
    return stft_host(cfg, ss::OUT_STFT, x, channels, n_samples, 1.0f, out);
}

int ss_stft_i16(const ss_config *cfg, const int16_t *x, size_t channels, size_t n_samples, float scale, float *out)
{
    return stft_host(cfg, ss::OUT_STFT, x, channels, n_samples, scale, out);
}

int ss_mel_spectrogram_device(const ss_config *cfg, const float *d_x, size_t channels, size_t n_samples,
                              size_t ld, float *d_out, void *stream)
{
    return launch_stft(cfg, ss::OUT_MEL, d_x, channels, n_samples, ld, d_out, static_cast<hipStream_t>(stream));
}

// The mel-spectrogram form of ss_mfcc_batches_device: n_batches independent [channels[b] x n_samples] blocks, each with its own
// output block.  Where the configuration runs on the twelve-wave 2048-point mel build and every block is large enough to select
// that build on its own, up to ss::kMaxLaunchBatches blocks share ONE launch; otherwise block by block on `stream`.  The results
// are those of separate ss_mel_spectrogram_device calls, bit for bit.
int ss_mel_spectrogram_batches_device(const ss_config *cfg, size_t n_batches, const float *const *d_x, const size_t *channels,
                                      size_t n_samples, size_t ld, float *const *d_out, void *stream)
{
    if (!cfg) return ss::fail(SS_ERR_ARG, "null config");
    if (n_batches == 0) return SS_OK;
    if (!d_x || !channels || !d_out) return ss::fail(SS_ERR_ARG, "null batch table");
    if (ld < n_samples) return ss::fail(SS_ERR_ARG, "leading dimension smaller than n_samples");
    hipStream_t st = static_cast<hipStream_t>(stream);
    return launch_batches(n_batches, d_x, channels, d_out, "bad clip length / channel count",
                          [&](const float *x, size_t chans, float *out, const MultiBatches *mb) {
                              return launch_stft(cfg, ss::OUT_MEL, x, chans, n_samples, ld, out, st, mb);
                          });
}

int ss_stft_device(const ss_config *cfg, const float *d_x, size_t channels, size_t n_samples, size_t ld,
                   float *d_out, void *stream)
{
    return launch_stft(cfg, ss::OUT_STFT, d_x, channels, n_samples, ld, d_out, static_cast<hipStream_t>(stream));
}

// ---- the STFT-path calls fed signed 16-bit PCM: sample = (float)pcm * scale (speechsauce_amd.h) ----
int ss_mel_spectrogram_i16_device(const ss_config *cfg, const int16_t *d_x, size_t channels, size_t n_samples, size_t ld, float scale,
                                  float *d_out, void *stream)
{
    const ss::BatchPcmArgs pcm{d_x, scale};
    return launch_stft(cfg, ss::OUT_MEL, nullptr, channels, n_samples, ld, d_out, static_cast<hipStream_t>(stream), nullptr, &pcm);
}

int ss_stft_i16_device(const ss_config *cfg, const int16_t *d_x, size_t channels, size_t n_samples, size_t ld, float scale, float *d_out,
                       void *stream)
{
    const ss::BatchPcmArgs pcm{d_x, scale};
    return launch_stft(cfg, ss::OUT_STFT, nullptr, channels, n_samples, ld, d_out, static_cast<hipStream_t>(stream), nullptr, &pcm);
}

int ss_mel_spectrogram_packed_i16_device(const ss_config *cfg, const int16_t *d_x, size_t n_clips, const int64_t *d_sample_offsets, float scale,
                                         const int64_t *d_row_offsets, size_t total_rows, float *d_out, void *stream)
{
    return launch_packed_stft(cfg, ss::OUT_MEL, PoolChunks(d_x, scale), n_clips, d_sample_offsets, d_row_offsets, total_rows, d_out,
                              static_cast<hipStream_t>(stream));
}

int ss_stft_packed_i16_device(const ss_config *cfg, const int16_t *d_x, size_t n_clips, const int64_t *d_sample_offsets, float scale,
                              const int64_t *d_row_offsets, size_t total_rows, float *d_out, void *stream)
{
    return launch_packed_stft(cfg, ss::OUT_STFT, PoolChunks(d_x, scale), n_clips, d_sample_offsets, d_row_offsets, total_rows, d_out,
                              static_cast<hipStream_t>(stream));
}

int ss_mel_spectrogram_packed_i16(const ss_config *cfg, const int16_t *x, size_t n_clips, const int64_t *sample_offsets, float scale, float *out)
{
    return packed_stft_host(cfg, ss::OUT_MEL, PoolChunks(x, scale), n_clips, sample_offsets, out);
}

int ss_stft_packed_i16(const ss_config *cfg, const int16_t *x, size_t n_clips, const int64_t *sample_offsets, float scale, float *out)
{
    return packed_stft_host(cfg, ss::OUT_STFT, PoolChunks(x, scale), n_clips, sample_offsets, out);
}

int ss_mel_spectrogram_stream_packed_i16_device(const ss_config *cfg, const int16_t *d_x, size_t n_active, const int64_t *d_sample_offsets,
                                                const int64_t *d_row_offsets, size_t total_rows, const int32_t *d_slots, size_t pool_streams,
                                                float scale, float *d_pool, float *d_out, void *stream)
{
    return launch_stft_stream_packed(cfg, ss::OUT_MEL, PoolChunks(d_x, scale), n_active, d_sample_offsets, d_row_offsets, total_rows, d_slots,
                                     pool_streams, d_pool, d_out, static_cast<hipStream_t>(stream));
}

int ss_stft_stream_packed_i16_device(const ss_config *cfg, const int16_t *d_x, size_t n_active, const int64_t *d_sample_offsets,
                                     const int64_t *d_row_offsets, size_t total_rows, const int32_t *d_slots, size_t pool_streams, float scale,
                                     float *d_pool, float *d_out, void *stream)
{
    return launch_stft_stream_packed(cfg, ss::OUT_STFT, PoolChunks(d_x, scale), n_active, d_sample_offsets, d_row_offsets, total_rows, d_slots,
                                     pool_streams, d_pool, d_out, static_cast<hipStream_t>(stream));
}

int ss_mel_spectrogram_stream_packed_i16(const ss_config *cfg, const int16_t *x, size_t n_active, const int64_t *sample_offsets,
                                         const int32_t *slots, size_t pool_streams, float scale, float *pool, float *out)
{
    return stft_stream_packed_host(cfg, ss::OUT_MEL, PoolChunks(x, scale), n_active, sample_offsets, slots, pool_streams, pool, out);
}

int ss_stft_stream_packed_i16(const ss_config *cfg, const int16_t *x, size_t n_active, const int64_t *sample_offsets, const int32_t *slots,
                              size_t pool_streams, float scale, float *pool, float *out)
{
    return stft_stream_packed_host(cfg, ss::OUT_STFT, PoolChunks(x, scale), n_active, sample_offsets, slots, pool_streams, pool, out);
}

int ss_stft_stream_device(const ss_config *cfg, int mode, const float *d_x, size_t n_streams, size_t n_samples, size_t ld,
                          float *d_state, float *d_out, void *stream)
{
    return launch_stft_stream(cfg, ss::OUT_STFT, mode, d_x, n_streams, n_samples, ld, d_state, d_out, static_cast<hipStream_t>(stream));
}

int ss_mel_spectrogram_stream_device(const ss_config *cfg, int mode, const float *d_x, size_t n_streams, size_t n_samples, size_t ld,
                                     float *d_state, float *d_out, void *stream)
{
    return launch_stft_stream(cfg, ss::OUT_MEL, mode, d_x, n_streams, n_samples, ld, d_state, d_out, static_cast<hipStream_t>(stream));
}

int ss_stft_stream(const ss_config *cfg, int mode, const float *x, size_t n_streams, size_t n_samples, size_t ld, float *state,
                   float *out)
{
    return stream_host(cfg, ss::OUT_STFT, mode, x, n_streams, n_samples, ld, state, out);
}

int ss_mel_spectrogram_stream(const ss_config *cfg, int mode, const float *x, size_t n_streams, size_t n_samples, size_t ld,
                              float *state, float *out)
{
    return stream_host(cfg, ss::OUT_MEL, mode, x, n_streams, n_samples, ld, state, out);
}

int ss_mfcc_stream_device(const ss_config *cfg, const float *d_x, size_t n_streams, size_t n_samples, size_t ld, uint32_t norm_frames,
                          float *d_state, float *d_out, void *stream)
{
    return launch_frame_stream(cfg, ss::OUT_MFCC, d_x, n_streams, n_samples, ld, norm_frames, d_state, d_out, nullptr,
                               static_cast<hipStream_t>(stream));
}

int ss_mfe_stream_device(const ss_config *cfg, const float *d_x, size_t n_streams, size_t n_samples, size_t ld, float *d_state,
                         float *d_feat, float *d_energy, void *stream)
{
    return launch_frame_stream(cfg, ss::OUT_MFE, d_x, n_streams, n_samples, ld, 1u, d_state, d_feat, d_energy, static_cast<hipStream_t>(stream));
}

int ss_mfcc_stream(const ss_config *cfg, const float *x, size_t n_streams, size_t n_samples, size_t ld, uint32_t norm_frames,
                   float *state, float *out)
{
    return frame_stream_host(cfg, ss::OUT_MFCC, x, n_streams, n_samples, ld, norm_frames, state, out, nullptr);
}

int ss_mfe_stream(const ss_config *cfg, const float *x, size_t n_streams, size_t n_samples, size_t ld, float *state, float *feat,
                  float *energy)
{
    return frame_stream_host(cfg, ss::OUT_MFE, x, n_streams, n_samples, ld, 1u, state, feat, energy);
}

int ss_mfcc_stream_packed_device(const ss_config *cfg, const float *d_x, size_t n_active, const int64_t *d_sample_offsets,
                                 const int64_t *d_row_offsets, size_t total_rows, const int32_t *d_slots, size_t pool_streams,
                                 uint32_t norm_frames, float *d_pool, float *d_out, void *stream)
{
    return launch_frame_stream_packed(cfg, ss::OUT_MFCC, d_x, n_active, d_sample_offsets, d_row_offsets, total_rows, d_slots, pool_streams,
                                      norm_frames, d_pool, d_out, nullptr, static_cast<hipStream_t>(stream));
}

int ss_mfe_stream_packed_device(const ss_config *cfg, const float *d_x, size_t n_active, const int64_t *d_sample_offsets,
                                const int64_t *d_row_offsets, size_t total_rows, const int32_t *d_slots, size_t pool_streams,
                                float *d_pool, float *d_feat, float *d_energy, void *stream)
{
    return launch_frame_stream_packed(cfg, ss::OUT_MFE, d_x, n_active, d_sample_offsets, d_row_offsets, total_rows, d_slots, pool_streams, 1u,
                                      d_pool, d_feat, d_energy, static_cast<hipStream_t>(stream));
}

int ss_mfcc_stream_packed(const ss_config *cfg, const float *x, size_t n_active, const int64_t *sample_offsets, const int32_t *slots,
                          size_t pool_streams, uint32_t norm_frames, float *pool, float *out)
{
    return frame_stream_packed_host(cfg, ss::OUT_MFCC, x, n_active, sample_offsets, slots, pool_streams, norm_frames, pool, out, nullptr);
}

int ss_mfe_stream_packed(const ss_config *cfg, const float *x, size_t n_active, const int64_t *sample_offsets, const int32_t *slots,
                         size_t pool_streams, float *pool, float *feat, float *energy)
{
    return frame_stream_packed_host(cfg, ss::OUT_MFE, x, n_active, sample_offsets, slots, pool_streams, 1u, pool, feat, energy);
}

int ss_mfcc_stream_packed_i16_device(const ss_config *cfg, const int16_t *d_x, size_t n_active, const int64_t *d_sample_offsets,
                                     const int64_t *d_row_offsets, size_t total_rows, const int32_t *d_slots, size_t pool_streams,
                                     float scale, uint32_t norm_frames, float *d_pool, float *d_out, void *stream)
{
    return launch_frame_stream_packed(cfg, ss::OUT_MFCC, PoolChunks(d_x, scale), n_active, d_sample_offsets, d_row_offsets, total_rows, d_slots,
                                      pool_streams, norm_frames, d_pool, d_out, nullptr, static_cast<hipStream_t>(stream));
}

int ss_mfe_stream_packed_i16_device(const ss_config *cfg, const int16_t *d_x, size_t n_active, const int64_t *d_sample_offsets,
                                    const int64_t *d_row_offsets, size_t total_rows, const int32_t *d_slots, size_t pool_streams,
                                    float scale, float *d_pool, float *d_feat, float *d_energy, void *stream)
{
    return launch_frame_stream_packed(cfg, ss::OUT_MFE, PoolChunks(d_x, scale), n_active, d_sample_offsets, d_row_offsets, total_rows, d_slots,
                                      pool_streams, 1u, d_pool, d_feat, d_energy, static_cast<hipStream_t>(stream));
}

int ss_mfcc_stream_packed_i16(const ss_config *cfg, const int16_t *x, size_t n_active, const int64_t *sample_offsets, const int32_t *slots,
                              size_t pool_streams, float scale, uint32_t norm_frames, float *pool, float *out)
{
    return frame_stream_packed_host(cfg, ss::OUT_MFCC, PoolChunks(x, scale), n_active, sample_offsets, slots, pool_streams, norm_frames, pool,
                                    out, nullptr);
}

int ss_mfe_stream_packed_i16(const ss_config *cfg, const int16_t *x, size_t n_active, const int64_t *sample_offsets, const int32_t *slots,
                             size_t pool_streams, float scale, float *pool, float *feat, float *energy)
{
    return frame_stream_packed_host(cfg, ss::OUT_MFE, PoolChunks(x, scale), n_active, sample_offsets, slots, pool_streams, 1u, pool, feat,
                                    energy);
}

int ss_mel_spectrogram_stream_packed_device(const ss_config *cfg, const float *d_x, size_t n_active, const int64_t *d_sample_offsets,
                                            const int64_t *d_row_offsets, size_t total_rows, const int32_t *d_slots, size_t pool_streams,
                                            float *d_pool, float *d_out, void *stream)
{
    return launch_stft_stream_packed(cfg, ss::OUT_MEL, d_x, n_active, d_sample_offsets, d_row_offsets, total_rows, d_slots, pool_streams,
                                     d_pool, d_out, static_cast<hipStream_t>(stream));
}

int ss_stft_stream_packed_device(const ss_config *cfg, const float *d_x, size_t n_active, const int64_t *d_sample_offsets,
                                 const int64_t *d_row_offsets, size_t total_rows, const int32_t *d_slots, size_t pool_streams,
                                 float *d_pool, float *d_out, void *stream)
{
    return launch_stft_stream_packed(cfg, ss::OUT_STFT, d_x, n_active, d_sample_offsets, d_row_offsets, total_rows, d_slots, pool_streams,
                                     d_pool, d_out, static_cast<hipStream_t>(stream));
}

int ss_mel_spectrogram_stream_packed(const ss_config *cfg, const float *x, size_t n_active, const int64_t *sample_offsets,
                                     const int32_t *slots, size_t pool_streams, float *pool, float *out)
{
    return stft_stream_packed_host(cfg, ss::OUT_MEL, x, n_active, sample_offsets, slots, pool_streams, pool, out);
}

int ss_stft_stream_packed(const ss_config *cfg, const float *x, size_t n_active, const int64_t *sample_offsets, const int32_t *slots,
                          size_t pool_streams, float *pool, float *out)
{
    return stft_stream_packed_host(cfg, ss::OUT_STFT, x, n_active, sample_offsets, slots, pool_streams, pool, out);
}

int ss_preemphasis_device(const float *d_x, size_t n_samples, long shift, float cof, float *d_y, void *stream)
{
    if (!d_x || !d_y) return ss::fail(SS_ERR_ARG, "null buffer");
    // slices s![..shift] / s![-shift..] panic for shift <= 0 or shift > len (processing.rs:43-50)
    if (n_samples == 0 || shift <= 0 || static_cast<size_t>(shift) > n_samples) return ss::fail(SS_ERR_ARG, "shift must be in [1, n_samples]");
    hipError_t e = ss::launch_preemphasis(d_x, d_y, n_samples, static_cast<size_t>(shift) % n_samples, cof,
                                          static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return hip_fail(e, "launch_preemphasis");
    g_last_kernel = "ss_preemphasis_kernel";
    return SS_OK;
}

// ---- host-pointer variants -------------------------------------------------------------------

int ss_mfcc_batch(const ss_config *cfg, const float *x, size_t batch, size_t n_samples, size_t ld, float *out)
{
    if (!cfg || !x || !out) return ss::fail(SS_ERR_ARG, "null argument");
    if (ld < n_samples) return ss::fail(SS_ERR_ARG, "leading dimension smaller than n_samples");
    size_t T = 0;
    int rc = ss::num_frames(cfg->host.params, n_samples, T);
    if (rc) return rc;
    if (batch == 0) return SS_OK;
    rc = check_device(cfg);
    if (rc) return rc;
    return host_pipeline(cfg, x, batch, n_samples, ld, out, T * cfg->host.params.num_cepstral, nullptr, 0,
                         [&](const float *d_x, size_t c, float *d_o0, float *, hipStream_t st) {
                             return ss_mfcc_batch_device(cfg, d_x, c, n_samples, ld, d_o0, st);
                         });
}

int ss_mfcc(const ss_config *cfg, const float *x, size_t n_samples, float *out)
{
    return ss_mfcc_batch(cfg, x, 1, n_samples, n_samples, out);
}

int ss_mfe_batch(const ss_config *cfg, const float *x, size_t batch, size_t n_samples, size_t ld, float *feat, float *energy)
{
    if (!cfg || !x || !feat || !energy) return ss::fail(SS_ERR_ARG, "null argument");
    if (ld < n_samples) return ss::fail(SS_ERR_ARG, "leading dimension smaller than n_samples");
    size_t T = 0;
    int rc = ss::num_frames(cfg->host.params, n_samples, T);
    if (rc) return rc;
    if (batch == 0) return SS_OK;
    rc = check_device(cfg);
    if (rc) return rc;
    return host_pipeline(cfg, x, batch, n_samples, ld, feat, T * cfg->host.params.num_filters, energy, T,
                         [&](const float *d_x, size_t c, float *d_o0, float *d_o1, hipStream_t st) {
                             return ss_mfe_batch_device(cfg, d_x, c, n_samples, ld, d_o0, d_o1, st);
                         });
}

int ss_mfe(const ss_config *cfg, const float *x, size_t n_samples, float *feat, float *energy)
{
    return ss_mfe_batch(cfg, x, 1, n_samples, n_samples, feat, energy);
}

// the same two from int16 host buffers: the samples cross the link as int16 (host_pipeline<int16_t>) and the device call converts
int ss_mfcc_batch_i16(const ss_config *cfg, const int16_t *x, size_t batch, size_t n_samples, size_t ld, float scale, float *out)
{
    if (!cfg || !x || !out) return ss::fail(SS_ERR_ARG, "null argument");
    int rc = check_pcm_scale(scale);
    if (rc) return rc;
    if (ld < n_samples) return ss::fail(SS_ERR_ARG, "leading dimension smaller than n_samples");
    size_t T = 0;
    rc = ss::num_frames(cfg->host.params, n_samples, T);
    if (rc) return rc;
    if (batch == 0) return SS_OK;
    rc = check_device(cfg);
    if (rc) return rc;
    return host_pipeline(cfg, x, batch, n_samples, ld, out, T * cfg->host.params.num_cepstral, nullptr, 0,
                         [&](const int16_t *d_x, size_t c, float *d_o0, float *, hipStream_t st) {
                             return ss_mfcc_batch_i16_device(cfg, d_x, c, n_samples, ld, scale, d_o0, st);
                         });
}

int ss_mfe_batch_i16(const ss_config *cfg, const int16_t *x, size_t batch, size_t n_samples, size_t ld, float scale, float *feat,
                     float *energy)
{
    if (!cfg || !x || !feat || !energy) return ss::fail(SS_ERR_ARG, "null argument");
    int rc = check_pcm_scale(scale);
    if (rc) return rc;
    if (ld < n_samples) return ss::fail(SS_ERR_ARG, "leading dimension smaller than n_samples");
    size_t T = 0;
    rc = ss::num_frames(cfg->host.params, n_samples, T);
    if (rc) return rc;
    if (batch == 0) return SS_OK;
    rc = check_device(cfg);
    if (rc) return rc;
    return host_pipeline(cfg, x, batch, n_samples, ld, feat, T * cfg->host.params.num_filters, energy, T,
                         [&](const int16_t *d_x, size_t c, float *d_o0, float *d_o1, hipStream_t st) {
                             return ss_mfe_batch_i16_device(cfg, d_x, c, n_samples, ld, scale, d_o0, d_o1, st);
                         });
}

int ss_mel_spectrogram(const ss_config *cfg, const float *x, size_t channels, size_t n_samples, float *out)
{
    return stft_host(cfg, ss::OUT_MEL, x, channels, n_samples, 1.0f, out);
}

int ss_mel_spectrogram_i16(const ss_config *cfg, const int16_t *x, size_t channels, size_t n_samples, float scale, float *out)
{
    return stft_host(cfg, ss::OUT_MEL, x, channels, n_samples, scale, out);
}

// ---- log-mel spectrogram: the mel calls with librosa's power_to_db, per clip, in the kernels' epilogue (speechsauce_amd.h) ----
int ss_log_mel_spectrogram_device(const ss_config *cfg, const float *d_x, size_t channels, size_t n_samples, size_t ld, float ref, float amin,
                                  float top_db, float *d_out, void *stream)
{
    return log_mel_dense(cfg, d_x, nullptr, channels, n_samples, ld, DbCall{ref, amin, top_db}, d_out, static_cast<hipStream_t>(stream));
}

int ss_log_mel_spectrogram_i16_device(const ss_config *cfg, const int16_t *d_x, size_t channels, size_t n_samples, size_t ld, float scale,
                                      float ref, float amin, float top_db, float *d_out, void *stream)
{
    const ss::BatchPcmArgs pcm{d_x, scale};
    return log_mel_dense(cfg, nullptr, &pcm, channels, n_samples, ld, DbCall{ref, amin, top_db}, d_out, static_cast<hipStream_t>(stream));
}

int ss_log_mel_spectrogram_packed_device(const ss_config *cfg, const float *d_x, size_t n_clips, const int64_t *d_sample_offsets,
                                         const int64_t *d_row_offsets, size_t total_rows, float ref, float amin, float top_db, float *d_out,
                                         void *stream)
{
    return log_mel_packed(cfg, d_x, n_clips, d_sample_offsets, d_row_offsets, total_rows, DbCall{ref, amin, top_db}, d_out,
                          static_cast<hipStream_t>(stream));
}

int ss_log_mel_spectrogram_packed_i16_device(const ss_config *cfg, const int16_t *d_x, size_t n_clips, const int64_t *d_sample_offsets, float scale,
                                             const int64_t *d_row_offsets, size_t total_rows, float ref, float amin, float top_db, float *d_out,
                                             void *stream)
{
    return log_mel_packed(cfg, PoolChunks(d_x, scale), n_clips, d_sample_offsets, d_row_offsets, total_rows, DbCall{ref, amin, top_db}, d_out,
                          static_cast<hipStream_t>(stream));
}

int ss_log_mel_spectrogram(const ss_config *cfg, const float *x, size_t channels, size_t n_samples, float ref, float amin, float top_db, float *out)
{
    const DbCall c{ref, amin, top_db};
    return stft_host(cfg, ss::OUT_MEL, x, channels, n_samples, 1.0f, out, &c);
}

int ss_log_mel_spectrogram_i16(const ss_config *cfg, const int16_t *x, size_t channels, size_t n_samples, float scale, float ref, float amin,
                               float top_db, float *out)
{
    const DbCall c{ref, amin, top_db};
    return stft_host(cfg, ss::OUT_MEL, x, channels, n_samples, scale, out, &c);
}

int ss_log_mel_spectrogram_packed(const ss_config *cfg, const float *x, size_t n_clips, const int64_t *sample_offsets, float ref, float amin,
                                  float top_db, float *out)
{
    const DbCall c{ref, amin, top_db};
    return packed_stft_host(cfg, ss::OUT_MEL, x, n_clips, sample_offsets, out, &c);
}

int ss_log_mel_spectrogram_packed_i16(const ss_config *cfg, const int16_t *x, size_t n_clips, const int64_t *sample_offsets, float scale, float ref,
                                      float amin, float top_db, float *out)
{
    const DbCall c{ref, amin, top_db};
    return packed_stft_host(cfg, ss::OUT_MEL, PoolChunks(x, scale), n_clips, sample_offsets, out, &c);
}

int ss_preemphasis(const float *x, size_t n_samples, long shift, float cof, float *y)
{
    if (!x || !y) return ss::fail(SS_ERR_ARG, "null argument");
    if (n_samples == 0 || shift <= 0 || static_cast<size_t>(shift) > n_samples) return ss::fail(SS_ERR_ARG, "shift must be in [1, n_samples]");
    if (!ss::have_device()) return ss::no_device("hot path");
    DeviceBuf dx, dy;
    int rc;
    if ((rc = dx.alloc(n_samples * sizeof(float))) || (rc = dy.alloc(n_samples * sizeof(float)))) return rc;
    SS_HIP(hipMemcpy(dx.p, x, n_samples * sizeof(float), hipMemcpyHostToDevice));
    rc = ss_preemphasis_device(dx.as<float>(), n_samples, shift, cof, dy.as<float>(), nullptr);
    if (rc) return rc;
    SS_HIP(hipMemcpy(y, dy.p, n_samples * sizeof(float), hipMemcpyDeviceToHost));
    return SS_OK;
}

// ---- diagnostics ---------------------------------------------------------------------------

const char *ss_last_kernel_name(void) { return g_last_kernel; }

// ---- test aids (include/speechsauce_amd_debug.h): exported by the LAB library only ----
#if SS_LAB
int ss_debug_force_generic(int on)
{
    g_force_generic.store(on ? 1 : 0, std::memory_order_relaxed);
    return SS_OK;
}

int ss_debug_mel_tile(int mode)
{
    // stored: 0 automatic, 1 eight waves + direct stores, 2 eight-wave builds only (tile when the batch allows), 3 twelve waves
    if (mode < 0 || mode > 3) return ss::fail(SS_ERR_ARG, "ss_debug_mel_tile: mode must be 0 .. 3");
    g_mel_tile_off.store(mode == 0 ? 1 : (mode == 1 ? 0 : mode), std::memory_order_relaxed);
    return SS_OK;
}

int ss_debug_tile_fault(int on)
{
    g_tile_fault.store(on ? 1u : 0u, std::memory_order_relaxed);
    return SS_OK;
}

int ss_debug_stamp_buffer(unsigned long long *d_stamps)
{
    g_stamp_buffer.store(d_stamps, std::memory_order_relaxed);
    return SS_OK;
}

int ss_debug_poison_lds(void *stream)
{
    int dev = 0, cus = 0;
    SS_HIP(hipGetDevice(&dev));
    SS_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    hipError_t e = ss::launch_poison_lds(static_cast<hipStream_t>(stream), cus);
    if (e != hipSuccess) return hip_fail(e, "launch_poison_lds");
    return SS_OK;
}
#endif  // SS_LAB

// Shader clock the part held during launches of the MFCC batch kernel: `launches` launches on `stream`, each with the kernel's
// per-wave stamps switched on (a wave writes its lifetime in shader cycles, s_memtime, and on the constant 100 MHz clock,
// s_memrealtime, once, as it ends), into a buffer this call owns; the mean of cycles / lifetime over the waves of the last
// launch.  A per-call diagnostic: nothing process-wide is touched, launches of other threads are not affected.  The stamps
// exist in the 512-point kernel only: SS_ERR_UNSUPPORTED for configurations that run on another kernel.
int ss_mfcc_shader_clock(const ss_config *cfg, const float *d_x, size_t batch, size_t n_samples, size_t ld, float *d_out,
                         void *stream, int launches, float *ghz)
{
    if (!cfg || !ghz || launches <= 0) return ss::fail(SS_ERR_ARG, "bad clock request");
    *ghz = 0.f;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t nwaves = static_cast<size_t>(cfg->num_cus) * 16, words = nwaves * 6;
    DeviceBuf db;
    int rc = db.alloc(words * sizeof(unsigned long long));
    if (rc) return rc;
    SS_HIP(hipMemsetAsync(db.p, 0, words * sizeof(unsigned long long), s));
    g_call_stamps = db.as<unsigned long long>();
    for (int i = 0; i < launches && rc == SS_OK; ++i) rc = ss_mfcc_batch_device(cfg, d_x, batch, n_samples, ld, d_out, stream);
    g_call_stamps = nullptr;
    const bool stamped = std::strncmp(g_last_kernel, "ss_mfcc_c256<", 13) == 0;
    const hipError_t es = hipStreamSynchronize(s);
    if (rc) return rc;
    if (es != hipSuccess) return hip_fail(es, "hipStreamSynchronize");
    if (!stamped) return ss::fail(SS_ERR_UNSUPPORTED, "the shader-clock stamps exist in the 512-point MFCC kernel only");
    std::vector<unsigned long long> w(words);
    SS_HIP(hipMemcpy(w.data(), db.p, words * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    double sum = 0.0;
    size_t n = 0;
    for (size_t k = 0; k < nwaves; ++k) {
        const unsigned long long t0 = w[6 * k], t1 = w[6 * k + 2], cyc = w[6 * k + 5];
        if (t1 <= t0 || (cyc >> 40) != 1) continue;  // waves that did not run / the two table waves of a workgroup (they report something else)
        sum += static_cast<double>(cyc & ((1ull << 40) - 1)) / (static_cast<double>(t1 - t0) * 10.0);  // cycles per ns
        ++n;
    }
    if (n == 0) return ss::fail(SS_ERR_DEVICE, "no wave reported its lifetime");
    *ghz = static_cast<float>(sum / static_cast<double>(n));
    return SS_OK;
}

extern "C++" {  // (a template: C++ linkage inside the extern "C" block)
namespace {
// Sums of the per-wave stamps of a timed region's launches: sums[0] += shader cycles lived, sums[1] += 100 MHz ticks lived,
// sums[2] += waves counted.  `slots` launches, each with `slot_words` words of records for `nwaves` waves.  Format 0 (512-point
// MFCC kernel): six words per wave -- start / end on the 100 MHz clock in words 0 / 2, cycles lived flagged 1 in bits 40..41 of
// word 5 (the two table waves of a workgroup report something else there and are skipped).  Format 1 (twelve-wave 4096-point MFCC
// and 2048-point mel builds): two words per wave -- cycles lived, ticks lived.  Records of waves that never ran are zero.
static __global__ __launch_bounds__(256) void stamp_sums_kernel(const unsigned long long *w, unsigned long long slots, unsigned long long slot_words,
                                                                unsigned long long nwaves, int format, unsigned long long *sums)
{
    unsigned long long cyc = 0, ticks = 0, cnt = 0;
    const unsigned long long n = slots * nwaves;
    for (unsigned long long k = static_cast<unsigned long long>(blockIdx.x) * blockDim.x + threadIdx.x; k < n;
         k += static_cast<unsigned long long>(gridDim.x) * blockDim.x) {
        const unsigned long long *r = w + (k / nwaves) * slot_words + (k % nwaves) * (format == 0 ? 6ull : 2ull);
        if (format == 0) {
            const unsigned long long t0 = r[0], t1 = r[2], c = r[5];
            if (t1 <= t0 || (c >> 40) != 1) continue;
            cyc += c & ((1ull << 40) - 1);
            ticks += t1 - t0;
        } else {
            if (r[1] == 0) continue;
            cyc += r[0];
            ticks += r[1];
        }
        ++cnt;
    }
    for (int m = 32; m > 0; m >>= 1) {
        cyc += __shfl_xor(cyc, m, 64);
        ticks += __shfl_xor(ticks, m, 64);
        cnt += __shfl_xor(cnt, m, 64);
    }
    if ((threadIdx.x & 63) == 0 && cnt) {
        atomicAdd(&sums[0], cyc);
        atomicAdd(&sums[1], ticks);
        atomicAdd(&sums[2], cnt);
    }
}

// The timed region behind ss_mfcc_timed_region / ss_mel_spectrogram_timed_region: `launches` launches through `launch(i)` on
// `stream` between two HIP events, the per-wave stamps of the last `stamped` of them kept (each launch in a slot of its own of a
// buffer this call owns) and summed on the device.
template <typename Launch>
int timed_region(const ss_config *cfg, void *stream, int launches, int stamped, float *avg_ms, float *ghz, float *wall_ms, Launch launch)
{
    *avg_ms = 0.f;
    *ghz = 0.f;
    if (wall_ms) *wall_ms = 0.f;
    if (stamped > launches) stamped = launches;
    if (stamped > 4096) stamped = 4096;  // 196 KB of wave records per stamped launch
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t nwaves = static_cast<size_t>(cfg->num_cus) * 16, words = nwaves * 6;
    DeviceBuf db;
    int rc = db.alloc(std::max<size_t>(1, static_cast<size_t>(stamped)) * words * sizeof(unsigned long long));
    if (rc) return rc;
    if (stamped) SS_HIP(hipMemsetAsync(db.p, 0, static_cast<size_t>(stamped) * words * sizeof(unsigned long long), s));
    hipEvent_t e0, e1;
    SS_HIP(hipEventCreate(&e0));
    {
        const hipError_t ec = hipEventCreate(&e1);
        if (ec != hipSuccess) {
            (void)hipEventDestroy(e0);
            return hip_fail(ec, "hipEventCreate");
        }
    }
    {
        const hipError_t es = hipStreamSynchronize(s);  // the region starts on an idle stream (the memset above is not part of it)
        if (es != hipSuccess) {
            (void)hipEventDestroy(e0);
            (void)hipEventDestroy(e1);
            return hip_fail(es, "hipStreamSynchronize");
        }
    }
    const auto w0 = std::chrono::steady_clock::now();
    (void)hipEventRecord(e0, s);
    int format = -1;  // which record format the stamped launches wrote (-2: a kernel without stamps, or not always the same one)
    for (int i = 0; i < launches && rc == SS_OK; ++i) {
        const int slot = i - (launches - stamped);
        g_call_stamps = g_call_stamps2 = slot >= 0 ? db.as<unsigned long long>() + static_cast<size_t>(slot) * words : nullptr;
        rc = launch(i);
        if (slot >= 0) {
            const int f = std::strncmp(g_last_kernel, "ss_mfcc_c256<", 13) == 0 ? 0
                          : (std::strncmp(g_last_kernel, "ss_mfcc_c2048<exact,mel8321,w12>", 32) == 0 || std::strncmp(g_last_kernel, "ss_mel_c1024<w12", 16) == 0) ? 1 : -2;
            format = (format == -1 || format == f) ? f : -2;
        }
    }
    g_call_stamps = g_call_stamps2 = nullptr;
    (void)hipEventRecord(e1, s);
    hipError_t e = hipSuccess;
    while ((e = hipEventQuery(e1)) == hipErrorNotReady) {  // polled: a blocking wait's wake-up latency is several launches long
    }
    if (wall_ms) *wall_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - w0).count();
    float ms = 0.f;
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    if (rc) return rc;
    if (e != hipSuccess) return hip_fail(e, "event timing");
    *avg_ms = ms / static_cast<float>(launches);
    if (stamped == 0) return SS_OK;
    if (format < 0) return ss::fail(SS_ERR_UNSUPPORTED, "the wave stamps exist in the 512-point MFCC kernel and in the twelve-wave builds of the 4096-point MFCC and 2048-point mel kernels only");
    // the records are summed on the device (1000 stamped launches are 196 MB of them): three words come back
    DeviceBuf sums;
    rc = sums.alloc(3 * sizeof(unsigned long long));
    if (rc) return rc;
    SS_HIP(hipMemsetAsync(sums.p, 0, 3 * sizeof(unsigned long long), s));
    hipLaunchKernelGGL(stamp_sums_kernel, dim3(1024), dim3(256), 0, s, db.as<unsigned long long>(), static_cast<unsigned long long>(stamped),
                       static_cast<unsigned long long>(words), static_cast<unsigned long long>(nwaves), format, sums.as<unsigned long long>());
    SS_HIP(hipGetLastError());
    unsigned long long hs[3] = {0, 0, 0};
    SS_HIP(hipMemcpyAsync(hs, sums.p, sizeof hs, hipMemcpyDeviceToHost, s));
    SS_HIP(hipStreamSynchronize(s));
    if (hs[1] == 0 || hs[2] == 0) return ss::fail(SS_ERR_DEVICE, "no wave reported its lifetime");
    *ghz = static_cast<float>(static_cast<double>(hs[0]) / (static_cast<double>(hs[1]) * 10.0));  // cycles per ns
    return SS_OK;
}
}  // namespace
}  // extern "C++"

// A timed region whose duration AND shader clock come from the same launches: `launches` launches of the MFCC batch kernel on
// `stream`, launch i reading d_x[i % n_x] and writing d_out[i % n_out] (a ring of inputs larger than the Infinity Cache keeps the
// samples coming from HBM), HIP events on `stream` around all of them, and the per-wave stamps of the LAST `stamped` launches kept,
// each launch in a slot of its own of a buffer this call owns.  *avg_ms = region / launches; *ghz = sum of the waves' shader
// cycles / sum of their lifetimes on the 100 MHz clock over every stamped launch.
int ss_mfcc_timed_region(const ss_config *cfg, const float *const *d_x, size_t n_x, size_t batch, size_t n_samples, size_t ld,
                         float *const *d_out, size_t n_out, void *stream, int launches, int stamped, float *avg_ms, float *ghz,
                         float *wall_ms)
{
    if (!cfg || !d_x || !d_out || n_x == 0 || n_out == 0 || launches <= 0 || stamped < 0 || !avg_ms || !ghz)
        return ss::fail(SS_ERR_ARG, "bad timed-region request");
    return timed_region(cfg, stream, launches, stamped, avg_ms, ghz, wall_ms, [&](int i) {
        return ss_mfcc_batch_device(cfg, d_x[static_cast<size_t>(i) % n_x], batch, n_samples, ld, d_out[static_cast<size_t>(i) % n_out], stream);
    });
}

// the same for the mel-spectrogram path (2048-point kernel, twelve-wave builds)
int ss_mel_spectrogram_timed_region(const ss_config *cfg, const float *const *d_x, size_t n_x, size_t channels, size_t n_samples, size_t ld,
                                    float *const *d_out, size_t n_out, void *stream, int launches, int stamped, float *avg_ms, float *ghz,
                                    float *wall_ms)
{
    if (!cfg || !d_x || !d_out || n_x == 0 || n_out == 0 || launches <= 0 || stamped < 0 || !avg_ms || !ghz)
        return ss::fail(SS_ERR_ARG, "bad timed-region request");
    return timed_region(cfg, stream, launches, stamped, avg_ms, ghz, wall_ms, [&](int i) {
        return ss_mel_spectrogram_device(cfg, d_x[static_cast<size_t>(i) % n_x], channels, n_samples, ld, d_out[static_cast<size_t>(i) % n_out], stream);
    });
}

namespace {
// One wave: shader cycles (s_memtime) against the constant 100 MHz counter (s_memrealtime) over about `ticks` of the latter,
// asleep in between (s_sleep: no issue slots, no memory traffic -- the workload beside it is not disturbed).  A lead-in of a
// tenth of the interval (at most 200 us) is slept through first and not counted: a probe launched just ahead of the load it is
// meant to watch does not average the idle clock of those first microseconds in.
static __global__ __launch_bounds__(64) void clock_probe_kernel(unsigned long long *out, unsigned ticks)
{
    if (threadIdx.x != 0) return;
    const unsigned lead = ticks / 10u < 20000u ? ticks / 10u : 20000u;
    unsigned long long t = __builtin_amdgcn_s_memrealtime();
    const unsigned long long tl = t;
    while (t - tl < lead) {
        __builtin_amdgcn_s_sleep(64);
        t = __builtin_amdgcn_s_memrealtime();
    }
    const unsigned long long c0 = __builtin_amdgcn_s_memtime();
    const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
    t = t0;
    while (t - t0 < ticks) {
        __builtin_amdgcn_s_sleep(64);
        t = __builtin_amdgcn_s_memrealtime();
    }
    const unsigned long long c1 = __builtin_amdgcn_s_memtime();
    const unsigned long long t1 = __builtin_amdgcn_s_memrealtime();
    out[0] = c1 - c0;
    out[1] = t1 - t0;
}
}  // namespace

int ss_shader_clock_probe_async(void *stream, uint32_t micros, unsigned long long *d_words)
{
    if (!d_words || micros < 10 || micros > 1000000) return ss::fail(SS_ERR_ARG, "bad clock probe request");
    hipLaunchKernelGGL(clock_probe_kernel, dim3(1), dim3(64), 0, static_cast<hipStream_t>(stream), d_words, micros * 100u);
    SS_HIP(hipGetLastError());
    return SS_OK;
}

int ss_shader_clock_probe(void *stream, uint32_t micros, float *ghz)
{
    if (!ghz || micros < 10 || micros > 1000000) return ss::fail(SS_ERR_ARG, "bad clock probe request");
    *ghz = 0.f;
    hipStream_t s = static_cast<hipStream_t>(stream);
    DeviceBuf db;
    int rc = db.alloc(2 * sizeof(unsigned long long));
    if (rc) return rc;
    SS_HIP(hipMemsetAsync(db.p, 0, 2 * sizeof(unsigned long long), s));
    hipLaunchKernelGGL(clock_probe_kernel, dim3(1), dim3(64), 0, s, db.as<unsigned long long>(), micros * 100u);
    SS_HIP(hipGetLastError());
    unsigned long long w[2] = {0, 0};
    SS_HIP(hipMemcpyAsync(w, db.p, sizeof w, hipMemcpyDeviceToHost, s));
    SS_HIP(hipStreamSynchronize(s));
    if (w[1] == 0) return ss::fail(SS_ERR_DEVICE, "the clock probe reported nothing");
    *ghz = static_cast<float>(static_cast<double>(w[0]) / (static_cast<double>(w[1]) * 10.0));  // cycles per ns
    return SS_OK;
}

int ss_time_mfcc_batch_device(const ss_config *cfg, const float *d_x, size_t batch, size_t n_samples, size_t ld,
                              float *d_out, void *stream, int iters, float *avg_ms)
{
    if (!avg_ms || iters <= 0) return ss::fail(SS_ERR_ARG, "bad timing request");
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipEvent_t e0, e1;
    SS_HIP(hipEventCreate(&e0));
    {
        const hipError_t ec = hipEventCreate(&e1);
        if (ec != hipSuccess) {
            (void)hipEventDestroy(e0);
            return hip_fail(ec, "hipEventCreate");
        }
    }
    int rc = ss_mfcc_batch_device(cfg, d_x, batch, n_samples, ld, d_out, stream);  // warm-up
    if (rc == SS_OK) {
        (void)hipEventRecord(e0, s);
        for (int i = 0; i < iters && rc == SS_OK; ++i) rc = ss_mfcc_batch_device(cfg, d_x, batch, n_samples, ld, d_out, stream);
        (void)hipEventRecord(e1, s);
        hipError_t e = hipEventSynchronize(e1);
        float ms = 0.f;
        if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
        if (e != hipSuccess) rc = hip_fail(e, "event timing");
        *avg_ms = ms / static_cast<float>(iters);
    }
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    return rc;
}

int ss_time_mel_spectrogram_device(const ss_config *cfg, const float *d_x, size_t channels, size_t n_samples,
                                   size_t ld, float *d_out, void *stream, int iters, float *avg_ms)
{
    if (!avg_ms || iters <= 0) return ss::fail(SS_ERR_ARG, "bad timing request");
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipEvent_t e0, e1;
    SS_HIP(hipEventCreate(&e0));
    {
        const hipError_t ec = hipEventCreate(&e1);
        if (ec != hipSuccess) {
            (void)hipEventDestroy(e0);
            return hip_fail(ec, "hipEventCreate");
        }
    }
    int rc = ss_mel_spectrogram_device(cfg, d_x, channels, n_samples, ld, d_out, stream);
    if (rc == SS_OK) {
        (void)hipEventRecord(e0, s);
        for (int i = 0; i < iters && rc == SS_OK; ++i) rc = ss_mel_spectrogram_device(cfg, d_x, channels, n_samples, ld, d_out, stream);
        (void)hipEventRecord(e1, s);
        hipError_t e = hipEventSynchronize(e1);
        float ms = 0.f;
        if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
        if (e != hipSuccess) rc = hip_fail(e, "event timing");
        *avg_ms = ms / static_cast<float>(iters);
    }
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    return rc;
}

}  // extern "C"

// ---- Kaldi-compatible fbank / MFCC front end (ss_kaldi_*; kernel: ss_kaldi512.hip) ------------------------------------------
// The handle: the validated parameters, the kernel's table block on the device it was created on, and a pinned device error word
// of its own (the packed calls' containment, as ss_config's).  Immutable after creation.
struct ss_kaldi_config {
    ss_kaldi_params params{};
    ss::KaldiTables tabs;
    int device = -1;
    int num_cus = 256;
    float *d_tab = nullptr;
    unsigned *h_err = nullptr, *d_err = nullptr;
};

namespace {

int kaldi_pending_error(const ss_kaldi_config *cfg)
{
    if (!cfg->h_err || __atomic_load_n(cfg->h_err, __ATOMIC_ACQUIRE) == 0) return SS_OK;
    const unsigned w = __atomic_exchange_n(cfg->h_err, 0u, __ATOMIC_ACQ_REL);
    if (w == 0) return SS_OK;
    return ss::fail(SS_ERR_DEVICE, "a kernel launched on this handle skipped a packed clip whose offsets are inconsistent (error word " +
                                       std::to_string(w) + "): the rows of that clip were left untouched");
}

int kaldi_ready(const ss_kaldi_config *cfg)
{
    int dev = -1;
    SS_HIP(hipGetDevice(&dev));
    if (dev != cfg->device) return ss::fail(SS_ERR_ARG, "the handle was created on a different HIP device than the current one");
    return kaldi_pending_error(cfg);
}

// the handle's part of the kernel's argument block
ss::KaldiArgs kaldi_args(const ss_kaldi_config *cfg, bool mfcc, const float *x, float *out, float *log_energy)
{
    const ss_kaldi_params &p = cfg->params;
    ss::KaldiArgs a{};
    a.x = x;
    a.flen = cfg->tabs.s.flen;
    a.step = cfg->tabs.s.shift;
    a.tab = cfg->d_tab;
    a.mel_wpitch = cfg->tabs.wpitch;
    std::copy(cfg->tabs.q4, cfg->tabs.q4 + 5, a.mel_q4);
    a.n_filters = p.num_mel_bins;
    a.n_ceps = p.num_ceps;
    a.input_scale = p.input_scale;
    a.preemph = p.preemph_coef;
    a.flen_f = static_cast<float>(cfg->tabs.s.flen);
    a.log_floor = p.energy_floor > 0.0f ? std::log(p.energy_floor) : -INFINITY;
    a.remove_dc = p.remove_dc_offset != 0;
    a.raw_energy = p.raw_energy != 0;
    a.use_energy = p.use_energy != 0;
    a.out_mfcc = mfcc;
    a.use_power = p.use_power != 0;
    a.out = out;
    a.out_energy = mfcc ? nullptr : log_energy;
    return a;
}

int kaldi_launched(hipError_t e, const ss::LaunchInfo &info)
{
    if (e != hipSuccess) return hip_fail(e, "launch_kaldi_c256");
    g_last_kernel = info.kernel_name;
    return SS_OK;
}

int kaldi_check_call(const ss_kaldi_config *cfg, bool mfcc)
{
    if (!cfg) return ss::fail(SS_ERR_ARG, "null handle");
    if (mfcc && cfg->params.num_ceps == 0) return ss::fail(SS_ERR_ARG, "the handle was created with num_ceps = 0: it serves the fbank calls only");
    return SS_OK;
}

// the 16-bit PCM samples of an ss_kpcm_* call: the scale, first among the data checks, and 2-byte alignment
int kaldi_check_pcm(const PoolChunks &x)
{
    if (!x.is_pcm) return SS_OK;
    if (int rc = check_pcm_scale(x.scale)) return rc;
    if (reinterpret_cast<uintptr_t>(x.pcm) & 1u) return ss::fail(SS_ERR_ARG, "the PCM buffer must be 2-byte aligned");
    return SS_OK;
}

// equal-length clips; T: the rows per clip.  x: floats, or 16-bit PCM (ss_kpcm_*)
int kaldi_check_dense(const ss_kaldi_config *cfg, bool mfcc, const PoolChunks &x, size_t batch, size_t n_samples, size_t ld, const float *out, size_t &T)
{
    if (int rc = kaldi_check_call(cfg, mfcc)) return rc;
    if (int rc = kaldi_check_pcm(x)) return rc;
    if (!x.ptr() || !out) return ss::fail(SS_ERR_ARG, "null buffer");
    if (ld < n_samples) return ss::fail(SS_ERR_ARG, "leading dimension smaller than n_samples");
    if (n_samples >= (1ull << 31) || batch >= (1ull << 31)) return ss::fail(SS_ERR_ARG, "batch and n_samples must be below 2^31");
    T = ss::kaldi_frames(cfg->tabs.s, n_samples);
    if (T == 0) return ss::fail(SS_ERR_SHORT_SIGNAL, "signal shorter than one frame");
    if (static_cast<unsigned long long>(batch) * T + 8 >= 0xffffffffull) return ss::fail(SS_ERR_ARG, "batch * frames must be below 2^32 - 8");
    return SS_OK;
}

int kaldi_dense_device(const ss_kaldi_config *cfg, bool mfcc, const PoolChunks &d_x, size_t batch, size_t n_samples, size_t ld, float *d_out,
                       float *d_log_energy, hipStream_t stream)
{
    if (batch == 0) return cfg ? kaldi_check_pcm(d_x) : ss::fail(SS_ERR_ARG, "null handle");
    size_t T = 0;
    if (int rc = kaldi_check_dense(cfg, mfcc, d_x, batch, n_samples, ld, d_out, T)) return rc;
    if (int rc = kaldi_ready(cfg)) return rc;
    ss::KaldiArgs a = kaldi_args(cfg, mfcc, d_x.f, d_out, d_log_energy);
    a.ld = ld;
    a.n_samples = static_cast<uint32_t>(n_samples);
    a.batch = static_cast<uint32_t>(batch);
    a.n_frames = static_cast<uint32_t>(T);
    ss::LaunchInfo info{};
    if (d_x.is_pcm) return kaldi_launched(ss::launch_kaldi_c256(a, ss::KaldiPcmArgs{d_x.pcm, d_x.scale}, stream, cfg->num_cus, &info), info);
    return kaldi_launched(ss::launch_kaldi_c256(a, stream, cfg->num_cus, &info), info);
}

// (PCM crosses the link as int16)
int kaldi_dense_host(const ss_kaldi_config *cfg, bool mfcc, const PoolChunks &x, size_t batch, size_t n_samples, size_t ld, float *out, float *log_energy)
{
    if (batch == 0) return cfg ? kaldi_check_pcm(x) : ss::fail(SS_ERR_ARG, "null handle");
    size_t T = 0;
    int rc = kaldi_check_dense(cfg, mfcc, x, batch, n_samples, ld, out, T);
    if (rc) return rc;
    if (!ss::have_device()) return ss::no_device("hot path");
    const size_t cols = mfcc ? cfg->params.num_ceps : cfg->params.num_mel_bins, rows = batch * T;
    ss::HostStage st("ss_kaldi");
    const size_t sb = x.sample_bytes();
    void *d_in = st.room<void>(batch * n_samples * sb);
    float *d_out = st.room<float>(rows * cols * sizeof(float));
    float *d_en = log_energy ? st.room<float>(rows * sizeof(float)) : nullptr;
    st.up_rows(d_in, x.ptr(), ld * sb, n_samples * sb, batch);
    if (st.ok())
        st.ran(kaldi_dense_device(cfg, mfcc,
                                  x.is_pcm ? PoolChunks(static_cast<const int16_t *>(d_in), x.scale) : PoolChunks(static_cast<const float *>(d_in)), batch,
                                  n_samples, n_samples, d_out, d_en, nullptr));
    st.sync();
    st.down(out, d_out, rows * cols * sizeof(float));
    if (log_energy) st.down(log_energy, d_en, rows * sizeof(float));
    return st.status();
}

int kaldi_packed_device(const ss_kaldi_config *cfg, bool mfcc, const PoolChunks &d_x, size_t n_clips, const int64_t *d_so, const int64_t *d_fo,
                        size_t total_frames, float *d_out, float *d_log_energy, hipStream_t stream)
{
    if (int rc = kaldi_check_call(cfg, mfcc)) return rc;
    if (int rc = kaldi_check_pcm(d_x)) return rc;
    if (n_clips == 0) return SS_OK;
    if (!d_x.ptr() || !d_so || !d_fo || !d_out) return ss::fail(SS_ERR_ARG, "null buffer");
    if (n_clips >= (1ull << 31)) return ss::fail(SS_ERR_ARG, "n_clips must be below 2^31");
    if (static_cast<unsigned long long>(total_frames) + 8 >= 0xffffffffull) return ss::fail(SS_ERR_ARG, "total_frames must be below 2^32 - 8");
    if (int rc = kaldi_ready(cfg)) return rc;
    if (total_frames == 0) return SS_OK;  // no clip can own a row
    const ss::KaldiArgs a = kaldi_args(cfg, mfcc, d_x.f, d_out, d_log_energy);
    ss::KaldiVarlenArgs v{};
    v.so = reinterpret_cast<const long long *>(d_so);
    v.fo = reinterpret_cast<const long long *>(d_fo);
    v.total_frames = total_frames;
    v.n_clips = static_cast<uint32_t>(n_clips);
    v.err = cfg->d_err;
    ss::LaunchInfo info{};
    if (d_x.is_pcm) return kaldi_launched(ss::launch_kaldi_c256_varlen(a, ss::KaldiVarlenPcmArgs{v, d_x.pcm, d_x.scale}, stream, cfg->num_cus, &info), info);
    return kaldi_launched(ss::launch_kaldi_c256_varlen(a, v, stream, cfg->num_cus, &info), info);
}

int kaldi_packed_host(const ss_kaldi_config *cfg, bool mfcc, const PoolChunks &x, size_t n_clips, const int64_t *so, float *out, float *log_energy)
{
    if (int rc = kaldi_check_call(cfg, mfcc)) return rc;
    if (x.is_pcm)
        if (int rc = check_pcm_scale(x.scale)) return rc;
    if (n_clips == 0) return SS_OK;
    if (!x.ptr() || !so || !out) return ss::fail(SS_ERR_ARG, "null buffer");
    if (n_clips >= (1ull << 31)) return ss::fail(SS_ERR_ARG, "n_clips must be below 2^31");
    std::vector<int64_t> fo(n_clips + 1);
    int rc = ss_kaldi_packed_frame_offsets(&cfg->params, n_clips, so, fo.data());
    if (rc) return rc;
    const size_t total_in = static_cast<size_t>(so[n_clips]), rows = static_cast<size_t>(fo[n_clips]);
    const size_t cols = mfcc ? cfg->params.num_ceps : cfg->params.num_mel_bins, tbytes = (n_clips + 1) * sizeof(int64_t);
    if (!ss::have_device()) return ss::no_device("hot path");
    ss::HostStage st("ss_kaldi");
    const void *d_in = st.up(x.ptr(), total_in * x.sample_bytes());
    float *d_out = st.room<float>(rows * cols * sizeof(float));
    float *d_en = log_energy ? st.room<float>(rows * sizeof(float)) : nullptr;
    const int64_t *d_so = st.up(so, tbytes), *d_fo = st.up(fo.data(), tbytes);
    if (st.ok())
        st.ran(kaldi_packed_device(cfg, mfcc,
                                   x.is_pcm ? PoolChunks(static_cast<const int16_t *>(d_in), x.scale) : PoolChunks(static_cast<const float *>(d_in)),
                                   n_clips, d_so, d_fo, rows, d_out, d_en, nullptr));
    st.sync();
    if (st.ok()) st.ran(kaldi_pending_error(cfg));
    st.down(out, d_out, rows * cols * sizeof(float));
    if (log_energy) st.down(log_energy, d_en, rows * sizeof(float));
    return st.status();
}

// Ragged streaming fbank / MFCC over a pool of stream states (ss_kstream_*_packed*_device): the rows of n_active entries of different
// hop counts, each over the pool row its slot names, then the advance of the named rows -- a linear chain of two kernels on `stream`
// (none for the advance where S == 0), the pool build of ss_kaldi_c256 and the frame pool's ss_stream_advance_packed over one entry
// block (state_len = S, step = shift).  The tables are device arrays read by the kernels only; the grids come from n_active and
// total_rows.  x: the packed chunks, floats or 16-bit PCM.
int kaldi_pool_device(const ss_kaldi_config *cfg, bool mfcc, const PoolChunks &x, size_t n_active, const int64_t *d_so, const int64_t *d_ro,
                      size_t total_rows, const int32_t *d_slots, size_t pool_streams, float *d_pool, float *d_out, float *d_log_energy,
                      hipStream_t stream)
{
    if (int rc = kaldi_check_call(cfg, mfcc)) return rc;
    if (n_active == 0) return SS_OK;
    size_t S = 0, D = 0;
    if (int rc = ss_kstream_state_len(&cfg->params, &S, &D)) return rc;
    if (!x.ptr() || !d_so || !d_ro || !d_slots || !d_out || (S > 0 && !d_pool)) return ss::fail(SS_ERR_ARG, "null buffer");
    if (x.is_pcm) {
        if (int rc = check_pcm_scale(x.scale)) return rc;
        if (reinterpret_cast<uintptr_t>(x.pcm) & 1u) return ss::fail(SS_ERR_ARG, "the PCM buffer must be 2-byte aligned");
    }
    if (n_active >= 0x80000000ull || pool_streams >= 0x80000000ull || total_rows >= 0x80000000ull)
        return ss::fail(SS_ERR_ARG, "n_active, pool_streams and total_rows must be below 2^31");
    if (pool_streams == 0) return ss::fail(SS_ERR_ARG, "the pool has no rows");
    const size_t cols = mfcc ? cfg->params.num_ceps : cfg->params.num_mel_bins;
    const size_t pbytes = pool_streams * S * sizeof(float);
    if (S > 0 && (ranges_overlap(d_pool, pbytes, d_out, total_rows * cols * sizeof(float)) ||
                  (!mfcc && d_log_energy && ranges_overlap(d_pool, pbytes, d_log_energy, total_rows * sizeof(float)))))
        return ss::fail(SS_ERR_ARG, "the pool overlaps an output");
    if (int rc = kaldi_ready(cfg)) return rc;
    const ss::KaldiArgs a = kaldi_args(cfg, mfcc, x.f, d_out, d_log_energy);
    ss::FrameStreamPackedPcmArgs sp{};
    sp.e.pool = d_pool;
    sp.e.state_len = static_cast<uint32_t>(S);
    sp.e.lead = static_cast<int32_t>(S);
    sp.e.so = reinterpret_cast<const long long *>(d_so);
    sp.e.ro = reinterpret_cast<const long long *>(d_ro);
    sp.e.slots = d_slots;
    sp.e.n_active = static_cast<uint32_t>(n_active);
    sp.e.pool_streams = static_cast<uint32_t>(pool_streams);
    sp.e.total_rows = static_cast<uint32_t>(total_rows);
    sp.e.step = a.step;
    sp.e.err = cfg->d_err;
    sp.x = x.pcm;
    sp.scale = x.scale;
    ss::LaunchInfo info{};
    if (int rc = kaldi_launched(ss::launch_kaldi_c256_stream_packed(a, sp, x.is_pcm, stream, cfg->num_cus, &info), info)) return rc;
    const hipError_t e = x.is_pcm ? ss::launch_stream_advance_packed(sp, stream) : ss::launch_stream_advance_packed(sp.e, x.f, stream);
    if (e != hipSuccess) return hip_fail(e, "launch_stream_advance_packed");
    return SS_OK;
}

// Host-pointer form, as frame_stream_packed_host: the tables are checked here, before anything touches the device; then x, the
// tables and the n_active named pool rows (a compact block whose row i is entry i's: the device call runs on slots 0 .. n_active - 1)
// go up, the outputs and the named rows come down.  The caller's pool is written only once everything before it succeeded.
int kaldi_pool_host(const ss_kaldi_config *cfg, bool mfcc, const PoolChunks &x, size_t n_active, const int64_t *so, const int32_t *slots,
                    size_t pool_streams, float *pool, float *out, float *log_energy)
{
    if (int rc = kaldi_check_call(cfg, mfcc)) return rc;
    if (n_active == 0) return SS_OK;
    size_t S = 0, D = 0;
    int rc = ss_kstream_state_len(&cfg->params, &S, &D);
    if (rc) return rc;
    if (!x.ptr() || !so || !slots || !out || (S > 0 && !pool)) return ss::fail(SS_ERR_ARG, "null buffer");
    if (x.is_pcm && (rc = check_pcm_scale(x.scale))) return rc;
    if (n_active >= 0x80000000ull || pool_streams >= 0x80000000ull)
        return ss::fail(SS_ERR_ARG, "n_active, pool_streams and total_rows must be below 2^31");
    if (pool_streams == 0) return ss::fail(SS_ERR_ARG, "the pool has no rows");
    std::vector<int64_t> ro(n_active + 1);
    if ((rc = ss_kstream_row_offsets(&cfg->params, n_active, so, ro.data()))) return rc;
    if ((rc = ss::check_slots(slots, n_active, pool_streams))) return rc;
    const size_t rows = static_cast<size_t>(ro[n_active]), samples = static_cast<size_t>(so[n_active]);
    if (rows >= 0x80000000ull) return ss::fail(SS_ERR_ARG, "n_active, pool_streams and total_rows must be below 2^31");
    const size_t cols = mfcc ? cfg->params.num_ceps : cfg->params.num_mel_bins;
    const size_t pbytes = pool_streams * S * sizeof(float);
    if (S > 0 && (ranges_overlap(pool, pbytes, x.ptr(), samples * x.sample_bytes()) || ranges_overlap(pool, pbytes, out, rows * cols * sizeof(float)) ||
                  (log_energy && ranges_overlap(pool, pbytes, log_energy, rows * sizeof(float)))))
        return ss::fail(SS_ERR_ARG, "the pool overlaps the input or an output");
    if (!ss::have_device()) return ss::no_device("hot path");
    ss::PoolRows named;  // the named pool rows, row i = entry i's
    named.gather(pool, slots, n_active, S);
    const size_t tbytes = (n_active + 1) * sizeof(int64_t);
    ss::HostStage st("ss_kstream");
    const void *dx = st.up(x.ptr(), samples * x.sample_bytes());
    const int64_t *dso = st.up(so, tbytes), *dro = st.up(ro.data(), tbytes);
    const auto d_named = st.up_pool(named);  // no rows where the pool has no state (S == 0)
    float *d0 = st.room<float>(rows * cols * sizeof(float));
    float *d1 = log_energy ? st.room<float>(rows * sizeof(float)) : nullptr;
    if (st.ok())
        st.ran(kaldi_pool_device(cfg, mfcc,
                                 x.is_pcm ? PoolChunks(static_cast<const int16_t *>(dx), x.scale) : PoolChunks(static_cast<const float *>(dx)),
                                 n_active, dso, dro, rows, d_named.slots, n_active, d_named.rows, d0, d1, nullptr));
    st.sync();
    if (st.ok()) st.ran(kaldi_pending_error(cfg));
    st.down(out, d0, rows * cols * sizeof(float));
    if (log_energy) st.down(log_energy, d1, rows * sizeof(float));
    st.down_pool(named, d_named, " (pool rows)");
    st.scatter(named, pool, slots);
    return st.status();
}

}  // namespace

extern "C" {

int ss_kaldi_config_create(const ss_kaldi_params *p, ss_kaldi_config **out)
{
    if (!p || !out) return ss::fail(SS_ERR_ARG, "null argument");
    *out = nullptr;
    if (int rc = ss::kaldi_validate(*p, nullptr)) return rc;
    std::unique_ptr<ss_kaldi_config> cfg(new ss_kaldi_config());
    cfg->params = *p;
    ss::build_kaldi512(*p, cfg->tabs);
    if (!cfg->tabs.ok) return ss::fail(SS_ERR_UNSUPPORTED, "the mel bank does not fit the kernel's five filter slots per lane");
    if (!ss::have_device()) return ss::no_device("hot path");
    SS_HIP(hipGetDevice(&cfg->device));
    hipDeviceProp_t prop;
    SS_HIP(hipGetDeviceProperties(&prop, cfg->device));
    cfg->num_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    if (int rc = upload(&cfg->d_tab, cfg->tabs.tab.data(), cfg->tabs.tab.size() * sizeof(float))) {
        ss_kaldi_config_destroy(cfg.release());
        return rc;
    }
    void *hp = nullptr, *dp = nullptr;
    hipError_t e = hipHostMalloc(&hp, 64, hipHostMallocMapped);
    if (e == hipSuccess) e = hipHostGetDevicePointer(&dp, hp, 0);
    if (e != hipSuccess) {
        if (hp) (void)hipHostFree(hp);
        ss_kaldi_config_destroy(cfg.release());
        return hip_fail(e, "hipHostMalloc (device error word)");
    }
    std::memset(hp, 0, 64);
    cfg->h_err = static_cast<unsigned *>(hp);
    cfg->d_err = static_cast<unsigned *>(dp);
    *out = cfg.release();
    return SS_OK;
}

void ss_kaldi_config_destroy(ss_kaldi_config *cfg)
{
    if (!cfg) return;
    if (cfg->d_tab) (void)hipFree(cfg->d_tab);
    if (cfg->h_err) (void)hipHostFree(cfg->h_err);
    delete cfg;
}

int ss_kaldi_config_params(const ss_kaldi_config *cfg, ss_kaldi_params *out)
{
    if (!cfg || !out) return ss::fail(SS_ERR_ARG, "null argument");
    *out = cfg->params;
    return SS_OK;
}

int ss_kaldi_config_device_status(const ss_kaldi_config *cfg)
{
    if (!cfg) return ss::fail(SS_ERR_ARG, "null handle");
    return kaldi_pending_error(cfg);
}

int ss_kaldi_fbank_device(const ss_kaldi_config *cfg, const float *d_x, size_t batch, size_t n_samples, size_t ld, float *d_out,
                          float *d_log_energy, void *stream)
{
    return kaldi_dense_device(cfg, false, d_x, batch, n_samples, ld, d_out, d_log_energy, static_cast<hipStream_t>(stream));
}

int ss_kaldi_fbank(const ss_kaldi_config *cfg, const float *x, size_t batch, size_t n_samples, size_t ld, float *out, float *log_energy)
{
    return kaldi_dense_host(cfg, false, x, batch, n_samples, ld, out, log_energy);
}

int ss_kaldi_mfcc_device(const ss_kaldi_config *cfg, const float *d_x, size_t batch, size_t n_samples, size_t ld, float *d_out, void *stream)
{
    return kaldi_dense_device(cfg, true, d_x, batch, n_samples, ld, d_out, nullptr, static_cast<hipStream_t>(stream));
}

int ss_kaldi_mfcc(const ss_kaldi_config *cfg, const float *x, size_t batch, size_t n_samples, size_t ld, float *out)
{
    return kaldi_dense_host(cfg, true, x, batch, n_samples, ld, out, nullptr);
}

int ss_kaldi_fbank_packed_device(const ss_kaldi_config *cfg, const float *d_x, size_t n_clips, const int64_t *d_sample_offsets,
                                 const int64_t *d_frame_offsets, size_t total_frames, float *d_out, float *d_log_energy, void *stream)
{
    return kaldi_packed_device(cfg, false, d_x, n_clips, d_sample_offsets, d_frame_offsets, total_frames, d_out, d_log_energy,
                               static_cast<hipStream_t>(stream));
}

int ss_kaldi_fbank_packed(const ss_kaldi_config *cfg, const float *x, size_t n_clips, const int64_t *sample_offsets, float *out,
                          float *log_energy)
{
    return kaldi_packed_host(cfg, false, x, n_clips, sample_offsets, out, log_energy);
}

int ss_kaldi_mfcc_packed_device(const ss_kaldi_config *cfg, const float *d_x, size_t n_clips, const int64_t *d_sample_offsets,
                                const int64_t *d_frame_offsets, size_t total_frames, float *d_out, void *stream)
{
    return kaldi_packed_device(cfg, true, d_x, n_clips, d_sample_offsets, d_frame_offsets, total_frames, d_out, nullptr,
                               static_cast<hipStream_t>(stream));
}

int ss_kaldi_mfcc_packed(const ss_kaldi_config *cfg, const float *x, size_t n_clips, const int64_t *sample_offsets, float *out)
{
    return kaldi_packed_host(cfg, true, x, n_clips, sample_offsets, out, nullptr);
}

// 16-bit PCM forms of the eight calls above (sample k is (float)x[k] * scale): the PCM builds of the same kernel
int ss_kpcm_fbank_device(const ss_kaldi_config *cfg, const int16_t *d_x, size_t batch, size_t n_samples, size_t ld, float scale, float *d_out,
                         float *d_log_energy, void *stream)
{
    return kaldi_dense_device(cfg, false, PoolChunks(d_x, scale), batch, n_samples, ld, d_out, d_log_energy, static_cast<hipStream_t>(stream));
}

int ss_kpcm_fbank(const ss_kaldi_config *cfg, const int16_t *x, size_t batch, size_t n_samples, size_t ld, float scale, float *out, float *log_energy)
{
    return kaldi_dense_host(cfg, false, PoolChunks(x, scale), batch, n_samples, ld, out, log_energy);
}

int ss_kpcm_mfcc_device(const ss_kaldi_config *cfg, const int16_t *d_x, size_t batch, size_t n_samples, size_t ld, float scale, float *d_out, void *stream)
{
    return kaldi_dense_device(cfg, true, PoolChunks(d_x, scale), batch, n_samples, ld, d_out, nullptr, static_cast<hipStream_t>(stream));
}

int ss_kpcm_mfcc(const ss_kaldi_config *cfg, const int16_t *x, size_t batch, size_t n_samples, size_t ld, float scale, float *out)
{
    return kaldi_dense_host(cfg, true, PoolChunks(x, scale), batch, n_samples, ld, out, nullptr);
}

int ss_kpcm_fbank_packed_device(const ss_kaldi_config *cfg, const int16_t *d_x, size_t n_clips, const int64_t *d_sample_offsets, float scale,
                                const int64_t *d_frame_offsets, size_t total_frames, float *d_out, float *d_log_energy, void *stream)
{
    return kaldi_packed_device(cfg, false, PoolChunks(d_x, scale), n_clips, d_sample_offsets, d_frame_offsets, total_frames, d_out, d_log_energy,
                               static_cast<hipStream_t>(stream));
}

int ss_kpcm_fbank_packed(const ss_kaldi_config *cfg, const int16_t *x, size_t n_clips, const int64_t *sample_offsets, float scale, float *out,
                         float *log_energy)
{
    return kaldi_packed_host(cfg, false, PoolChunks(x, scale), n_clips, sample_offsets, out, log_energy);
}

int ss_kpcm_mfcc_packed_device(const ss_kaldi_config *cfg, const int16_t *d_x, size_t n_clips, const int64_t *d_sample_offsets, float scale,
                               const int64_t *d_frame_offsets, size_t total_frames, float *d_out, void *stream)
{
    return kaldi_packed_device(cfg, true, PoolChunks(d_x, scale), n_clips, d_sample_offsets, d_frame_offsets, total_frames, d_out, nullptr,
                               static_cast<hipStream_t>(stream));
}

int ss_kpcm_mfcc_packed(const ss_kaldi_config *cfg, const int16_t *x, size_t n_clips, const int64_t *sample_offsets, float scale, float *out)
{
    return kaldi_packed_host(cfg, true, PoolChunks(x, scale), n_clips, sample_offsets, out, nullptr);
}

int ss_kstream_fbank_packed_device(const ss_kaldi_config *cfg, const float *d_x, size_t n_active, const int64_t *d_sample_offsets,
                                   const int64_t *d_row_offsets, size_t total_rows, const int32_t *d_slots, size_t pool_streams, float *d_pool,
                                   float *d_out, float *d_log_energy, void *stream)
{
    return kaldi_pool_device(cfg, false, PoolChunks(d_x), n_active, d_sample_offsets, d_row_offsets, total_rows, d_slots, pool_streams, d_pool, d_out,
                             d_log_energy, static_cast<hipStream_t>(stream));
}

int ss_kstream_mfcc_packed_device(const ss_kaldi_config *cfg, const float *d_x, size_t n_active, const int64_t *d_sample_offsets,
                                  const int64_t *d_row_offsets, size_t total_rows, const int32_t *d_slots, size_t pool_streams, float *d_pool,
                                  float *d_out, void *stream)
{
    return kaldi_pool_device(cfg, true, PoolChunks(d_x), n_active, d_sample_offsets, d_row_offsets, total_rows, d_slots, pool_streams, d_pool, d_out,
                             nullptr, static_cast<hipStream_t>(stream));
}

int ss_kstream_fbank_packed_i16_device(const ss_kaldi_config *cfg, const int16_t *d_x, size_t n_active, const int64_t *d_sample_offsets,
                                       const int64_t *d_row_offsets, size_t total_rows, const int32_t *d_slots, size_t pool_streams, float scale,
                                       float *d_pool, float *d_out, float *d_log_energy, void *stream)
{
    return kaldi_pool_device(cfg, false, PoolChunks(d_x, scale), n_active, d_sample_offsets, d_row_offsets, total_rows, d_slots, pool_streams, d_pool,
                             d_out, d_log_energy, static_cast<hipStream_t>(stream));
}

int ss_kstream_mfcc_packed_i16_device(const ss_kaldi_config *cfg, const int16_t *d_x, size_t n_active, const int64_t *d_sample_offsets,
                                      const int64_t *d_row_offsets, size_t total_rows, const int32_t *d_slots, size_t pool_streams, float scale,
                                      float *d_pool, float *d_out, void *stream)
{
    return kaldi_pool_device(cfg, true, PoolChunks(d_x, scale), n_active, d_sample_offsets, d_row_offsets, total_rows, d_slots, pool_streams, d_pool,
                             d_out, nullptr, static_cast<hipStream_t>(stream));
}

int ss_kstream_fbank_packed(const ss_kaldi_config *cfg, const float *x, size_t n_active, const int64_t *sample_offsets, const int32_t *slots,
                            size_t pool_streams, float *pool, float *out, float *log_energy)
{
    return kaldi_pool_host(cfg, false, PoolChunks(x), n_active, sample_offsets, slots, pool_streams, pool, out, log_energy);
}

int ss_kstream_mfcc_packed(const ss_kaldi_config *cfg, const float *x, size_t n_active, const int64_t *sample_offsets, const int32_t *slots,
                           size_t pool_streams, float *pool, float *out)
{
    return kaldi_pool_host(cfg, true, PoolChunks(x), n_active, sample_offsets, slots, pool_streams, pool, out, nullptr);
}

int ss_kstream_fbank_packed_i16(const ss_kaldi_config *cfg, const int16_t *x, size_t n_active, const int64_t *sample_offsets, const int32_t *slots,
                                size_t pool_streams, float scale, float *pool, float *out, float *log_energy)
{
    return kaldi_pool_host(cfg, false, PoolChunks(x, scale), n_active, sample_offsets, slots, pool_streams, pool, out, log_energy);
}

int ss_kstream_mfcc_packed_i16(const ss_kaldi_config *cfg, const int16_t *x, size_t n_active, const int64_t *sample_offsets, const int32_t *slots,
                               size_t pool_streams, float scale, float *pool, float *out)
{
    return kaldi_pool_host(cfg, true, PoolChunks(x, scale), n_active, sample_offsets, slots, pool_streams, pool, out, nullptr);
}

}  // extern "C"

// ---- NeMo / Parakeet log-mel front end (ss_nemo_*; kernels: ss_nemo512.hip) --------------------------------------------------
// The handle, as ss_kaldi_config: the validated parameters, the kernel's table block on the device it was created on, and a pinned
// device error word of its own.  Immutable after creation.
struct ss_nemo_config {
    ss_nemo_params params{};
    ss::NemoTables tabs;
    int device = -1;
    int num_cus = 256;
    float *d_tab = nullptr;
    unsigned *h_err = nullptr, *d_err = nullptr;
};

namespace {

int nemo_pending_error(const ss_nemo_config *cfg)
{
    if (!cfg->h_err || __atomic_load_n(cfg->h_err, __ATOMIC_ACQUIRE) == 0) return SS_OK;
    const unsigned w = __atomic_exchange_n(cfg->h_err, 0u, __ATOMIC_ACQ_REL);
    if (w == 0) return SS_OK;
    return ss::fail(SS_ERR_DEVICE, "a kernel launched on this handle skipped a packed clip whose offsets are inconsistent (error word " +
                                       std::to_string(w) + "): the rows of that clip were left untouched");
}

int nemo_ready(const ss_nemo_config *cfg)
{
    int dev = -1;
    SS_HIP(hipGetDevice(&dev));
    if (dev != cfg->device) return ss::fail(SS_ERR_ARG, "the handle was created on a different HIP device than the current one");
    return nemo_pending_error(cfg);
}

// the handle's part of the kernels' argument block
ss::NemoArgs nemo_args(const ss_nemo_config *cfg, const float *x, float *out)
{
    const ss_nemo_params &p = cfg->params;
    ss::NemoArgs a{};
    a.x = x;
    a.win_len = p.win_length;
    a.tab = cfg->d_tab;
    a.mel_wpitch = cfg->tabs.wpitch;
    std::copy(cfg->tabs.q4, cfg->tabs.q4 + ss::nemo512_layout::kSlots, a.mel_q4);
    a.n_mels = p.n_mels;
    a.preemph = p.preemph;
    a.log_guard = p.log_guard;
    a.norm_eps = p.norm_eps;
    a.out = out;
    return a;
}

// the rows, then (per-feature normalisation) step 8 in place on them: one or two launches on `stream`
int nemo_launch(const ss_nemo_config *cfg, const ss::NemoArgs &a, const ss::NemoVarlenArgs *v, hipStream_t stream)
{
    ss::LaunchInfo info{};
    const hipError_t e = v ? ss::launch_nemo_c256_varlen(a, *v, stream, cfg->num_cus, &info) : ss::launch_nemo_c256(a, stream, cfg->num_cus, &info);
    if (e != hipSuccess) return hip_fail(e, "launch_nemo_c256");
    g_last_kernel = info.kernel_name;
    if (cfg->params.normalize == SS_NEMO_NORM_PER_FEATURE) {
        const hipError_t n = ss::launch_nemo_norm(a, v, stream);
        if (n != hipSuccess) return hip_fail(n, "launch_nemo_norm");
    }
    return SS_OK;
}

// equal-length clips; T: the rows per clip (0: nothing to do)
int nemo_check_dense(const ss_nemo_config *cfg, const float *x, size_t n_samples, size_t batch, size_t ld, const float *out, size_t &T)
{
    if (!cfg) return ss::fail(SS_ERR_ARG, "null handle");
    if (!x || !out) return ss::fail(SS_ERR_ARG, "null buffer");
    if (ld < n_samples) return ss::fail(SS_ERR_ARG, "leading dimension smaller than n_samples");
    if (n_samples >= (1ull << 31) || batch >= (1ull << 31)) return ss::fail(SS_ERR_ARG, "batch and n_samples must be below 2^31");
    T = n_samples / ss::kNemoHop;
    if (static_cast<unsigned long long>(batch) * T + 8 >= 0xffffffffull) return ss::fail(SS_ERR_ARG, "batch * frames must be below 2^32 - 8");
    return SS_OK;
}

int nemo_dense_device(const ss_nemo_config *cfg, const float *d_x, size_t batch, size_t n_samples, size_t ld, float *d_out, hipStream_t stream)
{
    if (batch == 0) return cfg ? SS_OK : ss::fail(SS_ERR_ARG, "null handle");
    size_t T = 0;
    if (int rc = nemo_check_dense(cfg, d_x, n_samples, batch, ld, d_out, T)) return rc;
    if (int rc = nemo_ready(cfg)) return rc;
    if (T == 0) return SS_OK;  // clips shorter than one hop have no rows
    ss::NemoArgs a = nemo_args(cfg, d_x, d_out);
    a.ld = ld;
    a.n_samples = static_cast<uint32_t>(n_samples);
    a.batch = static_cast<uint32_t>(batch);
    a.n_frames = static_cast<uint32_t>(T);
    return nemo_launch(cfg, a, nullptr, stream);
}

int nemo_packed_device(const ss_nemo_config *cfg, const float *d_x, size_t n_clips, const int64_t *d_so, const int64_t *d_fo, size_t total_frames,
                       float *d_out, hipStream_t stream)
{
    if (!cfg) return ss::fail(SS_ERR_ARG, "null handle");
    if (n_clips == 0) return SS_OK;
    if (!d_x || !d_so || !d_fo || !d_out) return ss::fail(SS_ERR_ARG, "null buffer");
    if (n_clips >= (1ull << 31)) return ss::fail(SS_ERR_ARG, "n_clips must be below 2^31");
    if (static_cast<unsigned long long>(total_frames) + 8 >= 0xffffffffull) return ss::fail(SS_ERR_ARG, "total_frames must be below 2^32 - 8");
    if (int rc = nemo_ready(cfg)) return rc;
    if (total_frames == 0) return SS_OK;  // no clip can own a row
    const ss::NemoArgs a = nemo_args(cfg, d_x, d_out);
    ss::NemoVarlenArgs v{};
    v.so = reinterpret_cast<const long long *>(d_so);
    v.fo = reinterpret_cast<const long long *>(d_fo);
    v.total_frames = total_frames;
    v.n_clips = static_cast<uint32_t>(n_clips);
    v.err = cfg->d_err;
    return nemo_launch(cfg, a, &v, stream);
}

// ---- ss_nstream_*: the same front end over a pool of stream states (kernels: ss_nemo512_pool.hip) ----
// what every ss_nstream_* call on a handle checks first; S and L are the handle's pool sizes
int nstream_check_call(const ss_nemo_config *cfg, size_t &S, size_t &L)
{
    if (!cfg) return ss::fail(SS_ERR_ARG, "null handle");
    if (cfg->params.normalize != SS_NEMO_NORM_NONE)
        return ss::fail(SS_ERR_UNSUPPORTED, "per-feature normalisation needs a clip's statistics: a stream has none (chain ss_cmvn_* behind the pool)");
    return ss_nstream_state_len(&cfg->params, &S, &L);
}

// Ragged streaming log-mel over a pool of stream states (ss_nstream_log_mel_packed*_device): the rows of n_active entries of different
// hop counts, each over the pool row its slot names, then the advance of the named rows -- a linear chain of two kernels on `stream`,
// the pool build of ss_nemo_c256 and the frame pool's ss_stream_advance_packed over one entry block (state_len = S, step = 160,
// lead = S - 1).  The tables are device arrays read by the kernels only; the grids come from n_active and total_rows.  x: the packed
// chunks, floats or 16-bit PCM.
int nemo_pool_device(const ss_nemo_config *cfg, const PoolChunks &x, size_t n_active, const int64_t *d_so, const int64_t *d_ro, size_t total_rows,
                     const int32_t *d_slots, size_t pool_streams, float *d_pool, float *d_out, hipStream_t stream)
{
    size_t S = 0, L = 0;
    if (int rc = nstream_check_call(cfg, S, L)) return rc;
    if (n_active == 0) return SS_OK;
    if (!x.ptr() || !d_so || !d_ro || !d_slots || !d_out || !d_pool) return ss::fail(SS_ERR_ARG, "null buffer");
    if (x.is_pcm) {
        if (int rc = check_pcm_scale(x.scale)) return rc;
        if (reinterpret_cast<uintptr_t>(x.pcm) & 1u) return ss::fail(SS_ERR_ARG, "the PCM buffer must be 2-byte aligned");
    }
    if (n_active >= 0x80000000ull || pool_streams >= 0x80000000ull || total_rows >= 0x80000000ull)
        return ss::fail(SS_ERR_ARG, "n_active, pool_streams and total_rows must be below 2^31");
    if (pool_streams == 0) return ss::fail(SS_ERR_ARG, "the pool has no rows");
    if (ranges_overlap(d_pool, pool_streams * S * sizeof(float), d_out, total_rows * cfg->params.n_mels * sizeof(float)))
        return ss::fail(SS_ERR_ARG, "the pool overlaps an output");
    if (int rc = nemo_ready(cfg)) return rc;
    const ss::NemoArgs a = nemo_args(cfg, x.f, d_out);
    ss::FrameStreamPackedPcmArgs sp{};
    sp.e.pool = d_pool;
    sp.e.state_len = static_cast<uint32_t>(S);
    sp.e.lead = static_cast<int32_t>(S - 1);
    sp.e.so = reinterpret_cast<const long long *>(d_so);
    sp.e.ro = reinterpret_cast<const long long *>(d_ro);
    sp.e.slots = d_slots;
    sp.e.n_active = static_cast<uint32_t>(n_active);
    sp.e.pool_streams = static_cast<uint32_t>(pool_streams);
    sp.e.total_rows = static_cast<uint32_t>(total_rows);
    sp.e.step = ss::kNemoHop;
    sp.e.err = cfg->d_err;
    sp.x = x.pcm;
    sp.scale = x.scale;
    ss::LaunchInfo info{};
    hipError_t e = ss::launch_nemo_c256_stream_packed(a, sp, x.is_pcm, stream, cfg->num_cus, &info);
    if (e != hipSuccess) return hip_fail(e, "launch_nemo_c256_stream_packed");
    g_last_kernel = info.kernel_name;
    e = x.is_pcm ? ss::launch_stream_advance_packed(sp, stream) : ss::launch_stream_advance_packed(sp.e, x.f, stream);
    if (e != hipSuccess) return hip_fail(e, "launch_stream_advance_packed");
    return SS_OK;
}

// Host-pointer form, as kaldi_pool_host: the tables are checked here, before anything touches the device; then x, the tables and the
// n_active named pool rows (a compact block whose row i is entry i's) go up, the output and the named rows come down.  The caller's
// pool is written only once everything before it succeeded.
int nemo_pool_host(const ss_nemo_config *cfg, const PoolChunks &x, size_t n_active, const int64_t *so, const int32_t *slots, size_t pool_streams,
                   float *pool, float *out)
{
    size_t S = 0, L = 0;
    int rc = nstream_check_call(cfg, S, L);
    if (rc) return rc;
    if (n_active == 0) return SS_OK;
    if (!x.ptr() || !so || !slots || !out || !pool) return ss::fail(SS_ERR_ARG, "null buffer");
    if (x.is_pcm && (rc = check_pcm_scale(x.scale))) return rc;
    if (n_active >= 0x80000000ull || pool_streams >= 0x80000000ull)
        return ss::fail(SS_ERR_ARG, "n_active, pool_streams and total_rows must be below 2^31");
    if (pool_streams == 0) return ss::fail(SS_ERR_ARG, "the pool has no rows");
    std::vector<int64_t> ro(n_active + 1);
    if ((rc = ss_nstream_row_offsets(&cfg->params, n_active, so, ro.data()))) return rc;
    if ((rc = ss::check_slots(slots, n_active, pool_streams))) return rc;
    const size_t rows = static_cast<size_t>(ro[n_active]), samples = static_cast<size_t>(so[n_active]);
    if (rows >= 0x80000000ull) return ss::fail(SS_ERR_ARG, "n_active, pool_streams and total_rows must be below 2^31");
    const size_t obytes = rows * cfg->params.n_mels * sizeof(float), pbytes = pool_streams * S * sizeof(float);
    if (ranges_overlap(pool, pbytes, x.ptr(), samples * x.sample_bytes()) || ranges_overlap(pool, pbytes, out, obytes))
        return ss::fail(SS_ERR_ARG, "the pool overlaps the input or an output");
    if (!ss::have_device()) return ss::no_device("hot path");
    ss::PoolRows named;  // the named pool rows, row i = entry i's
    named.gather(pool, slots, n_active, S);
    const size_t tbytes = (n_active + 1) * sizeof(int64_t);
    ss::HostStage st("ss_nstream");
    const void *dx = st.up(x.ptr(), samples * x.sample_bytes());
    const int64_t *dso = st.up(so, tbytes), *dro = st.up(ro.data(), tbytes);
    const auto d_named = st.up_pool(named);
    float *d0 = st.room<float>(obytes);
    if (st.ok())
        st.ran(nemo_pool_device(cfg, x.is_pcm ? PoolChunks(static_cast<const int16_t *>(dx), x.scale) : PoolChunks(static_cast<const float *>(dx)),
                                n_active, dso, dro, rows, d_named.slots, n_active, d_named.rows, d0, nullptr));
    st.sync();
    if (st.ok()) st.ran(nemo_pending_error(cfg));
    st.down(out, d0, obytes);
    st.down_pool(named, d_named, " (pool rows)");
    st.scatter(named, pool, slots);
    return st.status();
}

// The flush: the L rows of every named stream (one launch, none where L == 0), then the zeroing of the named pool rows
int nemo_flush_device(const ss_nemo_config *cfg, size_t n_active, const int32_t *d_slots, size_t pool_streams, float *d_pool, float *d_out,
                      hipStream_t stream)
{
    size_t S = 0, L = 0;
    if (int rc = nstream_check_call(cfg, S, L)) return rc;
    if (n_active == 0) return SS_OK;
    if (!d_slots || !d_pool || (L > 0 && !d_out)) return ss::fail(SS_ERR_ARG, "null buffer");
    if (n_active >= 0x80000000ull || pool_streams >= 0x80000000ull || n_active * L >= 0x80000000ull)
        return ss::fail(SS_ERR_ARG, "n_active, pool_streams and the row count must be below 2^31");
    if (pool_streams == 0) return ss::fail(SS_ERR_ARG, "the pool has no rows");
    if (L > 0 && ranges_overlap(d_pool, pool_streams * S * sizeof(float), d_out, n_active * L * cfg->params.n_mels * sizeof(float)))
        return ss::fail(SS_ERR_ARG, "the pool overlaps an output");
    if (int rc = nemo_ready(cfg)) return rc;
    const ss::NemoArgs a = nemo_args(cfg, nullptr, d_out);
    ss::NemoFlushArgs s{};
    s.pool = d_pool;
    s.state_len = static_cast<uint32_t>(S);
    s.delay = static_cast<uint32_t>(L);
    s.slots = d_slots;
    s.n_active = static_cast<uint32_t>(n_active);
    s.pool_streams = static_cast<uint32_t>(pool_streams);
    s.err = cfg->d_err;
    ss::LaunchInfo info{};
    const hipError_t e = ss::launch_nemo_c256_flush(a, s, stream, cfg->num_cus, &info);
    if (e != hipSuccess) return hip_fail(e, "launch_nemo_c256_flush");
    g_last_kernel = info.kernel_name;
    return SS_OK;
}

int nemo_flush_host(const ss_nemo_config *cfg, size_t n_active, const int32_t *slots, size_t pool_streams, float *pool, float *out)
{
    size_t S = 0, L = 0;
    int rc = nstream_check_call(cfg, S, L);
    if (rc) return rc;
    if (n_active == 0) return SS_OK;
    if (!slots || !pool || (L > 0 && !out)) return ss::fail(SS_ERR_ARG, "null buffer");
    if (n_active >= 0x80000000ull || pool_streams >= 0x80000000ull || n_active * L >= 0x80000000ull)
        return ss::fail(SS_ERR_ARG, "n_active, pool_streams and the row count must be below 2^31");
    if (pool_streams == 0) return ss::fail(SS_ERR_ARG, "the pool has no rows");
    if ((rc = ss::check_slots(slots, n_active, pool_streams))) return rc;
    const size_t obytes = n_active * L * cfg->params.n_mels * sizeof(float);
    if (L > 0 && ranges_overlap(pool, pool_streams * S * sizeof(float), out, obytes)) return ss::fail(SS_ERR_ARG, "the pool overlaps an output");
    if (!ss::have_device()) return ss::no_device("hot path");
    ss::PoolRows named;
    named.gather(pool, slots, n_active, S);
    ss::HostStage st("ss_nstream");
    const auto d_named = st.up_pool(named);
    float *d0 = L > 0 ? st.room<float>(obytes) : nullptr;
    if (st.ok()) st.ran(nemo_flush_device(cfg, n_active, d_named.slots, n_active, d_named.rows, d0, nullptr));
    st.sync();
    if (st.ok()) st.ran(nemo_pending_error(cfg));
    if (L > 0) st.down(out, d0, obytes);
    st.down_pool(named, d_named, " (pool rows)");
    st.scatter(named, pool, slots);
    return st.status();
}

}  // namespace

extern "C" {

int ss_nemo_config_create(const ss_nemo_params *p, ss_nemo_config **out)
{
    if (!p || !out) return ss::fail(SS_ERR_ARG, "null argument");
    *out = nullptr;
    if (int rc = ss::nemo_validate(*p)) return rc;
    std::unique_ptr<ss_nemo_config> cfg(new ss_nemo_config());
    cfg->params = *p;
    ss::build_nemo512(*p, cfg->tabs);
    if (!cfg->tabs.ok) return ss::fail(SS_ERR_UNSUPPORTED, "the mel bank does not fit the kernel's eight filter slots per lane");
    if (!ss::have_device()) return ss::no_device("hot path");
    SS_HIP(hipGetDevice(&cfg->device));
    hipDeviceProp_t prop;
    SS_HIP(hipGetDeviceProperties(&prop, cfg->device));
    cfg->num_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    if (int rc = upload(&cfg->d_tab, cfg->tabs.tab.data(), cfg->tabs.tab.size() * sizeof(float))) {
        ss_nemo_config_destroy(cfg.release());
        return rc;
    }
    void *hp = nullptr, *dp = nullptr;
    hipError_t e = hipHostMalloc(&hp, 64, hipHostMallocMapped);
    if (e == hipSuccess) e = hipHostGetDevicePointer(&dp, hp, 0);
    if (e != hipSuccess) {
        if (hp) (void)hipHostFree(hp);
        ss_nemo_config_destroy(cfg.release());
        return hip_fail(e, "hipHostMalloc (device error word)");
    }
    std::memset(hp, 0, 64);
    cfg->h_err = static_cast<unsigned *>(hp);
    cfg->d_err = static_cast<unsigned *>(dp);
    *out = cfg.release();
    return SS_OK;
}

void ss_nemo_config_destroy(ss_nemo_config *cfg)
{
    if (!cfg) return;
    if (cfg->d_tab) (void)hipFree(cfg->d_tab);
    if (cfg->h_err) (void)hipHostFree(cfg->h_err);
    delete cfg;
}

int ss_nemo_config_params(const ss_nemo_config *cfg, ss_nemo_params *out)
{
    if (!cfg || !out) return ss::fail(SS_ERR_ARG, "null argument");
    *out = cfg->params;
    return SS_OK;
}

int ss_nemo_config_device_status(const ss_nemo_config *cfg)
{
    if (!cfg) return ss::fail(SS_ERR_ARG, "null handle");
    return nemo_pending_error(cfg);
}

int ss_nemo_log_mel_device(const ss_nemo_config *cfg, const float *d_x, size_t batch, size_t n_samples, size_t ld, float *d_out, void *stream)
{
    return nemo_dense_device(cfg, d_x, batch, n_samples, ld, d_out, static_cast<hipStream_t>(stream));
}

int ss_nemo_log_mel(const ss_nemo_config *cfg, const float *x, size_t batch, size_t n_samples, size_t ld, float *out)
{
    if (batch == 0) return cfg ? SS_OK : ss::fail(SS_ERR_ARG, "null handle");
    size_t T = 0;
    if (int rc = nemo_check_dense(cfg, x, n_samples, batch, ld, out, T)) return rc;
    if (T == 0) return SS_OK;
    if (!ss::have_device()) return ss::no_device("hot path");
    const size_t obytes = batch * T * cfg->params.n_mels * sizeof(float);
    ss::HostStage st("ss_nemo");
    float *d_in = st.room<float>(batch * n_samples * sizeof(float));
    float *d_out = st.room<float>(obytes);
    st.up_rows(d_in, x, ld * sizeof(float), n_samples * sizeof(float), batch);
    if (st.ok()) st.ran(nemo_dense_device(cfg, d_in, batch, n_samples, n_samples, d_out, nullptr));
    st.sync();
    st.down(out, d_out, obytes);
    return st.status();
}

int ss_nemo_log_mel_packed_device(const ss_nemo_config *cfg, const float *d_x, size_t n_clips, const int64_t *d_sample_offsets,
                                  const int64_t *d_frame_offsets, size_t total_frames, float *d_out, void *stream)
{
    return nemo_packed_device(cfg, d_x, n_clips, d_sample_offsets, d_frame_offsets, total_frames, d_out, static_cast<hipStream_t>(stream));
}

int ss_nemo_log_mel_packed(const ss_nemo_config *cfg, const float *x, size_t n_clips, const int64_t *sample_offsets, float *out)
{
    if (!cfg) return ss::fail(SS_ERR_ARG, "null handle");
    if (n_clips == 0) return SS_OK;
    if (!x || !sample_offsets || !out) return ss::fail(SS_ERR_ARG, "null buffer");
    if (n_clips >= (1ull << 31)) return ss::fail(SS_ERR_ARG, "n_clips must be below 2^31");
    std::vector<int64_t> fo(n_clips + 1);
    if (int rc = ss_nemo_packed_frame_offsets(&cfg->params, n_clips, sample_offsets, fo.data())) return rc;
    const size_t total_in = static_cast<size_t>(sample_offsets[n_clips]), rows = static_cast<size_t>(fo[n_clips]);
    if (rows == 0) return SS_OK;
    if (!ss::have_device()) return ss::no_device("hot path");
    const size_t obytes = rows * cfg->params.n_mels * sizeof(float), tbytes = (n_clips + 1) * sizeof(int64_t);
    ss::HostStage st("ss_nemo");
    const float *d_in = st.up(x, total_in * sizeof(float));
    float *d_out = st.room<float>(obytes);
    const int64_t *d_so = st.up(sample_offsets, tbytes), *d_fo = st.up(fo.data(), tbytes);
    if (st.ok()) st.ran(nemo_packed_device(cfg, d_in, n_clips, d_so, d_fo, rows, d_out, nullptr));
    st.sync();
    if (st.ok()) st.ran(nemo_pending_error(cfg));
    st.down(out, d_out, obytes);
    return st.status();
}

int ss_nstream_log_mel_packed_device(const ss_nemo_config *cfg, const float *d_x, size_t n_active, const int64_t *d_sample_offsets,
                                     const int64_t *d_row_offsets, size_t total_rows, const int32_t *d_slots, size_t pool_streams, float *d_pool,
                                     float *d_out, void *stream)
{
    return nemo_pool_device(cfg, PoolChunks(d_x), n_active, d_sample_offsets, d_row_offsets, total_rows, d_slots, pool_streams, d_pool, d_out,
                            static_cast<hipStream_t>(stream));
}

int ss_nstream_log_mel_packed(const ss_nemo_config *cfg, const float *x, size_t n_active, const int64_t *sample_offsets, const int32_t *slots,
                              size_t pool_streams, float *pool, float *out)
{
    return nemo_pool_host(cfg, PoolChunks(x), n_active, sample_offsets, slots, pool_streams, pool, out);
}

int ss_nstream_log_mel_packed_i16_device(const ss_nemo_config *cfg, const int16_t *d_x, size_t n_active, const int64_t *d_sample_offsets,
                                         const int64_t *d_row_offsets, size_t total_rows, const int32_t *d_slots, size_t pool_streams, float scale,
                                         float *d_pool, float *d_out, void *stream)
{
    return nemo_pool_device(cfg, PoolChunks(d_x, scale), n_active, d_sample_offsets, d_row_offsets, total_rows, d_slots, pool_streams, d_pool, d_out,
                            static_cast<hipStream_t>(stream));
}

int ss_nstream_log_mel_packed_i16(const ss_nemo_config *cfg, const int16_t *x, size_t n_active, const int64_t *sample_offsets, const int32_t *slots,
                                  size_t pool_streams, float scale, float *pool, float *out)
{
    return nemo_pool_host(cfg, PoolChunks(x, scale), n_active, sample_offsets, slots, pool_streams, pool, out);
}

int ss_nstream_flush_device(const ss_nemo_config *cfg, size_t n_active, const int32_t *d_slots, size_t pool_streams, float *d_pool, float *d_out,
                            void *stream)
{
    return nemo_flush_device(cfg, n_active, d_slots, pool_streams, d_pool, d_out, static_cast<hipStream_t>(stream));
}

int ss_nstream_flush(const ss_nemo_config *cfg, size_t n_active, const int32_t *slots, size_t pool_streams, float *pool, float *out)
{
    return nemo_flush_host(cfg, n_active, slots, pool_streams, pool, out);
}

}  // extern "C"
