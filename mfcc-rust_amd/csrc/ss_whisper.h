// What the host side (ss_host.cpp), the kernels (ss_whisper400.hip) and the tests share of the Whisper log-mel front end
// (ss_whisper_* of include/speechsauce_amd.h, whose comment is the definition): the sizes, the silent-frame rule, the reflected
// sample index, the unit arithmetic of the persistent loop and the layout of the table block.  Plain C++ (no HIP header): the host
// compiler builds it into ss_host.cpp, where ss_whisper_first_silent_frame hands the rule to the tests.
#pragma once

#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define SS_WH_HD __host__ __device__ __forceinline__
#else
#define SS_WH_HD inline
#endif

namespace ss {
namespace whisper {

constexpr uint32_t kSampleRate = 16000, kNfft = 400, kHop = 160, kHalf = 200, kBins = 201, kMaxMels = 128;
constexpr uint32_t kLanesPerFrame = 8, kPointsPerLane = 25;  // 200 = 25 x 8
constexpr uint32_t kPassFrames = 8;                          // frames of one transform pass of a wave
constexpr uint32_t kUnitFrames = 16;                         // frames of a work unit: two passes, so that a store writes 16 consecutive t
constexpr int kWaves = 8;                                    // waves of the persistent workgroup, one workgroup per CU
constexpr float kLogFloor = -10.0f;                          // log10(1e-10): the value of a silent frame and of an empty filter sum

// the first silent frame of a clip with L = min(len, n_frames * 160) live samples, at most n_frames: frames 0 and 1 touch sample 0
// through the reflection, frame t >= 2 starts at sample 160 t - 200 and the reflection at the end only reaches back to N - 41
SS_WH_HD uint32_t first_silent(uint32_t L, uint32_t n_frames)
{
    if (L == 0) return 0;
    uint32_t t = (L + kHalf + kHop - 1) / kHop;  // the smallest t with 160 t - 200 >= L
    if (t < 2) t = 2;
    return t < n_frames ? t : n_frames;
}

// index into the padded-or-trimmed clip a[0 .. N) of raw index i in [-200, N + 200): np.pad(a, 200, mode = "reflect")
SS_WH_HD int32_t reflect(int32_t i, int32_t N) { return i < 0 ? -i : (i >= N ? 2 * N - 2 - i : i); }

SS_WH_HD uint32_t units_per_clip(uint32_t n_frames) { return (n_frames + kUnitFrames - 1) / kUnitFrames; }

SS_WH_HD uint32_t bitrev3(uint32_t j) { return ((j & 1) << 2) | (j & 2) | ((j >> 2) & 1); }

// The table block, float offsets; global layout == LDS layout.  Lane j = lane & 7 of a frame's eight lanes holds the points
// n = j + 8 m, m < 25, before the transform and the bins k = 25 bitrev3(j) + k1, k1 < 25, behind it.
namespace layout {
constexpr int kWin = 0;                   // [25][8] float2: (w[16 m + 2 j], w[16 m + 2 j + 1])
constexpr int kTw2 = kWin + 400;          // [25][8] float2: exp(-2 pi i j k1 / 200)
constexpr int kTwn = kTw2 + 400;          // [25][8] float2: exp(-2 pi i (25 bitrev3(j) + k1) / 400)
constexpr int kStart = kTwn + 400;        // [128] int32: first bin of filter m
constexpr int kLen = kStart + 128;        // [128] int32: taps of filter m
constexpr int kOff = kLen + 128;          // [128] int32: first weight of filter m in kMelW
constexpr int kMelW = kOff + 128;         // [<= 416] the non-zero taps, filter by filter
constexpr int kMelWMax = 416;             // a bin lies under at most two triangles: <= 402 taps
constexpr int kFloats = kMelW + kMelWMax;  // 2000
}  // namespace layout

constexpr int kPRowPitch = 212;   // floats per power row (201 bins): 212 % 32 = 20, eight rows start on eight distinct groups of four banks
constexpr int kTilePitch = 17;    // floats per mel row of the [M][16] store tile
constexpr size_t kWaveFloats = kPassFrames * kPRowPitch + kMaxMels * kTilePitch;
constexpr size_t kLdsBytes = (layout::kFloats + 4 + kWaves * kWaveFloats) * sizeof(float);

}  // namespace whisper
}  // namespace ss
