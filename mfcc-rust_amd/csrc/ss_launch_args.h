// The argument blocks of the dedicated kernels (the *Args structs of ss_device.h), one builder per struct.  A builder is a pure
// function of the family's table description (the *Tables structs of ss_internal.h), the device address of that table block and the
// FrontArgs of the call: shape, framing, window, pre-emphasis, scales, output kind and pointers all come from `a`, so every layout
// (dense, streaming, packed, pool; float or PCM) hands its kernel the same block for the same configuration.  What a layout does
// not have (a packed call has no ld / batch / n_frames) is zero in its FrontArgs and so zero here.  Nothing of ss_config is known
// here, and nothing thread-local: the diagnostic pointers (dbg, stamps) and the device error word (ctl) are set by the caller, one
// line behind the builder.  tools/hosttest/test_launch_args.cpp pins every builder against a block written out field by field.
#pragma once

#include <cmath>
#include <cstddef>
#include <iterator>

#include "ss_device.h"
#include "ss_internal.h"

namespace ss {

// The DCT multipliers of FrontArgs (dct_scale_k / _0 / _00): feature.rs:126-131 (n = T * M as f32) over the clip's `frames` = T, or
// scipy ortho over the axis length (whatever the frame count).
struct DctScales {
    float k, s0, s00;
};
inline DctScales dct_scales(const ss_params &p, size_t frames)
{
    const float g = p.dct2_gain;
    const float M = static_cast<float>(p.num_filters);
    if (p.dct_norm == SS_DCT_ORTHO) return {g * (1.0f / sqrtf(2.0f * M)), g * (1.0f / sqrtf(4.0f * M)), g * (1.0f / sqrtf(4.0f * M))};
    const float nn = static_cast<float>(frames * p.num_filters);
    return {g * (1.0f / sqrtf(2.0f * nn)), g, g * (1.0f / sqrtf(4.0f * nn))};
}
// ... where every clip of the call has a frame count of its own (packed clips): the reference scaling's per-clip multipliers are
// formed on the device, only the gain of column 0 is known here; ortho as above
inline DctScales dct_scales_per_clip(const ss_params &p)
{
    if (p.dct_norm == SS_DCT_ORTHO) return dct_scales(p, 1);
    return {0.0f, p.dct2_gain, 0.0f};
}

// fft_points = 512 MFCC kernel (ss_mfcc512.hip)
inline Fast512Args fast512_args(const Fast512Tables &t, const float *tab, const FrontArgs &a)
{
    Fast512Args f{};
    f.x = a.x;
    f.ld = a.ld;
    f.n_samples = a.n_samples;
    f.batch = a.batch;
    f.flen = a.flen;
    f.step = a.step;
    f.n_frames = a.n_frames;
    f.scale = a.scale;
    f.spectrum_exponent = a.spectrum_exponent;
    f.tab = tab;
    f.mel_wpitch = t.wpitch;
    for (int s = 0; s < 3; ++s) f.mel_q4[s] = t.q4[s];
    f.n_filters = a.n_filters;
    f.n_ceps = a.n_ceps;
    f.dct_scale_k = a.dct_scale_k;
    f.dct_scale_0 = a.dct_scale_0;
    f.dct_scale_00 = a.dct_scale_00;
    f.dc_elimination = a.dc_elimination;
    f.out = a.out0;
    f.out_energy = a.out1;
    f.out_mfe = a.out_kind == OUT_MFE ? 1 : (a.out_kind == OUT_POWER ? 2 : 0);
    f.win_floats = a.window ? t.win_floats : 0;
    f.preemph = a.preemph;
    f.preemph_shift = a.preemph_shift;
    f.center = a.frame_mode == FRAME_CENTER;
    f.pad_reflect = a.pad_reflect;
    f.fullp = t.fullp;
    f.paired = t.paired ? (t.tight ? 2 : 1) : 0;
    return f;
}

// What the mel-spectrogram kernels that share Mel2048Args need of their table block: the 2048-point block (ss_mel2048.hip), the
// 1024-point one (ss_mel_c512) and the 4096-point one (ss_mel_c2048, which has no build for banks past (F+1)/2).
struct MelTableView {
    const float *tab;
    int32_t wpitch;
    const int32_t *q4;  // [4]
    bool fullp;
};
inline MelTableView mel_view(const Mel2048Tables &t, const float *tab) { return {tab, t.wpitch, t.q4, t.fullp}; }
inline MelTableView mel_view(const Mfcc1024Tables &t, const float *tab) { return {tab, t.wpitch, t.q4, t.fullp}; }
inline MelTableView mel_view(const Mfcc4096Tables &t, const float *tab) { return {tab, t.wpitch, t.q4, false}; }

inline Mel2048Args mel2048_args(const MelTableView &t, const FrontArgs &a)
{
    Mel2048Args m{};
    m.x = a.x;
    m.ld = a.ld;
    m.n_samples = a.n_samples;
    m.batch = a.batch;
    m.hop = a.hop;
    m.n_pad = a.n_pad;
    m.rows = a.rows;
    m.real_rows = a.real_rows;
    m.scale = a.scale;
    m.tab = t.tab;
    m.fullp = t.fullp;
    m.mel_wpitch = t.wpitch;
    for (int s = 0; s < 4; ++s) m.mel_q4[s] = t.q4[s];
    m.n_filters = a.n_filters;
    m.out = a.out0;
    m.out_stft = a.out_kind == OUT_STFT;
    return m;
}

// fft_points = 512 mel-spectrogram kernel (ss_mel512.hip)
inline Mel512Args mel512_args(const Mel512Tables &t, const float *tab, const FrontArgs &a)
{
    Mel512Args m{};
    m.x = a.x;
    m.ld = a.ld;
    m.n_samples = a.n_samples;
    m.batch = a.batch;
    m.hop = a.hop;
    m.n_pad = a.n_pad;
    m.rows = a.rows;
    m.real_rows = a.real_rows;
    m.scale = a.scale;
    m.tab = tab;
    m.mel_wpitch = t.wpitch;
    for (int s = 0; s < 5; ++s) m.mel_q4[s] = t.q4[s];
    m.fullp = t.fullp;
    m.n_filters = a.n_filters;
    m.out = a.out0;
    m.out_stft = a.out_kind == OUT_STFT;
    return m;
}

// fft_points = 256 MFCC / mfe kernel (ss_mfcc256.hip: Mfcc256Tables, three slots) and the wide-bank 512-point one (ss_mfcc512w.hip:
// Mfcc512wTables, five slots)
template <typename Tables>
Mfcc256Args mfcc256_args(const Tables &t, const float *tab, const FrontArgs &a)
{
    Mfcc256Args f{};
    f.center = a.frame_mode == FRAME_CENTER;
    f.pad_reflect = a.pad_reflect;
    f.preemph = a.preemph;
    f.preemph_shift = a.preemph_shift;
    f.x = a.x;
    f.ld = a.ld;
    f.n_samples = a.n_samples;
    f.batch = a.batch;
    f.flen = a.flen;
    f.step = a.step;
    f.n_frames = a.n_frames;
    f.scale = a.scale;
    f.spectrum_exponent = a.spectrum_exponent;
    f.tab = tab;
    f.mel_wpitch = t.wpitch;
    for (size_t s = 0; s < std::size(t.q4); ++s) f.mel_q4[s] = t.q4[s];
    f.n_filters = a.n_filters;
    f.n_ceps = a.n_ceps;
    f.dct_scale_k = a.dct_scale_k;
    f.dct_scale_0 = a.dct_scale_0;
    f.dct_scale_00 = a.dct_scale_00;
    f.dc_elimination = a.dc_elimination;
    f.windowed = t.windowed;
    f.out_mfe = a.out_kind == OUT_MFE;
    f.out = a.out0;
    f.out_energy = a.out1;
    return f;
}

// fft_points = 2048 / 1024 MFCC / mfe kernels (ss_mfcc2048.hip: Mfcc2048Tables, ss_mfcc1024.hip: Mfcc1024Tables)
template <typename Tables>
Mfcc2048Args mfcc2048_args(const Tables &t, const float *tab, const FrontArgs &a)
{
    Mfcc2048Args f{};
    f.preemph = a.preemph;
    f.preemph_shift = a.preemph_shift;
    f.x = a.x;
    f.ld = a.ld;
    f.n_samples = a.n_samples;
    f.batch = a.batch;
    f.flen = a.flen;
    f.step = a.step;
    f.n_frames = a.n_frames;
    f.scale = a.scale;
    f.spectrum_exponent = a.spectrum_exponent;
    f.tab = tab;
    f.mel_wpitch = t.wpitch;
    for (int s = 0; s < 4; ++s) f.mel_q4[s] = t.q4[s];
    f.n_filters = a.n_filters;
    f.n_ceps = a.n_ceps;
    f.dct_scale_k = a.dct_scale_k;
    f.dct_scale_0 = a.dct_scale_0;
    f.dct_scale_00 = a.dct_scale_00;
    f.dc_elimination = a.dc_elimination;
    f.windowed = t.windowed;
    f.out_mfe = a.out_kind == OUT_MFE;
    f.center = a.frame_mode == FRAME_CENTER;
    f.pad_reflect = a.pad_reflect;
    f.fullp = t.fullp;
    f.out = a.out0;
    f.out_energy = a.out1;
    return f;
}

// fft_points = 4096 MFCC / mfe kernel (ss_mfcc4096.hip)
inline Mfcc4096Args mfcc4096_args(const Mfcc4096Tables &t, const float *tab, const FrontArgs &a)
{
    Mfcc4096Args f{};
    f.preemph = a.preemph;
    f.preemph_shift = a.preemph_shift;
    f.x = a.x;
    f.ld = a.ld;
    f.n_samples = a.n_samples;
    f.batch = a.batch;
    f.flen = a.flen;
    f.step = a.step;
    f.n_frames = a.n_frames;
    f.scale = a.scale;
    f.spectrum_exponent = a.spectrum_exponent;
    f.tab = tab;
    f.mel_wpitch = t.wpitch;
    for (int s = 0; s < 4; ++s) f.mel_q4[s] = t.q4[s];
    f.cos_floats = t.cos_floats;
    f.dct_fold2 = t.dct_fold2 ? 1 : 0;
    f.n_filters = a.n_filters;
    f.n_ceps = a.n_ceps;
    f.dct_scale_k = a.dct_scale_k;
    f.dct_scale_0 = a.dct_scale_0;
    f.dct_scale_00 = a.dct_scale_00;
    f.dc_elimination = a.dc_elimination;
    f.out = a.out0;
    f.out_energy = a.out1;
    f.out_mfe = a.out_kind == OUT_MFE;
    f.window = a.window;
    return f;
}

}  // namespace ss
