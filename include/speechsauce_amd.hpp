// speechsauce_amd.hpp -- header-only C++ mirror of the reference crate's Rust API over the C ABI
// (speechsauce_amd.h).  Same names, argument meaning and error behaviour as the reference:
//   speechsauce::config::{SpeechConfigBuilder, SpeechConfig}   (speechsauce/src/config.rs:10-190)
//   speechsauce::feature::{mfcc, mfe, mel_spectrogram1, mel_spectrogram2}  (feature.rs:99-233)
//   speechsauce::processing::preemphasis                        (processing.rs:31-53)
//   speechsauce::processing::{stack_frames, power_spectrum}     (processing.rs:65-129, :179-181)
//   speechsauce::functions::{stft1, stft2}                      (functions.rs:199-233, :86-123)
//   speechsauce::processing::{cmvn, cmvnw, derivative_extraction}, feature::extract_derivative_feature
//                                                               (processing.rs:222-371, feature.rs:253-269)
// Where the reference panics, these throw speechsauce::Error carrying the ss_status.
// Arrays are plain row-major std::vector<float> plus shapes (the reference returns ndarray::ArrayN<f32>).
#pragma once

#include <algorithm>
#include <complex>
#include <cstddef>
#include <map>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "speechsauce_amd.h"

namespace speechsauce {

struct Error : std::runtime_error {
    int status;
    Error(int s, const std::string &what) : std::runtime_error(what), status(s) {}
};

inline void check(int status)
{
    if (status != SS_OK) {
        const char *d = ss_last_error_string();
        throw Error(status, (d && *d) ? d : ss_status_string(status));
    }
}

// 2-D / 3-D owning arrays, row-major
struct Array2 {
    std::size_t rows = 0, cols = 0;
    std::vector<float> data;
    float &operator()(std::size_t r, std::size_t c) { return data[r * cols + c]; }
    float operator()(std::size_t r, std::size_t c) const { return data[r * cols + c]; }
};
struct Array3 {
    std::size_t d0 = 0, d1 = 0, d2 = 0;
    std::vector<float> data;
};

class SpeechConfig;

// config.rs:10-97
class SpeechConfigBuilder {
public:
    explicit SpeechConfigBuilder(std::size_t sample_rate) { check(ss_params_default(&p_, static_cast<uint32_t>(sample_rate))); }
    SpeechConfigBuilder &high_freq(float v) { p_.high_frequency = v; return *this; }
    // librosa-compatible variants (ss_params switches): SS_FRAMING_CENTER + SS_PAD_*, SS_MEL_SLANEY / SS_MEL_HTK, SS_MEL_NORM_SLANEY
    SpeechConfigBuilder &framing(int v, int pad_mode = SS_PAD_REFLECT) { p_.framing = v; p_.pad_mode = pad_mode; return *this; }
    SpeechConfigBuilder &mel_scale(int scale, int norm = SS_MEL_NORM_NONE) { p_.mel_scale = scale; p_.mel_norm = norm; return *this; }
    SpeechConfigBuilder &low_freq(float v) { p_.low_frequency = v; return *this; }
    SpeechConfigBuilder &dc_elimination(bool v) { p_.dc_elimination = v; return *this; }
    SpeechConfigBuilder &num_cepstral(std::size_t v) { p_.num_cepstral = static_cast<uint32_t>(v); return *this; }
    SpeechConfigBuilder &frame_stride(float v) { p_.frame_stride = v; return *this; }
    SpeechConfigBuilder &frame_length(float v) { p_.frame_length = v; return *this; }
    SpeechConfigBuilder &fft_points(std::size_t v) { p_.fft_points = static_cast<uint32_t>(v); return *this; }
    // not settable in the reference builder (config.rs:49-82 has no num_filters setter); offered here
    SpeechConfigBuilder &num_filters(std::size_t v) { p_.num_filters = static_cast<uint32_t>(v); return *this; }
    // switches of include/speechsauce_amd.h (reference mode when untouched)
    ss_params &params() { return p_; }
    inline SpeechConfig build() const;

private:
    ss_params p_{};
};

// config.rs:98-190.  Immutable after creation: unlike the reference there is no STFT carry-over state.  Copyable like the
// reference's `#[derive(Clone)]` (config.rs:98): copies share one device handle, released with the last of them.
class SpeechConfig {
public:
    // SpeechConfig::new, config.rs:140-150
    SpeechConfig(std::size_t sample_rate, std::size_t fft_points, float frame_length, float frame_stride, std::size_t num_cepstral,
                 std::size_t num_filters, float low_frequency, float high_frequency, bool dc_elimination)
    {
        check(ss_params_default(&p_, static_cast<uint32_t>(sample_rate)));
        p_.fft_points = static_cast<uint32_t>(fft_points);
        p_.frame_length = frame_length;
        p_.frame_stride = frame_stride;
        p_.num_cepstral = static_cast<uint32_t>(num_cepstral);
        p_.num_filters = static_cast<uint32_t>(num_filters);
        p_.low_frequency = low_frequency;
        p_.high_frequency = high_frequency;
        p_.dc_elimination = dc_elimination;
        create_();
    }
    explicit SpeechConfig(const ss_params &p) : p_(p) { create_(); }
    SpeechConfig() : SpeechConfig(SpeechConfigBuilder(16000).build()) {}  // Default, config.rs:133-137

    const ss_params &params() const { return p_; }
    const ss_config *handle() const { return h_.get(); }
    // the reference's public plain-data fields (config.rs:100-126) as accessors
    std::size_t sample_rate() const { return p_.sample_rate; }
    std::size_t window_size() const { return p_.fft_points; }
    std::size_t window_size_half() const { return p_.fft_points / 2; }
    std::size_t freq_size() const { return p_.fft_points / 2 + 1; }
    std::size_t frame_size() const { return frame_size_; }    // trunc(frame_length * sample_rate), config.rs:154
    float frame_length() const { return p_.frame_length; }
    float frame_stride() const { return p_.frame_stride; }
    std::size_t num_cepstral() const { return p_.num_cepstral; }
    std::size_t num_filters() const { return p_.num_filters; }
    float low_frequency() const { return p_.low_frequency; }
    float high_frequency() const { return p_.high_frequency; }
    bool dc_elimination() const { return p_.dc_elimination != 0; }
    float wnorm() const { return wnorm_; }                    // 2 frame_size / fft_points^2, config.rs:178
    const std::vector<float> &window() const { return window_; }  // Vorbis window of window_size points, config.rs:151-160

private:
    void create_()
    {
        ss_config *h = nullptr;
        check(ss_config_create(&p_, &h));
        h_ = std::shared_ptr<ss_config>(h, [](ss_config *c) { ss_config_destroy(c); });
        // config.rs:154 / :178, the reference's own f32 arithmetic (every config has these two, not only the STFT-capable ones
        // ss_stft_sizes answers for): frame_size = trunc(frame_length * sample_rate), wnorm = 1 / (fft_points^2 / (2 frame_size))
        frame_size_ = static_cast<std::size_t>(p_.frame_length * static_cast<float>(p_.sample_rate));
        const std::size_t n2 = static_cast<std::size_t>(p_.fft_points) * p_.fft_points;
        wnorm_ = 1.0f / (static_cast<float>(n2) / static_cast<float>(2 * frame_size_));
        window_.resize(p_.fft_points);
        check(ss_vorbis_window(window_.size(), window_.data()));
    }
    ss_params p_{};
    std::shared_ptr<ss_config> h_;
    std::size_t frame_size_ = 0;
    float wnorm_ = 0.f;
    std::vector<float> window_;
};

inline SpeechConfig SpeechConfigBuilder::build() const { return SpeechConfig(p_); }

// feature.rs:99-148
inline Array2 mfcc(const float *signal, std::size_t n, const SpeechConfig &cfg)
{
    std::size_t t = 0;
    check(ss_num_frames(&cfg.params(), n, &t));
    Array2 out{t, cfg.num_cepstral(), std::vector<float>(t * cfg.num_cepstral())};
    check(ss_mfcc(cfg.handle(), signal, n, out.data.data()));
    return out;
}
inline Array2 mfcc(const std::vector<float> &signal, const SpeechConfig &cfg) { return mfcc(signal.data(), signal.size(), cfg); }

// feature.rs:200-233: (features [T x M], frame energies [T])
inline std::pair<Array2, std::vector<float>> mfe(const float *signal, std::size_t n, const SpeechConfig &cfg)
{
    std::size_t t = 0;
    check(ss_num_frames(&cfg.params(), n, &t));
    Array2 feat{t, cfg.num_filters(), std::vector<float>(t * cfg.num_filters())};
    std::vector<float> energy(t);
    check(ss_mfe(cfg.handle(), signal, n, feat.data.data(), energy.data()));
    return {std::move(feat), std::move(energy)};
}

// feature.rs:163-174: signal [channels x n] -> [channels x num_filters x rows]
inline Array3 mel_spectrogram2(const float *signal, std::size_t channels, std::size_t n, const SpeechConfig &cfg)
{
    std::size_t rows = 0, real_rows = 0;
    check(ss_stft_rows(&cfg.params(), n, &rows, &real_rows));
    Array3 out{channels, cfg.num_filters(), rows, std::vector<float>(channels * cfg.num_filters() * rows)};
    check(ss_mel_spectrogram(cfg.handle(), signal, channels, n, out.data.data()));
    return out;
}

// feature.rs:151-162 (one channel; the reference's axis mix-up is not reproduced)
inline Array2 mel_spectrogram1(const float *signal, std::size_t n, const SpeechConfig &cfg)
{
    Array3 a = mel_spectrogram2(signal, 1, n, cfg);
    return Array2{a.d1, a.d2, std::move(a.data)};
}

// functions.rs:86-123: Array3<Complex32> [channels x rows x freq_size]
struct ComplexArray3 {
    std::size_t d0 = 0, d1 = 0, d2 = 0;
    std::vector<std::complex<float>> data;
};
inline ComplexArray3 stft2(const float *signal, std::size_t channels, std::size_t n, const SpeechConfig &cfg)
{
    std::size_t rows = 0, real_rows = 0;
    check(ss_stft_rows(&cfg.params(), n, &rows, &real_rows));
    ComplexArray3 out{channels, rows, cfg.freq_size(), std::vector<std::complex<float>>(channels * rows * cfg.freq_size())};
    // std::complex<float> is layout-compatible with float[2] (re, im): the interleaved block the ABI writes
    check(ss_stft(cfg.handle(), signal, channels, n, reinterpret_cast<float *>(out.data.data())));
    return out;
}
// functions.rs:199-233 (one channel): [rows x freq_size]
inline ComplexArray3 stft1(const float *signal, std::size_t n, const SpeechConfig &cfg) { return stft2(signal, 1, n, cfg); }

// processing.rs:65-129 with the reference's own argument list:
//   stack_frames(signal, sample_rate, frame_length, frame_stride, filter, zero_padding) -> frames [num_frames x frame_len]
// `filter` (may be null) is called with the frame length and returns the window as an Array2 of shape (1, frame_len) -- row 0
// multiplies every frame, what repeat_axis(filt, Axis(0), numframes) does in processing.rs:122-126 (a (frame_len, 1) column is
// read down its column).  No SpeechConfig and no FFT length are involved: any sampling rate and frame length.
using FrameFilter = Array2 (*)(std::size_t);
inline Array2 stack_frames(const float *signal, std::size_t n, std::size_t sample_rate, float frame_length, float frame_stride,
                           FrameFilter filter, bool zero_padding)
{
    std::size_t t = 0, flen = 0;
    check(ss_stack_frames_shape(n, static_cast<uint32_t>(sample_rate), frame_length, frame_stride, zero_padding ? 1 : 0, &t, &flen));
    std::vector<float> window;
    if (filter) {
        const Array2 w = filter(flen);
        if (w.rows * w.cols != flen || (w.rows != 1 && w.cols != 1)) throw Error(SS_ERR_ARG, "stack_frames: filter(frame_len) must give frame_len values");
        window = w.data;
    }
    Array2 out{t, flen, std::vector<float>(t * flen)};
    check(ss_stack_frames_signal(signal, n, static_cast<uint32_t>(sample_rate), frame_length, frame_stride,
                                 filter ? window.data() : nullptr, zero_padding ? 1 : 0, out.data.data()));
    return out;
}
inline Array2 stack_frames(const std::vector<float> &signal, std::size_t sample_rate, float frame_length, float frame_stride,
                           FrameFilter filter, bool zero_padding)
{
    return stack_frames(signal.data(), signal.size(), sample_rate, frame_length, frame_stride, filter, zero_padding);
}

// The same stage with the framing taken from a config (its framing / mfcc_window / pad_mode switches apply: literal and centred
// framing exist only in this form).  An extra beside the reference's signature above.
inline Array2 stack_frames(const float *signal, std::size_t n, const SpeechConfig &cfg)
{
    std::size_t t = 0, flen = 0, step = 0;
    check(ss_num_frames(&cfg.params(), n, &t));
    check(ss_frame_sizes(&cfg.params(), &flen, &step));
    Array2 out{t, flen, std::vector<float>(t * flen)};
    check(ss_stack_frames(cfg.handle(), signal, n, out.data.data()));
    return out;
}

// processing.rs:179-181 on an existing config (fft_points = the config's).  An extra beside the reference's signature below.
inline Array2 power_spectrum(const Array2 &frames, const SpeechConfig &cfg)
{
    Array2 out{frames.rows, cfg.freq_size(), std::vector<float>(frames.rows * cfg.freq_size())};
    check(ss_power_spectrum_frames(cfg.handle(), frames.data.data(), frames.rows, frames.cols, out.data.data()));
    return out;
}

// processing.rs:179-181 with the reference's own argument list: power_spectrum(frames, fft_points).  Only fft_points matters to
// this stage; the config it runs on is kept per fft_points in a small process-wide cache (the Python front memoises the same
// way), guarded by a mutex, so repeated calls cost one lookup.
inline Array2 power_spectrum(const Array2 &frames, std::size_t fft_points)
{
    static std::mutex mu;
    static std::map<std::size_t, std::unique_ptr<SpeechConfig>> cache;
    const SpeechConfig *cfg = nullptr;
    {
        std::lock_guard<std::mutex> lock(mu);
        auto it = cache.find(fft_points);
        if (it == cache.end()) {
            // a config that validates for this FFT length: a frame of half its length, a bank that fits its spectrum
            SpeechConfigBuilder b(16000);
            const std::size_t nf = std::max<std::size_t>(1, std::min<std::size_t>(40, fft_points / 8));
            b.fft_points(fft_points).frame_length(static_cast<float>(fft_points) / 32000.0f).frame_stride(static_cast<float>(fft_points) / 64000.0f)
                .num_filters(nf).num_cepstral(std::min<std::size_t>(13, nf));
            it = cache.emplace(fft_points, std::make_unique<SpeechConfig>(b.build())).first;
        }
        cfg = it->second.get();  // configs are immutable and thread-safe; entries are never removed
    }
    return power_spectrum(frames, *cfg);
}

// processing.rs:31-53
inline std::vector<float> preemphasis(const std::vector<float> &signal, long shift = 1, float cof = 0.98f)
{
    std::vector<float> y(signal.size());
    check(ss_preemphasis(signal.data(), signal.size(), shift, cof, y.data()));
    return y;
}

// ---- post-processing on a row-major [rows x cols] feature matrix ----

// processing.rs:265-300
inline std::vector<float> cmvn(const std::vector<float> &vec, size_t rows, size_t cols, bool variance_normalization = false)
{
    if (vec.size() != rows * cols) throw Error(SS_ERR_ARG, "cmvn: shape mismatch");
    std::vector<float> out(vec.size());
    check(ss_cmvn(vec.data(), rows, cols, variance_normalization ? 1 : 0, out.data()));
    return out;
}

// processing.rs:315-371 (win_size must be odd, as the reference asserts)
inline std::vector<float> cmvnw(const std::vector<float> &vec, size_t rows, size_t cols, size_t win_size = 301,
                                bool variance_normalization = false)
{
    if (vec.size() != rows * cols) throw Error(SS_ERR_ARG, "cmvnw: shape mismatch");
    std::vector<float> out(vec.size());
    check(ss_cmvnw(vec.data(), rows, cols, win_size, variance_normalization ? 1 : 0, out.data()));
    return out;
}

// Ragged streaming MFCC / mfe over a pool of stream states, fed signed 16-bit PCM (ss_*_stream_packed_i16*): stream sample =
// pcm * scale, scale a power of two in [2^-64, 2^64]; the pool stays float.  Device forms: raw device pointers and a hipStream_t,
// asynchronous (d_x 4-byte aligned).  Host forms: x the packed chunks, sample_offsets n_active + 1 offsets in samples, slots the
// pool row of each entry, pool the [pool_streams x S] states (updated in place); rows = sample_offsets.back() / hop.
inline void mfcc_stream_packed_i16_device(const SpeechConfig &cfg, const int16_t *d_x, std::size_t n_active, const int64_t *d_sample_offsets,
                                          const int64_t *d_row_offsets, std::size_t total_rows, const int32_t *d_slots,
                                          std::size_t pool_streams, float scale, uint32_t norm_frames, float *d_pool, float *d_out, void *stream)
{
    check(ss_mfcc_stream_packed_i16_device(cfg.handle(), d_x, n_active, d_sample_offsets, d_row_offsets, total_rows, d_slots, pool_streams,
                                           scale, norm_frames, d_pool, d_out, stream));
}

inline void mfe_stream_packed_i16_device(const SpeechConfig &cfg, const int16_t *d_x, std::size_t n_active, const int64_t *d_sample_offsets,
                                         const int64_t *d_row_offsets, std::size_t total_rows, const int32_t *d_slots,
                                         std::size_t pool_streams, float scale, float *d_pool, float *d_feat, float *d_energy, void *stream)
{
    check(ss_mfe_stream_packed_i16_device(cfg.handle(), d_x, n_active, d_sample_offsets, d_row_offsets, total_rows, d_slots, pool_streams,
                                          scale, d_pool, d_feat, d_energy, stream));
}

inline void mfcc_stream_packed_i16(const SpeechConfig &cfg, const std::vector<int16_t> &x, const std::vector<int64_t> &sample_offsets,
                                   const std::vector<int32_t> &slots, std::size_t pool_streams, float scale, uint32_t norm_frames,
                                   std::vector<float> &pool, std::vector<float> &out)
{
    if (sample_offsets.size() != slots.size() + 1) throw Error(SS_ERR_ARG, "mfcc_stream_packed_i16: one offset more than slots");
    check(ss_mfcc_stream_packed_i16(cfg.handle(), x.data(), slots.size(), sample_offsets.data(), slots.data(), pool_streams, scale,
                                    norm_frames, pool.data(), out.data()));
}

inline void mfe_stream_packed_i16(const SpeechConfig &cfg, const std::vector<int16_t> &x, const std::vector<int64_t> &sample_offsets,
                                  const std::vector<int32_t> &slots, std::size_t pool_streams, float scale, std::vector<float> &pool,
                                  std::vector<float> &feat, std::vector<float> &energy)
{
    if (sample_offsets.size() != slots.size() + 1) throw Error(SS_ERR_ARG, "mfe_stream_packed_i16: one offset more than slots");
    check(ss_mfe_stream_packed_i16(cfg.handle(), x.data(), slots.size(), sample_offsets.data(), slots.data(), pool_streams, scale,
                                   pool.data(), feat.data(), energy.data()));
}

// The one-shot MFCC / mfe calls fed signed 16-bit PCM (ss_*_batch_i16*, ss_*_packed_i16*): sample = pcm * scale, scale a power of two
// in [2^-64, 2^64]; bit for bit the float calls on the converted buffer.  ld and the offsets are in samples; 2-byte alignment is
// enough.  Device forms: raw device pointers and a hipStream_t, asynchronous.  Host forms: the samples cross the link as int16.
inline void mfcc_batch_i16_device(const SpeechConfig &cfg, const int16_t *d_x, std::size_t batch, std::size_t n_samples, std::size_t ld,
                                  float scale, float *d_out, void *stream)
{
    check(ss_mfcc_batch_i16_device(cfg.handle(), d_x, batch, n_samples, ld, scale, d_out, stream));
}

inline void mfe_batch_i16_device(const SpeechConfig &cfg, const int16_t *d_x, std::size_t batch, std::size_t n_samples, std::size_t ld,
                                 float scale, float *d_feat, float *d_energy, void *stream)
{
    check(ss_mfe_batch_i16_device(cfg.handle(), d_x, batch, n_samples, ld, scale, d_feat, d_energy, stream));
}

inline void mfcc_packed_i16_device(const SpeechConfig &cfg, const int16_t *d_x, std::size_t n_clips, const int64_t *d_sample_offsets,
                                   float scale, const int64_t *d_frame_offsets, std::size_t total_frames, float *d_out, void *stream)
{
    check(ss_mfcc_packed_i16_device(cfg.handle(), d_x, n_clips, d_sample_offsets, scale, d_frame_offsets, total_frames, d_out, stream));
}

inline void mfe_packed_i16_device(const SpeechConfig &cfg, const int16_t *d_x, std::size_t n_clips, const int64_t *d_sample_offsets,
                                  float scale, const int64_t *d_frame_offsets, std::size_t total_frames, float *d_feat, float *d_energy,
                                  void *stream)
{
    check(ss_mfe_packed_i16_device(cfg.handle(), d_x, n_clips, d_sample_offsets, scale, d_frame_offsets, total_frames, d_feat, d_energy,
                                   stream));
}

// x: batch rows of n_samples at row stride ld; out [batch x frames x num_cepstral] (feat [.. x num_filters], energy [batch x frames])
inline void mfcc_batch_i16(const SpeechConfig &cfg, const std::vector<int16_t> &x, std::size_t batch, std::size_t n_samples, std::size_t ld,
                           float scale, std::vector<float> &out)
{
    if (batch && (ld < n_samples || x.size() < (batch - 1) * ld + n_samples)) throw Error(SS_ERR_ARG, "mfcc_batch_i16: x is too short");
    check(ss_mfcc_batch_i16(cfg.handle(), x.data(), batch, n_samples, ld, scale, out.data()));
}

inline void mfe_batch_i16(const SpeechConfig &cfg, const std::vector<int16_t> &x, std::size_t batch, std::size_t n_samples, std::size_t ld,
                          float scale, std::vector<float> &feat, std::vector<float> &energy)
{
    if (batch && (ld < n_samples || x.size() < (batch - 1) * ld + n_samples)) throw Error(SS_ERR_ARG, "mfe_batch_i16: x is too short");
    check(ss_mfe_batch_i16(cfg.handle(), x.data(), batch, n_samples, ld, scale, feat.data(), energy.data()));
}

// x: the packed clips, sample_offsets n_clips + 1 offsets in samples; the outputs hold the clips' rows end to end
inline void mfcc_packed_i16(const SpeechConfig &cfg, const std::vector<int16_t> &x, const std::vector<int64_t> &sample_offsets, float scale,
                            std::vector<float> &out)
{
    if (sample_offsets.empty()) throw Error(SS_ERR_ARG, "mfcc_packed_i16: n_clips + 1 offsets");
    check(ss_mfcc_packed_i16(cfg.handle(), x.data(), sample_offsets.size() - 1, sample_offsets.data(), scale, out.data()));
}

inline void mfe_packed_i16(const SpeechConfig &cfg, const std::vector<int16_t> &x, const std::vector<int64_t> &sample_offsets, float scale,
                           std::vector<float> &feat, std::vector<float> &energy)
{
    if (sample_offsets.empty()) throw Error(SS_ERR_ARG, "mfe_packed_i16: n_clips + 1 offsets");
    check(ss_mfe_packed_i16(cfg.handle(), x.data(), sample_offsets.size() - 1, sample_offsets.data(), scale, feat.data(), energy.data()));
}

// The mel spectrogram / STFT calls fed signed 16-bit PCM (ss_mel_spectrogram*_i16*, ss_stft*_i16*): sample = pcm * scale, scale a
// power of two in [2^-64, 2^64]; bit for bit the float calls on the converted buffer.  ld and the offsets are in samples; 2-byte
// alignment is enough (4-byte for the pool's device forms; the pool stays float).  Device forms: raw device pointers and a
// hipStream_t, asynchronous.  Host forms: the samples cross the link as int16.
inline void mel_spectrogram_i16_device(const SpeechConfig &cfg, const int16_t *d_x, std::size_t channels, std::size_t n_samples,
                                       std::size_t ld, float scale, float *d_out, void *stream)
{
    check(ss_mel_spectrogram_i16_device(cfg.handle(), d_x, channels, n_samples, ld, scale, d_out, stream));
}

inline void stft_i16_device(const SpeechConfig &cfg, const int16_t *d_x, std::size_t channels, std::size_t n_samples, std::size_t ld,
                            float scale, float *d_out, void *stream)
{
    check(ss_stft_i16_device(cfg.handle(), d_x, channels, n_samples, ld, scale, d_out, stream));
}

inline void mel_spectrogram_packed_i16_device(const SpeechConfig &cfg, const int16_t *d_x, std::size_t n_clips,
                                              const int64_t *d_sample_offsets, float scale, const int64_t *d_row_offsets,
                                              std::size_t total_rows, float *d_out, void *stream)
{
    check(ss_mel_spectrogram_packed_i16_device(cfg.handle(), d_x, n_clips, d_sample_offsets, scale, d_row_offsets, total_rows, d_out, stream));
}

inline void stft_packed_i16_device(const SpeechConfig &cfg, const int16_t *d_x, std::size_t n_clips, const int64_t *d_sample_offsets,
                                   float scale, const int64_t *d_row_offsets, std::size_t total_rows, float *d_out, void *stream)
{
    check(ss_stft_packed_i16_device(cfg.handle(), d_x, n_clips, d_sample_offsets, scale, d_row_offsets, total_rows, d_out, stream));
}

inline void mel_spectrogram_stream_packed_i16_device(const SpeechConfig &cfg, const int16_t *d_x, std::size_t n_active,
                                                     const int64_t *d_sample_offsets, const int64_t *d_row_offsets, std::size_t total_rows,
                                                     const int32_t *d_slots, std::size_t pool_streams, float scale, float *d_pool,
                                                     float *d_out, void *stream)
{
    check(ss_mel_spectrogram_stream_packed_i16_device(cfg.handle(), d_x, n_active, d_sample_offsets, d_row_offsets, total_rows, d_slots,
                                                      pool_streams, scale, d_pool, d_out, stream));
}

inline void stft_stream_packed_i16_device(const SpeechConfig &cfg, const int16_t *d_x, std::size_t n_active, const int64_t *d_sample_offsets,
                                          const int64_t *d_row_offsets, std::size_t total_rows, const int32_t *d_slots,
                                          std::size_t pool_streams, float scale, float *d_pool, float *d_out, void *stream)
{
    check(ss_stft_stream_packed_i16_device(cfg.handle(), d_x, n_active, d_sample_offsets, d_row_offsets, total_rows, d_slots, pool_streams,
                                           scale, d_pool, d_out, stream));
}

// x: channels rows of n_samples; out [channels x num_filters x rows] (stft: [channels x rows x (fft_points / 2 + 1) x 2])
inline void mel_spectrogram_i16(const SpeechConfig &cfg, const std::vector<int16_t> &x, std::size_t channels, std::size_t n_samples,
                                float scale, std::vector<float> &out)
{
    if (x.size() < channels * n_samples) throw Error(SS_ERR_ARG, "mel_spectrogram_i16: x is too short");
    check(ss_mel_spectrogram_i16(cfg.handle(), x.data(), channels, n_samples, scale, out.data()));
}

inline void stft_i16(const SpeechConfig &cfg, const std::vector<int16_t> &x, std::size_t channels, std::size_t n_samples, float scale,
                     std::vector<float> &out)
{
    if (x.size() < channels * n_samples) throw Error(SS_ERR_ARG, "stft_i16: x is too short");
    check(ss_stft_i16(cfg.handle(), x.data(), channels, n_samples, scale, out.data()));
}

// x: the packed clips, sample_offsets n_clips + 1 offsets in samples; out holds the clips' blocks / rows end to end
inline void mel_spectrogram_packed_i16(const SpeechConfig &cfg, const std::vector<int16_t> &x, const std::vector<int64_t> &sample_offsets,
                                       float scale, std::vector<float> &out)
{
    if (sample_offsets.empty()) throw Error(SS_ERR_ARG, "mel_spectrogram_packed_i16: n_clips + 1 offsets");
    check(ss_mel_spectrogram_packed_i16(cfg.handle(), x.data(), sample_offsets.size() - 1, sample_offsets.data(), scale, out.data()));
}

inline void stft_packed_i16(const SpeechConfig &cfg, const std::vector<int16_t> &x, const std::vector<int64_t> &sample_offsets, float scale,
                            std::vector<float> &out)
{
    if (sample_offsets.empty()) throw Error(SS_ERR_ARG, "stft_packed_i16: n_clips + 1 offsets");
    check(ss_stft_packed_i16(cfg.handle(), x.data(), sample_offsets.size() - 1, sample_offsets.data(), scale, out.data()));
}

// Log-mel spectrogram (ss_log_mel_spectrogram*): the mel calls with librosa's power_to_db per clip, converted in the mel kernels'
// epilogue -- per clip bit for bit the mel call followed by ss_power_to_db_packed_device with every clip as its own segment.  The
// top_db floor is each clip's own maximum - top_db (top_db < 0: no floor); ss_power_to_db_device on a multi-channel block takes one
// maximum over the whole block instead.  Shapes, layouts and errors are the mel calls'; amin > 0 and ref not NaN, else SS_ERR_ARG.
struct DbScale {
    float ref = 1.0f, amin = 1e-10f, top_db = 80.0f;
};

inline void log_mel_spectrogram_device(const SpeechConfig &cfg, const float *d_x, std::size_t channels, std::size_t n_samples, std::size_t ld,
                                       const DbScale &db, float *d_out, void *stream)
{
    check(ss_log_mel_spectrogram_device(cfg.handle(), d_x, channels, n_samples, ld, db.ref, db.amin, db.top_db, d_out, stream));
}

inline void log_mel_spectrogram_i16_device(const SpeechConfig &cfg, const int16_t *d_x, std::size_t channels, std::size_t n_samples,
                                           std::size_t ld, float scale, const DbScale &db, float *d_out, void *stream)
{
    check(ss_log_mel_spectrogram_i16_device(cfg.handle(), d_x, channels, n_samples, ld, scale, db.ref, db.amin, db.top_db, d_out, stream));
}

inline void log_mel_spectrogram_packed_device(const SpeechConfig &cfg, const float *d_x, std::size_t n_clips, const int64_t *d_sample_offsets,
                                              const int64_t *d_row_offsets, std::size_t total_rows, const DbScale &db, float *d_out,
                                              void *stream)
{
    check(ss_log_mel_spectrogram_packed_device(cfg.handle(), d_x, n_clips, d_sample_offsets, d_row_offsets, total_rows, db.ref, db.amin,
                                               db.top_db, d_out, stream));
}

inline void log_mel_spectrogram_packed_i16_device(const SpeechConfig &cfg, const int16_t *d_x, std::size_t n_clips,
                                                  const int64_t *d_sample_offsets, float scale, const int64_t *d_row_offsets,
                                                  std::size_t total_rows, const DbScale &db, float *d_out, void *stream)
{
    check(ss_log_mel_spectrogram_packed_i16_device(cfg.handle(), d_x, n_clips, d_sample_offsets, scale, d_row_offsets, total_rows, db.ref,
                                                   db.amin, db.top_db, d_out, stream));
}

// x: channels rows of n_samples; out [channels x num_filters x rows]
inline void log_mel_spectrogram(const SpeechConfig &cfg, const std::vector<float> &x, std::size_t channels, std::size_t n_samples,
                                const DbScale &db, std::vector<float> &out)
{
    if (x.size() < channels * n_samples) throw Error(SS_ERR_ARG, "log_mel_spectrogram: x is too short");
    check(ss_log_mel_spectrogram(cfg.handle(), x.data(), channels, n_samples, db.ref, db.amin, db.top_db, out.data()));
}

inline void log_mel_spectrogram_i16(const SpeechConfig &cfg, const std::vector<int16_t> &x, std::size_t channels, std::size_t n_samples,
                                    float scale, const DbScale &db, std::vector<float> &out)
{
    if (x.size() < channels * n_samples) throw Error(SS_ERR_ARG, "log_mel_spectrogram_i16: x is too short");
    check(ss_log_mel_spectrogram_i16(cfg.handle(), x.data(), channels, n_samples, scale, db.ref, db.amin, db.top_db, out.data()));
}

// x: the packed clips, sample_offsets n_clips + 1 offsets in samples; out holds the clips' [num_filters x R_b] blocks end to end
inline void log_mel_spectrogram_packed(const SpeechConfig &cfg, const std::vector<float> &x, const std::vector<int64_t> &sample_offsets,
                                       const DbScale &db, std::vector<float> &out)
{
    if (sample_offsets.empty()) throw Error(SS_ERR_ARG, "log_mel_spectrogram_packed: n_clips + 1 offsets");
    check(ss_log_mel_spectrogram_packed(cfg.handle(), x.data(), sample_offsets.size() - 1, sample_offsets.data(), db.ref, db.amin, db.top_db,
                                        out.data()));
}

inline void log_mel_spectrogram_packed_i16(const SpeechConfig &cfg, const std::vector<int16_t> &x, const std::vector<int64_t> &sample_offsets,
                                           float scale, const DbScale &db, std::vector<float> &out)
{
    if (sample_offsets.empty()) throw Error(SS_ERR_ARG, "log_mel_spectrogram_packed_i16: n_clips + 1 offsets");
    check(ss_log_mel_spectrogram_packed_i16(cfg.handle(), x.data(), sample_offsets.size() - 1, sample_offsets.data(), scale, db.ref, db.amin,
                                            db.top_db, out.data()));
}

// x the packed chunks, slots the pool row of each entry, pool the [pool_streams x S] states (updated in place)
inline void mel_spectrogram_stream_packed_i16(const SpeechConfig &cfg, const std::vector<int16_t> &x, const std::vector<int64_t> &sample_offsets,
                                              const std::vector<int32_t> &slots, std::size_t pool_streams, float scale,
                                              std::vector<float> &pool, std::vector<float> &out)
{
    if (sample_offsets.size() != slots.size() + 1) throw Error(SS_ERR_ARG, "mel_spectrogram_stream_packed_i16: one offset more than slots");
    check(ss_mel_spectrogram_stream_packed_i16(cfg.handle(), x.data(), slots.size(), sample_offsets.data(), slots.data(), pool_streams, scale,
                                               pool.data(), out.data()));
}

inline void stft_stream_packed_i16(const SpeechConfig &cfg, const std::vector<int16_t> &x, const std::vector<int64_t> &sample_offsets,
                                   const std::vector<int32_t> &slots, std::size_t pool_streams, float scale, std::vector<float> &pool,
                                   std::vector<float> &out)
{
    if (sample_offsets.size() != slots.size() + 1) throw Error(SS_ERR_ARG, "stft_stream_packed_i16: one offset more than slots");
    check(ss_stft_stream_packed_i16(cfg.handle(), x.data(), slots.size(), sample_offsets.data(), slots.data(), pool_streams, scale,
                                    pool.data(), out.data()));
}

// cmvn / cmvnw / power_to_db of every clip of a packed block on its own rows (ss_*_packed): clip b owns rows offsets[b] ..
// offsets[b+1] of the [total_rows x cols] block `vec`; offsets has n_clips + 1 non-decreasing entries and starts at 0
inline std::vector<float> cmvn_packed(const std::vector<float> &vec, const std::vector<int64_t> &offsets, size_t cols,
                                      bool variance_normalization = false)
{
    if (cols == 0 || vec.size() % cols || offsets.empty()) throw Error(SS_ERR_ARG, "cmvn_packed: shape mismatch");
    std::vector<float> out(vec.size());
    check(ss_cmvn_packed(vec.data(), offsets.size() - 1, offsets.data(), vec.size() / cols, cols, variance_normalization ? 1 : 0, out.data()));
    return out;
}

// Grouped CMVN (ss_cmvn_stats_packed / ss_cmvn_apply_packed / ss_cmvn_grouped_packed): per-speaker and global statistics.  A group's
// statistics are a row [n | mean | var] of cmvn_stats_len(cols) = 2 * cols + 1 doubles; `stats` is [n_groups x that], all zeros =
// fresh; groups[b] is clip b's group, -1 leaves the clip out, an empty `groups` puts every clip into group 0.
inline size_t cmvn_stats_len(size_t cols)
{
    size_t len = 0;
    check(ss_cmvn_stats_len(cols, &len));
    return len;
}
inline void cmvn_stats_packed(const std::vector<float> &vec, const std::vector<int64_t> &offsets, size_t cols, const std::vector<int32_t> &groups,
                              size_t n_groups, std::vector<double> &stats)
{
    if (cols == 0 || vec.size() % cols || offsets.empty() || (!groups.empty() && groups.size() != offsets.size() - 1) ||
        stats.size() != n_groups * (2 * cols + 1))
        throw Error(SS_ERR_ARG, "cmvn_stats_packed: shape mismatch");
    check(ss_cmvn_stats_packed(vec.data(), offsets.size() - 1, offsets.data(), vec.size() / cols, cols, groups.empty() ? nullptr : groups.data(),
                               n_groups, stats.data()));
}
// rows of clips that are left out (group -1, a group that has seen no row) come back as zeros
inline std::vector<float> cmvn_apply_packed(const std::vector<float> &vec, const std::vector<int64_t> &offsets, size_t cols,
                                            const std::vector<int32_t> &groups, size_t n_groups, const std::vector<double> &stats,
                                            bool variance_normalization = false)
{
    if (cols == 0 || vec.size() % cols || offsets.empty() || (!groups.empty() && groups.size() != offsets.size() - 1) ||
        stats.size() != n_groups * (2 * cols + 1))
        throw Error(SS_ERR_ARG, "cmvn_apply_packed: shape mismatch");
    std::vector<float> out(vec.size());
    check(ss_cmvn_apply_packed(vec.data(), offsets.size() - 1, offsets.data(), vec.size() / cols, cols, groups.empty() ? nullptr : groups.data(),
                               n_groups, stats.data(), variance_normalization ? 1 : 0, out.data()));
    return out;
}
inline std::vector<float> cmvn_grouped_packed(const std::vector<float> &vec, const std::vector<int64_t> &offsets, size_t cols,
                                              const std::vector<int32_t> &groups, size_t n_groups, bool variance_normalization = false)
{
    if (cols == 0 || vec.size() % cols || offsets.empty() || (!groups.empty() && groups.size() != offsets.size() - 1))
        throw Error(SS_ERR_ARG, "cmvn_grouped_packed: shape mismatch");
    std::vector<float> out(vec.size());
    check(ss_cmvn_grouped_packed(vec.data(), offsets.size() - 1, offsets.data(), vec.size() / cols, cols, groups.empty() ? nullptr : groups.data(),
                                 n_groups, variance_normalization ? 1 : 0, out.data()));
    return out;
}
// one statistics row <-> Kaldi's [2 x (cols + 1)] accumulator (sum x | count, then sum x^2 | 0)
inline std::vector<double> cmvn_stats_to_kaldi(const std::vector<double> &stats_row)
{
    if (stats_row.size() < 3 || stats_row.size() % 2 == 0) throw Error(SS_ERR_ARG, "cmvn_stats_to_kaldi: a row has 2 * cols + 1 doubles");
    const size_t cols = (stats_row.size() - 1) / 2;
    std::vector<double> kaldi(2 * (cols + 1));
    check(ss_cmvn_stats_to_kaldi(stats_row.data(), cols, kaldi.data()));
    return kaldi;
}
inline std::vector<double> cmvn_stats_from_kaldi(const std::vector<double> &kaldi)
{
    if (kaldi.size() < 4 || kaldi.size() % 2) throw Error(SS_ERR_ARG, "cmvn_stats_from_kaldi: an accumulator has 2 * (cols + 1) doubles");
    const size_t cols = kaldi.size() / 2 - 1;
    std::vector<double> row(2 * cols + 1);
    check(ss_cmvn_stats_from_kaldi(kaldi.data(), cols, row.data()));
    return row;
}

// Kaldi add-deltas of every clip of a packed block on its own rows (ss_add_deltas_packed): -> [total_rows x (order + 1) * cols], row t =
// [x[t] | delta | delta-delta] over neighbouring frames; order 1 or 2, order * window at most 32.  A dense matrix: offsets = {0, rows}
inline std::vector<float> add_deltas_packed(const std::vector<float> &vec, const std::vector<int64_t> &offsets, size_t cols, size_t order = 2,
                                            size_t window = 2)
{
    if (cols == 0 || vec.size() % cols || offsets.empty() || order == 0 || order > 2) throw Error(SS_ERR_ARG, "add_deltas_packed: shape mismatch");
    std::vector<float> out(vec.size() * (order + 1));
    check(ss_add_deltas_packed(vec.data(), offsets.size() - 1, offsets.data(), vec.size() / cols, cols, order, window, out.data()));
    return out;
}

// Frame splicing and subsampling of every clip of a packed block on its own rows (ss_splice_packed): output row k of a clip is its rows
// k * stride - left .. k * stride + right side by side, clamped to the clip (bit copies); ceil(T_b / stride) rows of (left + 1 + right)
// * cols floats per clip, in the clips' order.  left, right at most 32, stride 1 .. 32.  A dense matrix: offsets = {0, rows}
inline std::vector<float> splice_packed(const std::vector<float> &vec, const std::vector<int64_t> &offsets, size_t cols, size_t left, size_t right,
                                        size_t stride = 1)
{
    if (cols == 0 || vec.size() % cols || offsets.empty() || left > 32 || right > 32) throw Error(SS_ERR_ARG, "splice_packed: shape mismatch");
    std::vector<int64_t> out_offsets(offsets.size());
    check(ss_splice_packed_offsets(offsets.size() - 1, offsets.data(), stride, out_offsets.data()));
    std::vector<float> out(static_cast<size_t>(out_offsets.back()) * (left + 1 + right) * cols);
    check(ss_splice_packed(vec.data(), offsets.size() - 1, offsets.data(), vec.size() / cols, cols, left, right, stride, out.data()));
    return out;
}

// An affine transform [out_dim x in_dim] (+ bias) applied behind the splice stage without the spliced block ever being written
// (ss_affine_*, ss_affine_splice_packed; not in the reference crate): Kaldi's splice-feats | transform-feats.  The handle is shared
// by copies; the first call that runs uploads the matrix.
class Affine {
public:
    // matrix: row-major [out_dim x in_dim] (1 .. 256 by 1 .. 4096); bias: empty, or [out_dim]
    Affine(const std::vector<float> &matrix, size_t out_dim, size_t in_dim, const std::vector<float> &bias = {}) : out_dim_(out_dim), in_dim_(in_dim)
    {
        if (matrix.size() != out_dim * in_dim || (!bias.empty() && bias.size() != out_dim)) throw Error(SS_ERR_ARG, "Affine: shape mismatch");
        ss_affine *raw = nullptr;
        check(ss_affine_create(matrix.data(), out_dim, in_dim, in_dim, bias.empty() ? nullptr : bias.data(), &raw));
        h_ = std::shared_ptr<ss_affine>(raw, ss_affine_destroy);
    }
    const ss_affine *handle() const { return h_.get(); }
    size_t out_dim() const { return out_dim_; }
    size_t in_dim() const { return in_dim_; }
    // 4 * ceil(in_dim / 4): the steps of every output element's fmaf chain
    size_t chain_len() const
    {
        size_t k4 = 0;
        check(ss_affine_chain_len(in_dim_, &k4));
        return k4;
    }
    // splice_packed followed by the transform, in one launch: ceil(T_b / stride) rows of out_dim floats per clip, in the clips' order;
    // in_dim must be (left + 1 + right) * cols.  left = right = 0, stride = 1 is transform-feats.  A dense matrix: offsets = {0, rows}
    std::vector<float> splice_packed(const std::vector<float> &vec, const std::vector<int64_t> &offsets, size_t cols, size_t left, size_t right,
                                     size_t stride = 1) const
    {
        if (cols == 0 || vec.size() % cols || offsets.empty() || left > 32 || right > 32) throw Error(SS_ERR_ARG, "Affine::splice_packed: shape mismatch");
        std::vector<int64_t> out_offsets(offsets.size());
        check(ss_splice_packed_offsets(offsets.size() - 1, offsets.data(), stride, out_offsets.data()));
        std::vector<float> out(static_cast<size_t>(out_offsets.back()) * out_dim_);
        check(ss_affine_splice_packed(h_.get(), vec.data(), offsets.size() - 1, offsets.data(), vec.size() / cols, cols, left, right, stride, out.data()));
        return out;
    }

private:
    std::shared_ptr<ss_affine> h_;
    size_t out_dim_, in_dim_;
};

// Kaldi compute-vad-energy of every clip of a packed block on its own rows (ss_vad_energy_packed): one byte 0 / 1 per row, and (where
// `counts` is given) the voiced rows of every clip.  The defaults are Kaldi's; the x-vector recipes use 5.5 / 0.5 / 2 / 0.12.  A dense
// matrix: offsets = {0, rows}
inline std::vector<uint8_t> vad_energy_packed(const std::vector<float> &vec, const std::vector<int64_t> &offsets, size_t cols, size_t energy_col = 0,
                                              float energy_threshold = 5.0f, float energy_mean_scale = 0.5f, size_t frames_context = 0,
                                              float proportion_threshold = 0.6f, std::vector<int64_t> *counts = nullptr)
{
    if (cols == 0 || vec.size() % cols || offsets.empty()) throw Error(SS_ERR_ARG, "vad_energy_packed: shape mismatch");
    std::vector<uint8_t> mask(vec.size() / cols);
    if (counts) counts->assign(offsets.size() - 1, 0);
    check(ss_vad_energy_packed(vec.data(), offsets.size() - 1, offsets.data(), vec.size() / cols, cols, energy_col, energy_threshold, energy_mean_scale,
                               frames_context, proportion_threshold, mask.data(), counts ? counts->data() : nullptr));
    return mask;
}

// Kaldi select-voiced-frames on a packed block (ss_select_rows_packed): the rows whose mask byte is not 0, clip by clip in order (bit
// copies), and in `out_offsets` the table of the result.  `mask` is any byte mask with one entry per row, vad_energy_packed's or another
inline std::vector<float> select_rows_packed(const std::vector<float> &vec, const std::vector<int64_t> &offsets, size_t cols,
                                             const std::vector<uint8_t> &mask, std::vector<int64_t> &out_offsets)
{
    if (cols == 0 || vec.size() % cols || offsets.empty() || mask.size() != vec.size() / cols) throw Error(SS_ERR_ARG, "select_rows_packed: shape mismatch");
    std::vector<float> out(vec.size());
    out_offsets.assign(offsets.size(), 0);
    check(ss_select_rows_packed(vec.data(), offsets.size() - 1, offsets.data(), vec.size() / cols, cols, mask.data(), out_offsets.data(), out.data()));
    out.resize(static_cast<size_t>(out_offsets.back()) * cols);
    return out;
}

// The padded batch of a packed block (ss_pad_packed): [n_clips x max_rows x cols] (SS_PAD_BTC) or [n_clips x cols x max_rows]
// (SS_PAD_BCT) as raw bytes of `dtype` (SS_PAD_F32: bit copies; SS_PAD_F16 / SS_PAD_BF16: round to nearest even), clip b's first
// min(T_b, max_rows) rows with pad_value behind them, and in `lengths` the rows kept of every clip
inline std::vector<uint8_t> pad_packed(const std::vector<float> &vec, const std::vector<int64_t> &offsets, size_t cols, size_t max_rows,
                                       std::vector<int32_t> &lengths, int layout = SS_PAD_BTC, int dtype = SS_PAD_F32, float pad_value = 0.0f)
{
    if (cols == 0 || vec.size() % cols || offsets.empty()) throw Error(SS_ERR_ARG, "pad_packed: shape mismatch");
    size_t bytes = 0;
    check(ss_pad_packed_out_bytes(offsets.size() - 1, max_rows, cols, dtype, &bytes));
    std::vector<uint8_t> out(bytes);
    lengths.assign(offsets.size() - 1, 0);
    const float none = 0.0f;  // a block without rows still needs an address
    check(ss_pad_packed(vec.empty() ? &none : vec.data(), offsets.size() - 1, offsets.data(), vec.size() / cols, cols, max_rows, layout, dtype, pad_value,
                        out.data(), lengths.data()));
    return out;
}

// SpecAugment of a packed block (ss_specaug_*): n_time spans of at most min(max_time_width, time_ratio * T_b) rows and n_freq spans of
// at most max_freq_width columns of every clip are overwritten with mask_value; the spans are Philox4x32-10 draws of rng = {seed,
// epoch} and clip_base + b.  The defaults are the LibriSpeech policy.
struct SpecAugPolicy {
    size_t n_time = 2, max_time_width = 100;
    float time_ratio = 1.0f;
    size_t n_freq = 2, max_freq_width = 27;
    float mask_value = 0.0f;
    size_t clip_base = 0;
};

// the spans table [n_clips x (n_time + n_freq) x 2] of (start, width) pairs that spec_augment_packed draws: host only, no device
inline std::vector<int32_t> spec_augment_spans(const uint64_t (&rng)[2], const std::vector<int64_t> &offsets, size_t total_rows, size_t cols,
                                               const SpecAugPolicy &policy = SpecAugPolicy())
{
    if (offsets.empty()) throw Error(SS_ERR_ARG, "spec_augment_spans: shape mismatch");
    std::vector<int32_t> spans((offsets.size() - 1) * (policy.n_time + policy.n_freq) * 2);
    check(ss_specaug_spans(rng, policy.clip_base, offsets.size() - 1, offsets.data(), total_rows, cols, policy.n_time, policy.max_time_width, policy.time_ratio,
                           policy.n_freq, policy.max_freq_width, spans.data()));
    return spans;
}

// the block with the spans of `spans` overwritten (time spans first); a span outside its clip is skipped whole
inline std::vector<float> mask_spans_packed(const std::vector<float> &vec, const std::vector<int64_t> &offsets, size_t cols, const std::vector<int32_t> &spans,
                                            size_t n_time, size_t n_freq, float mask_value = 0.0f)
{
    if (cols == 0 || vec.size() % cols || offsets.empty() || spans.size() != (offsets.size() - 1) * (n_time + n_freq) * 2)
        throw Error(SS_ERR_ARG, "mask_spans_packed: shape mismatch");
    std::vector<float> out(vec);
    if (!vec.empty())
        check(ss_mask_spans_packed(vec.data(), offsets.size() - 1, offsets.data(), vec.size() / cols, cols, spans.data(), n_time, n_freq, mask_value, out.data()));
    return out;
}

// plan + apply; rng[1] (the epoch) is advanced by one and `spans` receives the table that was applied
inline std::vector<float> spec_augment_packed(const std::vector<float> &vec, const std::vector<int64_t> &offsets, size_t cols, uint64_t (&rng)[2],
                                              std::vector<int32_t> &spans, const SpecAugPolicy &policy = SpecAugPolicy())
{
    if (cols == 0 || vec.size() % cols || offsets.empty()) throw Error(SS_ERR_ARG, "spec_augment_packed: shape mismatch");
    std::vector<float> out(vec);
    spans.assign((offsets.size() - 1) * (policy.n_time + policy.n_freq) * 2, 0);
    const float none = 0.0f;  // a block without rows still needs an address
    float spare = 0.0f;
    check(ss_specaug_packed(vec.empty() ? &none : vec.data(), offsets.size() - 1, offsets.data(), vec.size() / cols, cols, rng, policy.clip_base, policy.n_time,
                            policy.max_time_width, policy.time_ratio, policy.n_freq, policy.max_freq_width, policy.mask_value,
                            vec.empty() ? &spare : out.data(), spans.data()));
    return out;
}

// Additive noise at a drawn SNR and gain perturbation of packed clips (ss_noise_*): with probability prob a clip gets a segment of a
// drawn clip of the bank at an SNR drawn from snr_db, and every clip a gain drawn from gain_db; the draws are Philox4x32-10 of rng =
// {seed, epoch} and clip_base + b.  The plan rows are ss_noise_plan_row of the C header.
using NoisePlanRow = ss_noise_plan_row;
static_assert(sizeof(NoisePlanRow) == 40 && alignof(NoisePlanRow) == 8, "ss_noise_plan_row is 40 bytes, 8-byte aligned");
struct NoisePolicy {
    float prob = 1.0f;
    float snr_lo_db = 10.0f, snr_hi_db = 30.0f;
    float gain_lo_db = 0.0f, gain_hi_db = 0.0f;
    size_t clip_base = 0;
};

// the draw fields of the plan noise_mix_packed writes (gains and energies 0): host only, no device
inline std::vector<NoisePlanRow> noise_draws(const uint64_t (&rng)[2], const std::vector<int64_t> &sample_offsets, size_t total_samples,
                                             const std::vector<int64_t> &noise_offsets, size_t total_noise, const NoisePolicy &policy = NoisePolicy())
{
    if (sample_offsets.empty() || noise_offsets.empty()) throw Error(SS_ERR_ARG, "noise_draws: shape mismatch");
    std::vector<NoisePlanRow> plan(sample_offsets.size() - 1);
    check(ss_noise_draws(rng, policy.clip_base, plan.size(), sample_offsets.data(), total_samples, noise_offsets.size() - 1, noise_offsets.data(), total_noise,
                         policy.prob, policy.snr_lo_db, policy.snr_hi_db, policy.gain_lo_db, policy.gain_hi_db, plan.data()));
    return plan;
}

// bytes of the caller-owned scratch of the device plan and mix forms
inline size_t noise_mix_work_bytes(size_t n_clips, size_t total_samples)
{
    size_t n = 0;
    check(ss_noise_mix_work_bytes(n_clips, total_samples, &n));
    return n;
}

// the mix alone, on any plan table: out[i] = fma(noise_gain, noise[(start + i) mod N], speech_gain * x[i])
inline std::vector<float> noise_apply_packed(const std::vector<float> &x, const std::vector<int64_t> &sample_offsets, const std::vector<float> &bank,
                                             const std::vector<int64_t> &noise_offsets, const std::vector<NoisePlanRow> &plan)
{
    if (sample_offsets.empty() || noise_offsets.empty() || plan.size() != sample_offsets.size() - 1) throw Error(SS_ERR_ARG, "noise_apply_packed: shape mismatch");
    std::vector<float> out(x);
    if (!x.empty())
        check(ss_noise_apply_packed(x.data(), plan.size(), sample_offsets.data(), x.size(), bank.data(), noise_offsets.size() - 1, noise_offsets.data(),
                                    bank.size(), plan.data(), out.data()));
    return out;
}

// ... on 16-bit PCM: a sample is pcm * scale, both scales powers of two; out is float
inline std::vector<float> noise_apply_packed_i16(const std::vector<int16_t> &x, float x_scale, const std::vector<int64_t> &sample_offsets,
                                                 const std::vector<int16_t> &bank, float noise_scale, const std::vector<int64_t> &noise_offsets,
                                                 const std::vector<NoisePlanRow> &plan)
{
    if (sample_offsets.empty() || noise_offsets.empty() || plan.size() != sample_offsets.size() - 1)
        throw Error(SS_ERR_ARG, "noise_apply_packed_i16: shape mismatch");
    std::vector<float> out(x.size());
    for (size_t i = 0; i < x.size(); ++i) out[i] = static_cast<float>(x[i]) * x_scale;  // samples in no clip: the converted signal
    if (!x.empty())
        check(ss_noise_apply_packed_i16(x.data(), x_scale, plan.size(), sample_offsets.data(), x.size(), bank.data(), noise_scale, noise_offsets.size() - 1,
                                        noise_offsets.data(), bank.size(), plan.data(), out.data()));
    return out;
}

// plan + apply; rng[1] (the epoch) is advanced by one and `plan` receives the table that was applied
inline std::vector<float> noise_mix_packed(const std::vector<float> &x, const std::vector<int64_t> &sample_offsets, const std::vector<float> &bank,
                                           const std::vector<int64_t> &noise_offsets, uint64_t (&rng)[2], std::vector<NoisePlanRow> &plan,
                                           const NoisePolicy &policy = NoisePolicy())
{
    if (sample_offsets.empty() || noise_offsets.empty()) throw Error(SS_ERR_ARG, "noise_mix_packed: shape mismatch");
    std::vector<float> out(x);
    plan.assign(sample_offsets.size() - 1, NoisePlanRow{});
    if (!x.empty())
        check(ss_noise_mix_packed(x.data(), plan.size(), sample_offsets.data(), x.size(), bank.data(), noise_offsets.size() - 1, noise_offsets.data(),
                                  bank.size(), rng, policy.clip_base, policy.prob, policy.snr_lo_db, policy.snr_hi_db, policy.gain_lo_db, policy.gain_hi_db,
                                  out.data(), plan.data()));
    return out;
}

inline std::vector<float> noise_mix_packed_i16(const std::vector<int16_t> &x, float x_scale, const std::vector<int64_t> &sample_offsets,
                                               const std::vector<int16_t> &bank, float noise_scale, const std::vector<int64_t> &noise_offsets,
                                               uint64_t (&rng)[2], std::vector<NoisePlanRow> &plan, const NoisePolicy &policy = NoisePolicy())
{
    if (sample_offsets.empty() || noise_offsets.empty()) throw Error(SS_ERR_ARG, "noise_mix_packed_i16: shape mismatch");
    std::vector<float> out(x.size());
    for (size_t i = 0; i < x.size(); ++i) out[i] = static_cast<float>(x[i]) * x_scale;
    plan.assign(sample_offsets.size() - 1, NoisePlanRow{});
    if (!x.empty())
        check(ss_noise_mix_packed_i16(x.data(), x_scale, plan.size(), sample_offsets.data(), x.size(), bank.data(), noise_scale, noise_offsets.size() - 1,
                                      noise_offsets.data(), bank.size(), rng, policy.clip_base, policy.prob, policy.snr_lo_db, policy.snr_hi_db,
                                      policy.gain_lo_db, policy.gain_hi_db, out.data(), plan.data()));
    return out;
}

// Reverberation of packed clips from a bank of room impulse responses (ss_reverb_*): with probability prob a clip is convolved with a
// drawn response, out[i] = sum_k h[k] x[i + shift - k], the clip's length kept; the draws are Philox4x32-10 of rng = {seed, epoch} and
// clip_base + b (counter word 0x30000: one block may serve SpecAugment, the noise stage and this one).  The handle is shared by
// copies; the first call that runs uploads the partition spectra.
using ReverbPlanRow = ss_reverb_plan_row;
static_assert(sizeof(ReverbPlanRow) == 8, "ss_reverb_plan_row is 8 bytes");
class ReverbBank {
public:
    enum Normalize { kAsGiven = 0, kUnitEnergy = 1, kUnitPeak = 2 };
    // rirs: the responses packed; offsets: n_rir + 1 entries from 0; every response has 1 .. 16384 finite taps
    ReverbBank(const std::vector<float> &rirs, const std::vector<int64_t> &offsets, Normalize normalize = kUnitEnergy, bool align_peak = true)
    {
        if (offsets.empty()) throw Error(SS_ERR_ARG, "ReverbBank: shape mismatch");
        ss_reverb_bank *raw = nullptr;
        check(ss_reverb_bank_create(rirs.data(), offsets.size() - 1, offsets.data(), rirs.size(), static_cast<int>(normalize), align_peak ? 1 : 0, &raw));
        h_ = std::shared_ptr<ss_reverb_bank>(raw, ss_reverb_bank_destroy);
    }
    const ss_reverb_bank *handle() const { return h_.get(); }
    size_t size() const { return info(0); }
    size_t block() const { return info(1); }
    size_t max_taps() const { return info(2); }
    size_t partitions() const { return info(3); }
    // the normalised taps of response c as the spectra were made from them, and the first index of their largest magnitude
    std::vector<float> rir(size_t c, size_t *peak = nullptr) const
    {
        size_t n = 0, pk = 0;
        check(ss_reverb_bank_rir(h_.get(), c, nullptr, 0, &n, &pk));
        std::vector<float> taps(n);
        check(ss_reverb_bank_rir(h_.get(), c, taps.data(), taps.size(), &n, &pk));
        if (peak) *peak = pk;
        return taps;
    }
    // partition p of response c: 2 * 2 * block() floats, (re, im) of bin 0 first
    std::vector<float> spectrum(size_t c, size_t p) const
    {
        std::vector<float> out(4 * block());
        check(ss_reverb_bank_spectrum(h_.get(), c, p, out.data()));
        return out;
    }

private:
    size_t info(int which) const
    {
        size_t v[4] = {0, 0, 0, 0};
        check(ss_reverb_bank_info(h_.get(), &v[0], &v[1], &v[2], &v[3]));
        return v[which];
    }
    std::shared_ptr<ss_reverb_bank> h_;
};

// the plan reverb_packed writes: host only, no device
inline std::vector<ReverbPlanRow> reverb_draws(const uint64_t (&rng)[2], const std::vector<int64_t> &sample_offsets, size_t total_samples, const ReverbBank &bank,
                                               float prob = 1.0f, size_t clip_base = 0)
{
    if (sample_offsets.empty()) throw Error(SS_ERR_ARG, "reverb_draws: shape mismatch");
    std::vector<ReverbPlanRow> plan(sample_offsets.size() - 1);
    check(ss_reverb_draws(rng, clip_base, plan.size(), sample_offsets.data(), total_samples, bank.handle(), prob, plan.data()));
    return plan;
}

// the convolution alone, on any plan table; rows with rir == -1 (or out of range for the bank) are copies
inline std::vector<float> reverb_apply_packed(const std::vector<float> &x, const std::vector<int64_t> &sample_offsets, const ReverbBank &bank,
                                              const std::vector<ReverbPlanRow> &plan)
{
    if (sample_offsets.empty() || plan.size() != sample_offsets.size() - 1) throw Error(SS_ERR_ARG, "reverb_apply_packed: shape mismatch");
    std::vector<float> out(x);
    if (!x.empty()) check(ss_reverb_apply_packed(x.data(), plan.size(), sample_offsets.data(), x.size(), bank.handle(), plan.data(), out.data()));
    return out;
}

// ... on 16-bit PCM: a sample is pcm * x_scale, a power of two; out is float
inline std::vector<float> reverb_apply_packed_i16(const std::vector<int16_t> &x, float x_scale, const std::vector<int64_t> &sample_offsets, const ReverbBank &bank,
                                                  const std::vector<ReverbPlanRow> &plan)
{
    if (sample_offsets.empty() || plan.size() != sample_offsets.size() - 1) throw Error(SS_ERR_ARG, "reverb_apply_packed_i16: shape mismatch");
    std::vector<float> out(x.size());
    for (size_t i = 0; i < x.size(); ++i) out[i] = static_cast<float>(x[i]) * x_scale;  // samples in no clip: the converted signal
    if (!x.empty()) check(ss_reverb_apply_packed_i16(x.data(), x_scale, plan.size(), sample_offsets.data(), x.size(), bank.handle(), plan.data(), out.data()));
    return out;
}

// plan + apply; rng[1] (the epoch) is advanced by one and `plan` receives the table that was applied
inline std::vector<float> reverb_packed(const std::vector<float> &x, const std::vector<int64_t> &sample_offsets, const ReverbBank &bank, uint64_t (&rng)[2],
                                        std::vector<ReverbPlanRow> &plan, float prob = 1.0f, size_t clip_base = 0)
{
    if (sample_offsets.empty()) throw Error(SS_ERR_ARG, "reverb_packed: shape mismatch");
    std::vector<float> out(x);
    plan.assign(sample_offsets.size() - 1, ReverbPlanRow{});
    if (!x.empty()) check(ss_reverb_packed(x.data(), plan.size(), sample_offsets.data(), x.size(), bank.handle(), rng, clip_base, prob, out.data(), plan.data()));
    return out;
}

inline std::vector<float> reverb_packed_i16(const std::vector<int16_t> &x, float x_scale, const std::vector<int64_t> &sample_offsets, const ReverbBank &bank,
                                            uint64_t (&rng)[2], std::vector<ReverbPlanRow> &plan, float prob = 1.0f, size_t clip_base = 0)
{
    if (sample_offsets.empty()) throw Error(SS_ERR_ARG, "reverb_packed_i16: shape mismatch");
    std::vector<float> out(x.size());
    for (size_t i = 0; i < x.size(); ++i) out[i] = static_cast<float>(x[i]) * x_scale;
    plan.assign(sample_offsets.size() - 1, ReverbPlanRow{});
    if (!x.empty())
        check(ss_reverb_packed_i16(x.data(), x_scale, plan.size(), sample_offsets.data(), x.size(), bank.handle(), rng, clip_base, prob, out.data(), plan.data()));
    return out;
}

inline std::vector<float> cmvnw_packed(const std::vector<float> &vec, const std::vector<int64_t> &offsets, size_t cols, size_t win_size = 301,
                                       bool variance_normalization = false)
{
    if (cols == 0 || vec.size() % cols || offsets.empty()) throw Error(SS_ERR_ARG, "cmvnw_packed: shape mismatch");
    std::vector<float> out(vec.size());
    check(ss_cmvnw_packed(vec.data(), offsets.size() - 1, offsets.data(), vec.size() / cols, cols, win_size, variance_normalization ? 1 : 0,
                          out.data()));
    return out;
}

// top_db < 0: no floor
inline std::vector<float> power_to_db_packed(const std::vector<float> &s, const std::vector<int64_t> &offsets, size_t cols, float ref = 1.0f,
                                             float amin = 1e-10f, float top_db = 80.0f)
{
    if (cols == 0 || s.size() % cols || offsets.empty()) throw Error(SS_ERR_ARG, "power_to_db_packed: shape mismatch");
    std::vector<float> out(s.size());
    check(ss_power_to_db_packed(s.data(), offsets.size() - 1, offsets.data(), s.size() / cols, cols, ref, amin, top_db, out.data()));
    return out;
}

// Polyphase windowed-sinc resampler for one pair of rates (ss_resample*; not in the reference crate): torchaudio's default
// sinc_interp_hann filter.  The handle is shared by copies; the first call that runs uploads its table.
class Resampler {
public:
    Resampler(uint32_t orig_rate, uint32_t new_rate, uint32_t lowpass_filter_width = 6, float rolloff = 0.99f) : orig_(orig_rate), new_(new_rate)
    {
        ss_resampler *raw = nullptr;
        check(ss_resampler_create(orig_rate, new_rate, lowpass_filter_width, rolloff, &raw));
        h_ = std::shared_ptr<ss_resampler>(raw, ss_resampler_destroy);
        check(ss_resampler_info(raw, &info_));
    }
    const ss_resample_info &info() const { return info_; }
    const ss_resampler *handle() const { return h_.get(); }
    size_t out_len(size_t n_samples) const { return (n_samples * info_.n + info_.o - 1) / info_.o; }
    // one clip -> its out_len(x.size()) resampled samples
    std::vector<float> resample(const std::vector<float> &x) const
    {
        std::vector<float> out(out_len(x.size()));
        check(ss_resample(h_.get(), x.data(), 1, x.size(), x.size(), out.data(), out.size()));
        return out;
    }
    // clips packed end to end, clip b = x[sample_offsets[b] .. sample_offsets[b+1]) -> the resampled block; out_offsets receives
    // its offsets, which are the sample_offsets of the packed feature calls on that block
    std::vector<float> resample_packed(const std::vector<float> &x, const std::vector<int64_t> &sample_offsets, std::vector<int64_t> &out_offsets) const
    {
        if (sample_offsets.empty() || sample_offsets.back() < 0 || static_cast<size_t>(sample_offsets.back()) > x.size())
            throw Error(SS_ERR_ARG, "resample_packed: shape mismatch");
        out_offsets.assign(sample_offsets.size(), 0);
        check(ss_resample_packed_offsets(orig_, new_, sample_offsets.size() - 1, sample_offsets.data(), out_offsets.data()));
        std::vector<float> out(static_cast<size_t>(out_offsets.back()));
        check(ss_resample_packed(h_.get(), x.data(), sample_offsets.size() - 1, sample_offsets.data(), out_offsets.data(), out.data()));
        return out;
    }

private:
    uint32_t orig_, new_;
    std::shared_ptr<ss_resampler> h_;
    ss_resample_info info_{};
};

// Kaldi's compute-fbank-feats / compute-mfcc-feats as torchaudio.compliance.kaldi restates them (ss_kaldi_*; not in the reference
// crate), for frames that pad to 512 points.  The handle is shared by copies.
inline ss_kaldi_params kaldi_params(uint32_t sample_rate)  // torchaudio's defaults
{
    ss_kaldi_params p;
    check(ss_kaldi_params_default(&p, sample_rate));
    return p;
}
class KaldiFrontEnd {
public:
    explicit KaldiFrontEnd(const ss_kaldi_params &p) : p_(p)
    {
        ss_kaldi_config *raw = nullptr;
        check(ss_kaldi_config_create(&p, &raw));
        h_ = std::shared_ptr<ss_kaldi_config>(raw, ss_kaldi_config_destroy);
    }
    const ss_kaldi_params &params() const { return p_; }
    const ss_kaldi_config *handle() const { return h_.get(); }
    size_t num_frames(size_t n_samples) const
    {
        size_t t = 0;
        check(ss_kaldi_num_frames(&p_, n_samples, &t));
        return t;
    }
    // one clip -> [T x num_mel_bins] log-mel rows; log_energy (may be null) receives the [T] log energies
    std::vector<float> fbank(const std::vector<float> &x, std::vector<float> *log_energy = nullptr) const
    {
        const size_t t = num_frames(x.size());
        std::vector<float> out(t * p_.num_mel_bins);
        if (log_energy) log_energy->assign(t, 0.0f);
        check(ss_kaldi_fbank(h_.get(), x.data(), 1, x.size(), x.size(), out.data(), log_energy ? log_energy->data() : nullptr));
        return out;
    }
    // one clip -> [T x num_ceps] cepstra
    std::vector<float> mfcc(const std::vector<float> &x) const
    {
        std::vector<float> out(num_frames(x.size()) * p_.num_ceps);
        check(ss_kaldi_mfcc(h_.get(), x.data(), 1, x.size(), x.size(), out.data()));
        return out;
    }
    // clips packed end to end, clip b = x[sample_offsets[b] .. sample_offsets[b+1]) -> the [sum T_b x cols] rows; frame_offsets
    // receives the row offsets
    std::vector<float> fbank_packed(const std::vector<float> &x, const std::vector<int64_t> &sample_offsets, std::vector<int64_t> &frame_offsets,
                                    std::vector<float> *log_energy = nullptr) const
    {
        const size_t rows = packed_rows(x, sample_offsets, frame_offsets);
        std::vector<float> out(rows * p_.num_mel_bins);
        if (log_energy) log_energy->assign(rows, 0.0f);
        check(ss_kaldi_fbank_packed(h_.get(), x.data(), sample_offsets.size() - 1, sample_offsets.data(), out.data(),
                                    log_energy ? log_energy->data() : nullptr));
        return out;
    }
    std::vector<float> mfcc_packed(const std::vector<float> &x, const std::vector<int64_t> &sample_offsets, std::vector<int64_t> &frame_offsets) const
    {
        std::vector<float> out(packed_rows(x, sample_offsets, frame_offsets) * p_.num_ceps);
        check(ss_kaldi_mfcc_packed(h_.get(), x.data(), sample_offsets.size() - 1, sample_offsets.data(), out.data()));
        return out;
    }
    // The same four calls fed signed 16-bit PCM (ss_kpcm_*): sample = pcm * scale, scale a power of two (1.0: Kaldi's integer-valued
    // samples, 2^-15: normalised ones); bit for bit the float call on the converted samples
    std::vector<float> fbank_i16(const std::vector<int16_t> &x, float scale, std::vector<float> *log_energy = nullptr) const
    {
        const size_t t = num_frames(x.size());
        std::vector<float> out(t * p_.num_mel_bins);
        if (log_energy) log_energy->assign(t, 0.0f);
        check(ss_kpcm_fbank(h_.get(), x.data(), 1, x.size(), x.size(), scale, out.data(), log_energy ? log_energy->data() : nullptr));
        return out;
    }
    std::vector<float> mfcc_i16(const std::vector<int16_t> &x, float scale) const
    {
        std::vector<float> out(num_frames(x.size()) * p_.num_ceps);
        check(ss_kpcm_mfcc(h_.get(), x.data(), 1, x.size(), x.size(), scale, out.data()));
        return out;
    }
    std::vector<float> fbank_packed_i16(const std::vector<int16_t> &x, const std::vector<int64_t> &sample_offsets, float scale,
                                        std::vector<int64_t> &frame_offsets, std::vector<float> *log_energy = nullptr) const
    {
        const size_t rows = packed_rows(x, sample_offsets, frame_offsets);
        std::vector<float> out(rows * p_.num_mel_bins);
        if (log_energy) log_energy->assign(rows, 0.0f);
        check(ss_kpcm_fbank_packed(h_.get(), x.data(), sample_offsets.size() - 1, sample_offsets.data(), scale, out.data(),
                                   log_energy ? log_energy->data() : nullptr));
        return out;
    }
    std::vector<float> mfcc_packed_i16(const std::vector<int16_t> &x, const std::vector<int64_t> &sample_offsets, float scale,
                                       std::vector<int64_t> &frame_offsets) const
    {
        std::vector<float> out(packed_rows(x, sample_offsets, frame_offsets) * p_.num_ceps);
        check(ss_kpcm_mfcc_packed(h_.get(), x.data(), sample_offsets.size() - 1, sample_offsets.data(), scale, out.data()));
        return out;
    }

    // The stream pool (ss_kstream_*): S = the floats of a pool row, D = the warm-up rows after a reset.
    size_t stream_state_len(size_t *delay_rows = nullptr) const
    {
        size_t S = 0, D = 0;
        check(ss_kstream_state_len(&p_, &S, &D));
        if (delay_rows) *delay_rows = D;
        return S;
    }
    // Entry i is the chunk x[sample_offsets[i] .. sample_offsets[i+1]) (whole hops, floats or 16-bit PCM times the power-of-two
    // `scale`) of the stream whose state is row slots[i] of pool [pool_streams x S] (all-zero rows: fresh streams) -> the packed
    // rows; row_offsets receives the entries' row offsets.  The first D rows of a fresh stream are warm-up rows.
    std::vector<float> fbank_stream_packed(const std::vector<float> &x, const std::vector<int64_t> &sample_offsets, const std::vector<int32_t> &slots,
                                           std::vector<float> &pool, std::vector<int64_t> &row_offsets, std::vector<float> *log_energy = nullptr) const
    {
        const size_t rows = stream_rows(x.size(), sample_offsets, slots, row_offsets);
        std::vector<float> out(rows * p_.num_mel_bins);
        if (log_energy) log_energy->assign(rows, 0.0f);
        check(ss_kstream_fbank_packed(h_.get(), x.data(), slots.size(), sample_offsets.data(), slots.data(), pool_rows(pool, slots), pool.data(),
                                      out.data(), log_energy ? log_energy->data() : nullptr));
        return out;
    }
    std::vector<float> mfcc_stream_packed(const std::vector<float> &x, const std::vector<int64_t> &sample_offsets, const std::vector<int32_t> &slots,
                                          std::vector<float> &pool, std::vector<int64_t> &row_offsets) const
    {
        std::vector<float> out(stream_rows(x.size(), sample_offsets, slots, row_offsets) * p_.num_ceps);
        check(ss_kstream_mfcc_packed(h_.get(), x.data(), slots.size(), sample_offsets.data(), slots.data(), pool_rows(pool, slots), pool.data(),
                                     out.data()));
        return out;
    }
    std::vector<float> fbank_stream_packed_i16(const std::vector<int16_t> &x, const std::vector<int64_t> &sample_offsets,
                                               const std::vector<int32_t> &slots, float scale, std::vector<float> &pool,
                                               std::vector<int64_t> &row_offsets, std::vector<float> *log_energy = nullptr) const
    {
        const size_t rows = stream_rows(x.size(), sample_offsets, slots, row_offsets);
        std::vector<float> out(rows * p_.num_mel_bins);
        if (log_energy) log_energy->assign(rows, 0.0f);
        check(ss_kstream_fbank_packed_i16(h_.get(), x.data(), slots.size(), sample_offsets.data(), slots.data(), pool_rows(pool, slots), scale,
                                          pool.data(), out.data(), log_energy ? log_energy->data() : nullptr));
        return out;
    }
    std::vector<float> mfcc_stream_packed_i16(const std::vector<int16_t> &x, const std::vector<int64_t> &sample_offsets,
                                              const std::vector<int32_t> &slots, float scale, std::vector<float> &pool,
                                              std::vector<int64_t> &row_offsets) const
    {
        std::vector<float> out(stream_rows(x.size(), sample_offsets, slots, row_offsets) * p_.num_ceps);
        check(ss_kstream_mfcc_packed_i16(h_.get(), x.data(), slots.size(), sample_offsets.data(), slots.data(), pool_rows(pool, slots), scale,
                                         pool.data(), out.data()));
        return out;
    }

private:
    size_t stream_rows(size_t n_samples, const std::vector<int64_t> &sample_offsets, const std::vector<int32_t> &slots,
                       std::vector<int64_t> &row_offsets) const
    {
        if (sample_offsets.size() != slots.size() + 1 || sample_offsets.back() < 0 || static_cast<size_t>(sample_offsets.back()) > n_samples)
            throw Error(SS_ERR_ARG, "kaldi pool call: shape mismatch");
        row_offsets.assign(sample_offsets.size(), 0);
        check(ss_kstream_row_offsets(&p_, slots.size(), sample_offsets.data(), row_offsets.data()));
        return static_cast<size_t>(row_offsets.back());
    }
    // the pool's row count (S == 0, a pool without state: one more than the largest slot)
    size_t pool_rows(const std::vector<float> &pool, const std::vector<int32_t> &slots) const
    {
        const size_t S = stream_state_len();
        if (S > 0) {
            if (pool.empty() || pool.size() % S) throw Error(SS_ERR_ARG, "kaldi pool call: the pool is not a whole number of rows");
            return pool.size() / S;
        }
        int32_t top = 0;
        for (int32_t v : slots) top = v > top ? v : top;
        return static_cast<size_t>(top) + 1;
    }
    template <typename T>  // T: float, or int16_t (the _i16 forms)
    size_t packed_rows(const std::vector<T> &x, const std::vector<int64_t> &sample_offsets, std::vector<int64_t> &frame_offsets) const
    {
        if (sample_offsets.empty() || sample_offsets.back() < 0 || static_cast<size_t>(sample_offsets.back()) > x.size())
            throw Error(SS_ERR_ARG, "kaldi packed call: shape mismatch");
        frame_offsets.assign(sample_offsets.size(), 0);
        check(ss_kaldi_packed_frame_offsets(&p_, sample_offsets.size() - 1, sample_offsets.data(), frame_offsets.data()));
        return static_cast<size_t>(frame_offsets.back());
    }
    ss_kaldi_params p_;
    std::shared_ptr<ss_kaldi_config> h_;
};

// The Whisper log-mel block (ss_whisper_*; not in the reference crate): [n_mels x n_frames] per clip, every clip padded or trimmed to
// n_frames * 160 samples.  The handle is shared by copies; calls on one handle must be ordered on one stream.
inline ss_whisper_params whisper_params(uint32_t n_mels)  // 16000 / 400 / 160
{
    ss_whisper_params p;
    check(ss_whisper_params_default(&p, n_mels));
    return p;
}
class WhisperFrontEnd {
public:
    explicit WhisperFrontEnd(uint32_t n_mels = 80) : p_(whisper_params(n_mels))
    {
        ss_whisper_config *raw = nullptr;
        check(ss_whisper_config_create(&p_, &raw));
        h_ = std::shared_ptr<ss_whisper_config>(raw, ss_whisper_config_destroy);
    }
    const ss_whisper_params &params() const { return p_; }
    const ss_whisper_config *handle() const { return h_.get(); }
    static size_t num_frames(size_t n_samples)  // n_samples / 160
    {
        size_t t = 0;
        check(ss_whisper_num_frames(n_samples, &t));
        return t;
    }
    // bytes of f32 scratch the device calls take for a 16-bit dtype (0 for SS_PAD_F32)
    size_t work_bytes(size_t batch, size_t n_frames, int dtype) const
    {
        size_t n = 0;
        check(ss_whisper_work_bytes(&p_, batch, n_frames, dtype, &n));
        return n;
    }
    // throws Error(SS_ERR_DEVICE) once if a packed launch has met a bad table entry since the last look
    void device_status() const { check(ss_whisper_config_device_status(h_.get())); }
    // one clip -> [n_mels x n_frames], f32
    std::vector<float> log_mel(const std::vector<float> &x, size_t n_frames) const
    {
        std::vector<float> out(p_.n_mels * n_frames);
        const float keep[4] = {0, 0, 0, 0};  // an empty clip reads nothing: any address will do
        check(ss_whisper_log_mel(h_.get(), x.empty() ? keep : x.data(), 1, x.size(), x.size(), n_frames, SS_PAD_F32, out.data()));
        return out;
    }
    // clips packed end to end, clip b = x[sample_offsets[b] .. sample_offsets[b+1]) -> [n_clips x n_mels x n_frames]; lengths (may be
    // null) receives min(len_b / 160, n_frames)
    std::vector<float> log_mel_packed(const std::vector<float> &x, const std::vector<int64_t> &sample_offsets, size_t n_frames,
                                      std::vector<int32_t> *lengths = nullptr) const
    {
        if (sample_offsets.empty() || sample_offsets.back() < 0 || static_cast<size_t>(sample_offsets.back()) > x.size())
            throw Error(SS_ERR_ARG, "whisper packed call: shape mismatch");
        const size_t n = sample_offsets.size() - 1;
        std::vector<float> out(n * p_.n_mels * n_frames);
        if (lengths) lengths->assign(n, 0);
        const float keep[4] = {0, 0, 0, 0};
        check(ss_whisper_log_mel_packed(h_.get(), x.empty() ? keep : x.data(), n, sample_offsets.data(), n_frames, SS_PAD_F32, out.data(),
                                        lengths ? lengths->data() : nullptr));
        return out;
    }
    // the device calls on `stream`: device pointers, nothing is copied or allocated
    void log_mel_device(const float *d_x, size_t batch, size_t n_samples, size_t ld, size_t n_frames, int dtype, void *d_work, void *d_out,
                        void *stream) const
    {
        check(ss_whisper_log_mel_device(h_.get(), d_x, batch, n_samples, ld, n_frames, dtype, d_work, d_out, stream));
    }
    void log_mel_packed_device(const float *d_x, size_t n_clips, const int64_t *d_sample_offsets, size_t n_frames, int dtype, void *d_work, void *d_out,
                               int32_t *d_lengths, void *stream) const
    {
        check(ss_whisper_log_mel_packed_device(h_.get(), d_x, n_clips, d_sample_offsets, n_frames, dtype, d_work, d_out, d_lengths, stream));
    }
    // The same four calls fed signed 16-bit PCM: sample = pcm * scale, scale a power of two (2^-15: Whisper's convention); bit for bit
    // the float call on the converted samples
    std::vector<float> log_mel_i16(const std::vector<int16_t> &x, float scale, size_t n_frames) const
    {
        std::vector<float> out(p_.n_mels * n_frames);
        const int16_t keep[4] = {0, 0, 0, 0};
        check(ss_whisper_log_mel_i16(h_.get(), x.empty() ? keep : x.data(), 1, x.size(), x.size(), scale, n_frames, SS_PAD_F32, out.data()));
        return out;
    }
    std::vector<float> log_mel_packed_i16(const std::vector<int16_t> &x, const std::vector<int64_t> &sample_offsets, float scale, size_t n_frames,
                                          std::vector<int32_t> *lengths = nullptr) const
    {
        if (sample_offsets.empty() || sample_offsets.back() < 0 || static_cast<size_t>(sample_offsets.back()) > x.size())
            throw Error(SS_ERR_ARG, "whisper packed call: shape mismatch");
        const size_t n = sample_offsets.size() - 1;
        std::vector<float> out(n * p_.n_mels * n_frames);
        if (lengths) lengths->assign(n, 0);
        const int16_t keep[4] = {0, 0, 0, 0};
        check(ss_whisper_log_mel_packed_i16(h_.get(), x.empty() ? keep : x.data(), n, sample_offsets.data(), scale, n_frames, SS_PAD_F32, out.data(),
                                            lengths ? lengths->data() : nullptr));
        return out;
    }
    void log_mel_i16_device(const int16_t *d_x, size_t batch, size_t n_samples, size_t ld, float scale, size_t n_frames, int dtype, void *d_work,
                            void *d_out, void *stream) const
    {
        check(ss_whisper_log_mel_i16_device(h_.get(), d_x, batch, n_samples, ld, scale, n_frames, dtype, d_work, d_out, stream));
    }
    void log_mel_packed_i16_device(const int16_t *d_x, size_t n_clips, const int64_t *d_sample_offsets, float scale, size_t n_frames, int dtype,
                                   void *d_work, void *d_out, int32_t *d_lengths, void *stream) const
    {
        check(ss_whisper_log_mel_packed_i16_device(h_.get(), d_x, n_clips, d_sample_offsets, scale, n_frames, dtype, d_work, d_out, d_lengths, stream));
    }

private:
    ss_whisper_params p_;
    std::shared_ptr<ss_whisper_config> h_;
};

// The NeMo / Parakeet log-mel rows (ss_nemo_*; not in the reference crate): [len / 160 x n_mels] per clip, packed rows for clips of
// different lengths.
inline ss_nemo_params nemo_params(uint32_t n_mels)  // 16000 / 512 / 400 / 160, pre-emphasis 0.97, per-feature normalisation
{
    ss_nemo_params p;
    check(ss_nemo_params_default(&p, n_mels));
    return p;
}
class NemoFrontEnd {
public:
    explicit NemoFrontEnd(const ss_nemo_params &p) : p_(p)
    {
        ss_nemo_config *raw = nullptr;
        check(ss_nemo_config_create(&p_, &raw));
        h_ = std::shared_ptr<ss_nemo_config>(raw, ss_nemo_config_destroy);
    }
    explicit NemoFrontEnd(uint32_t n_mels = 80) : NemoFrontEnd(nemo_params(n_mels)) {}
    const ss_nemo_params &params() const { return p_; }
    const ss_nemo_config *handle() const { return h_.get(); }
    // n_samples / 160: the rows kept of a clip (0 for a clip shorter than one hop)
    size_t num_frames(size_t n_samples) const
    {
        size_t t = 0;
        check(ss_nemo_num_frames(&p_, n_samples, &t));
        return t;
    }
    // SS_ERR_DEVICE once if a packed launch has skipped an inconsistent clip since the last look
    void device_status() const { check(ss_nemo_config_device_status(h_.get())); }
    // one clip -> [len / 160 x n_mels]
    std::vector<float> log_mel(const std::vector<float> &x) const
    {
        std::vector<float> out(num_frames(x.size()) * p_.n_mels);
        if (!out.empty()) check(ss_nemo_log_mel(h_.get(), x.data(), 1, x.size(), x.size(), out.data()));
        return out;
    }
    // clips packed end to end, clip b = x[sample_offsets[b] .. sample_offsets[b+1]) -> the rows [sum T_b x n_mels]; frame_offsets (may
    // be null) receives the n_clips + 1 row offsets
    std::vector<float> log_mel_packed(const std::vector<float> &x, const std::vector<int64_t> &sample_offsets,
                                      std::vector<int64_t> *frame_offsets = nullptr) const
    {
        if (sample_offsets.empty() || sample_offsets.back() < 0 || static_cast<size_t>(sample_offsets.back()) > x.size())
            throw Error(SS_ERR_ARG, "nemo packed call: shape mismatch");
        const size_t n = sample_offsets.size() - 1;
        std::vector<int64_t> fo(n + 1);
        check(ss_nemo_packed_frame_offsets(&p_, n, sample_offsets.data(), fo.data()));
        std::vector<float> out(static_cast<size_t>(fo[n]) * p_.n_mels);
        if (!out.empty()) check(ss_nemo_log_mel_packed(h_.get(), x.data(), n, sample_offsets.data(), out.data()));
        if (frame_offsets) *frame_offsets = fo;
        return out;
    }
    // the device calls on `stream`: device pointers, nothing is copied or allocated
    void log_mel_device(const float *d_x, size_t batch, size_t n_samples, size_t ld, float *d_out, void *stream) const
    {
        check(ss_nemo_log_mel_device(h_.get(), d_x, batch, n_samples, ld, d_out, stream));
    }
    void log_mel_packed_device(const float *d_x, size_t n_clips, const int64_t *d_sample_offsets, const int64_t *d_frame_offsets,
                               size_t total_frames, float *d_out, void *stream) const
    {
        check(ss_nemo_log_mel_packed_device(h_.get(), d_x, n_clips, d_sample_offsets, d_frame_offsets, total_frames, d_out, stream));
    }

    // The stream pool (ss_nstream_*; a handle with normalize none): S = the floats of a pool row, L = the warm-up rows after a reset
    // and the rows a flush returns per stream.
    size_t stream_state_len(size_t *delay_rows = nullptr) const
    {
        size_t S = 0, L = 0;
        check(ss_nstream_state_len(&p_, &S, &L));
        if (delay_rows) *delay_rows = L;
        return S;
    }
    // Entry i is the chunk x[sample_offsets[i] .. sample_offsets[i+1]) (whole 160-sample hops, floats or 16-bit PCM times the
    // power-of-two `scale`) of the stream whose state is row slots[i] of pool [pool_streams x S] (all-zero rows: fresh streams) -> the
    // packed rows; row_offsets receives the entries' row offsets.  The first L rows of a fresh stream are warm-up rows.
    std::vector<float> log_mel_stream_packed(const std::vector<float> &x, const std::vector<int64_t> &sample_offsets, const std::vector<int32_t> &slots,
                                             std::vector<float> &pool, std::vector<int64_t> &row_offsets) const
    {
        std::vector<float> out(stream_rows(x.size(), sample_offsets, slots, row_offsets) * p_.n_mels);
        check(ss_nstream_log_mel_packed(h_.get(), x.data(), slots.size(), sample_offsets.data(), slots.data(), pool_rows(pool), pool.data(),
                                        out.data()));
        return out;
    }
    std::vector<float> log_mel_stream_packed_i16(const std::vector<int16_t> &x, const std::vector<int64_t> &sample_offsets,
                                                 const std::vector<int32_t> &slots, float scale, std::vector<float> &pool,
                                                 std::vector<int64_t> &row_offsets) const
    {
        std::vector<float> out(stream_rows(x.size(), sample_offsets, slots, row_offsets) * p_.n_mels);
        check(ss_nstream_log_mel_packed_i16(h_.get(), x.data(), slots.size(), sample_offsets.data(), slots.data(), pool_rows(pool), scale,
                                            pool.data(), out.data()));
        return out;
    }
    // the end of the named streams -> [slots.size() * L x n_mels], stream i's last L rows at rows i * L ..; the named pool rows are zero
    // (fresh streams) afterwards
    std::vector<float> stream_flush(const std::vector<int32_t> &slots, std::vector<float> &pool) const
    {
        size_t L = 0;
        stream_state_len(&L);
        std::vector<float> out(slots.size() * L * p_.n_mels);
        check(ss_nstream_flush(h_.get(), slots.size(), slots.data(), pool_rows(pool), pool.data(), out.data()));
        return out;
    }

private:
    size_t stream_rows(size_t n_samples, const std::vector<int64_t> &sample_offsets, const std::vector<int32_t> &slots,
                       std::vector<int64_t> &row_offsets) const
    {
        if (sample_offsets.size() != slots.size() + 1 || sample_offsets.back() < 0 || static_cast<size_t>(sample_offsets.back()) > n_samples)
            throw Error(SS_ERR_ARG, "nemo pool call: shape mismatch");
        row_offsets.assign(sample_offsets.size(), 0);
        check(ss_nstream_row_offsets(&p_, slots.size(), sample_offsets.data(), row_offsets.data()));
        return static_cast<size_t>(row_offsets.back());
    }
    size_t pool_rows(const std::vector<float> &pool) const
    {
        const size_t S = stream_state_len();
        if (pool.empty() || pool.size() % S) throw Error(SS_ERR_ARG, "nemo pool call: the pool is not a whole number of rows");
        return pool.size() / S;
    }
    ss_nemo_params p_;
    std::shared_ptr<ss_nemo_config> h_;
};

// processing.rs:222-254
inline std::vector<float> derivative_extraction(const std::vector<float> &feat, size_t rows, size_t cols, size_t delta_windows)
{
    if (feat.size() != rows * cols) throw Error(SS_ERR_ARG, "derivative_extraction: shape mismatch");
    std::vector<float> out(feat.size());
    check(ss_derivative_extraction(feat.data(), rows, cols, delta_windows, out.data()));
    return out;
}

// feature.rs:253-269: [rows x cols x 3]
inline std::vector<float> extract_derivative_feature(const std::vector<float> &feature, size_t rows, size_t cols)
{
    if (feature.size() != rows * cols) throw Error(SS_ERR_ARG, "extract_derivative_feature: shape mismatch");
    std::vector<float> cube(3 * feature.size());
    check(ss_extract_derivative_feature(feature.data(), rows, cols, cube.data()));
    return cube;
}

}  // namespace speechsauce
