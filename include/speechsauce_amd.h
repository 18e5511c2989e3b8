/*
 * speechsauce_amd.h -- C ABI of the MI355X-native MFCC / mel-spectrogram hot path.
 *
 * The reference crate (secretsauceai/mfcc-rust, `speechsauce`) has no FFI of its own: the path
 * sits behind plain Rust functions and a PyO3 module.  This header is the `extern "C"` layer a
 * maintainer binds instead of those functions; every entry point cites the reference item it
 * replaces (paths relative to the reference checkout).  INTEGRATION.md shows the Rust / Python
 * side of the binding.
 *
 * Conventions
 *   - plain pointers and sizes only; f32 everywhere (the crate is f32-only, README.md:17);
 *     row-major, contiguous; batches carry an explicit leading dimension `ld` (in elements).
 *   - the caller allocates outputs (sizes from the query functions); the library owns only the
 *     opaque config handle and its device-resident tables.
 *   - every function returns an ss_status; nothing unwinds across the boundary.  The reference
 *     panics where these return an error (usize underflow processing.rs:101,105; config.rs:162;
 *     functions.rs:136; asserts feature.rs:47-51).
 *   - `*_device` variants take device pointers and a hipStream_t (passed as void*) and are
 *     asynchronous; the others take host pointers and are synchronous (H2D + kernels + D2H).
 *   - a config handle is immutable after creation and may be used from several threads /
 *     streams concurrently.  The STFT carry-over state of config.rs:126,162 lives in
 *     caller-owned buffers instead: the ss_*_stream entry points take and update it.
 *   - there is NO CPU fallback: without a usable HIP device every compute entry point fails
 *     with SS_ERR_HIP.
 */
#ifndef SPEECHSAUCE_AMD_H
#define SPEECHSAUCE_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SS_ABI_VERSION 7 /* 7: the ragged streaming calls over a pool of stream states (ss_frame_stream_packed_row_offsets, ss_mfcc_stream_packed*, ss_mfe_stream_packed*; ss_stream_packed_row_offsets, ss_mel_spectrogram_stream_packed*, ss_stft_stream_packed*), the one-shot calls' 16-bit PCM forms (ss_mfcc_batch_i16*, ss_mfe_batch_i16*, ss_mfcc_packed_i16*, ss_mfe_packed_i16*; ss_mel_spectrogram_i16*, ss_stft_i16*, ss_mel_spectrogram_packed_i16*, ss_stft_packed_i16*, ss_mel_spectrogram_stream_packed_i16*, ss_stft_stream_packed_i16*), ss_mfcc_batches_device, ss_mel_spectrogram_batches_device, ss_mfcc_timed_region, the packed post-processing calls (ss_cmvn_packed*, ss_cmvnw_packed*, ss_power_to_db_packed*, ss_lmfe_packed*); 6: ss_shader_clock_probe; 5: config-free stack_frames entry points, ss_mfcc_shader_clock; the ss_debug_* test aids left the product library */

typedef enum ss_status {
    SS_OK = 0,
    SS_ERR_SHORT_SIGNAL = 1, /* fewer samples than one frame / zero frames (reference: usize underflow panic) */
    SS_ERR_BAD_CONFIG = 2,   /* parameter combination the reference asserts on or underflows with */
    SS_ERR_ARG = 3,          /* null pointer, bad leading dimension, ... */
    SS_ERR_HIP = 4,          /* HIP runtime error or no device (see ss_last_error_string) */
    SS_ERR_UNSUPPORTED = 5,  /* valid in the reference but not built here (fft_points > 8192, or > 2730 and not a power of two) */
    SS_ERR_DEVICE = 6        /* a kernel reported a device-side protocol error through the config's error word: the results of
                                that launch are incomplete (ss_config_device_status) */
} ss_status;

enum { SS_FRAMING_CONTRACT = 0, SS_FRAMING_LITERAL = 1, SS_FRAMING_CENTER = 2, SS_FRAMING_PADDED = 3 };
enum { SS_DCT_REFERENCE = 0, SS_DCT_ORTHO = 1 };
enum { SS_WINDOW_RECT = 0, SS_WINDOW_HANN = 1 /* periodic, functions.rs:349-357 */, SS_WINDOW_VORBIS = 2 };
/* librosa-compatible variants (the reference's stated goal, README.md:3,44) */
enum { SS_MEL_REFERENCE = 0, SS_MEL_SLANEY = 1, SS_MEL_HTK = 2 };
enum { SS_MEL_NORM_NONE = 0, SS_MEL_NORM_SLANEY = 1 };
enum { SS_PAD_REFLECT = 0, SS_PAD_CONSTANT = 1 };

/* DCT-II gain of the un-vendored ndrustfft `nddct2` (feature.rs:123): scipy's un-normalised
 * convention y[k] = 2 * sum x[n] cos(pi k (2n+1) / 2N).  One named constant; "parity unpinned". */
#define SS_DCT2_GAIN 2.0f

/*
 * ss_params: the nine arguments of SpeechConfig::new (config.rs:140-150) one-for-one, followed by
 * the switches of SURVEY.md section 0.  ss_params_default() fills SpeechConfigBuilder::new's
 * defaults (config.rs:35-47) and the reference-mode switches.
 */
typedef struct ss_params {
    uint32_t struct_size;       /* = sizeof(ss_params); checked by ss_config_create */
    uint32_t sample_rate;       /* config.rs:141 */
    uint32_t fft_points;        /* :142  (power of two 32..8192, or any length 16..2730: chirp-z transform) */
    float    frame_length;      /* :143  seconds */
    float    frame_stride;      /* :144  seconds */
    uint32_t num_cepstral;      /* :145 */
    uint32_t num_filters;       /* :146 */
    float    low_frequency;     /* :147 */
    float    high_frequency;    /* :148 */
    int32_t  dc_elimination;    /* :149 */
    /* ---- switches (reference mode = what ss_params_default sets) ---- */
    int32_t  framing;           /* SS_FRAMING_CONTRACT: frames[t,:] = x[t*step : t*step+flen], the documented
                                   contract (processing.rs:55-64).  SS_FRAMING_LITERAL: the exact_chunks copy as
                                   written (processing.rs:110-120), which leaves every frame zero for > 2 frames.
                                   SS_FRAMING_CENTER: librosa center=True -- frame t covers
                                   x[t*step - flen/2 : t*step + flen/2), 1 + n/step frames, edges per pad_mode.
                                   SS_FRAMING_PADDED: stack_frames(zero_padding = true), processing.rs:85-97 --
                                   ceil((L - flen) / step) frames, the last ones reading appended zeros (what the
                                   reference's test_stack_frames calls, lib.rs:50-68) */
    int32_t  spectrum_exponent; /* 1: |X|/N as written (processing.rs:168,180); 2: |X|^2/N (speechpy) */
    int32_t  dct_norm;          /* SS_DCT_REFERENCE: scaling as written (feature.rs:126-131); SS_DCT_ORTHO */
    float    dct2_gain;         /* SS_DCT2_GAIN */
    int32_t  mfcc_window;       /* window on the MFCC frames; reference applies none (feature.rs:203-210) */
    float    preemph_coef;      /* fused pre-emphasis y[n] = x[n] - c*x[(n-shift) mod L] (processing.rs:31-53);
                                   0 = off (reference mfcc() applies none) */
    int32_t  preemph_shift;     /* >= 1 */
    /* ---- librosa-compatible variants (all 0 in reference mode) ---- */
    int32_t  mel_scale;         /* SS_MEL_REFERENCE: feature.rs:36-90 as written (HTK formula, integer bin mapping
                                   floor((F+1) hz / sr)).  SS_MEL_SLANEY / SS_MEL_HTK: librosa.filters.mel -- triangles
                                   in Hz evaluated at the FFT bin frequencies, mel points on the Slaney (htk=False) or
                                   HTK scale */
    int32_t  mel_norm;          /* SS_MEL_NORM_SLANEY: each filter scaled by 2 / (f[m+2] - f[m]) (librosa norm="slaney");
                                   needs a non-reference mel_scale */
    int32_t  pad_mode;          /* SS_FRAMING_CENTER only: how samples outside the clip are read (np.pad reflect / zeros) */
} ss_params;

typedef struct ss_config ss_config; /* opaque; replaces speechsauce::config::SpeechConfig (config.rs:99-131) */

/* ---- configuration ------------------------------------------------------------------------ */

/* SpeechConfigBuilder::new(sample_rate) defaults, config.rs:35-47 (Default = 16 kHz, :133-137). */
int ss_params_default(ss_params *p, uint32_t sample_rate);

/* SpeechConfig::new, config.rs:140-185: derives sizes, builds the Vorbis window, the sparse mel
 * bank (feature.rs:36-90), FFT twiddles and the DCT table, and uploads them to the current HIP
 * device.  Fails with SS_ERR_HIP when no device is usable. */
int ss_config_create(const ss_params *p, ss_config **out);
void ss_config_destroy(ss_config *cfg);
int ss_config_params(const ss_config *cfg, ss_params *out);
/* Device-side status of the asynchronous (*_device) launches made on this config: SS_OK, or SS_ERR_DEVICE if a kernel has
 * reported a protocol error since the last call (the word is cleared).  Call it after synchronising the stream; the
 * host-pointer entry points check it themselves before they return, and every launch on a config with a pending error
 * fails with SS_ERR_DEVICE instead of queueing more work behind a broken one. */
int ss_config_device_status(const ss_config *cfg);

/* Validation and table construction only (no device): what ss_config_create checks. */
int ss_params_validate(const ss_params *p);

/* ---- derived sizes (host only, no device needed) --------------------------------------------- */

/* frame_sample_length / frame_step_size, processing.rs:77-78 */
int ss_frame_sizes(const ss_params *p, size_t *frame_len, size_t *frame_step);
/* numframes with zero_padding=false, processing.rs:101 (what mfe/mfcc use, feature.rs:203-210) */
int ss_num_frames(const ss_params *p, size_t n_samples, size_t *n_frames);
/* STFT geometry: hop = frame_size (config.rs:154), n_pad (functions.rs:96), wnorm (config.rs:178) */
int ss_stft_sizes(const ss_params *p, size_t *hop, size_t *n_pad, float *wnorm);
/* rows returned by stft1/stft2 = ceil(n/hop) (functions.rs:95-98,121); the last n_pad are zero */
int ss_stft_rows(const ss_params *p, size_t n_samples, size_t *rows, size_t *real_rows);

/* ---- tables (host only) ------------------------------------------------------------------- */

/* dense bank [num_filters x (fft_points/2+1)], feature.rs:36-90; idx (may be NULL) gets the
 * num_filters+2 bin indices of feature.rs:69-70 */
int ss_filterbank(const ss_params *p, float *fb, int32_t *idx);
/* SpeechConfig.window (Vorbis), config.rs:151-160; n = fft_points */
int ss_vorbis_window(size_t n, float *w);

/* ---- hot path, host pointers (synchronous) -------------------------------------------------- */

/* speechsauce::feature::mfcc(ArrayView1<f32>, &SpeechConfig) -> Array2<f32>  (feature.rs:99-148)
 * out: [n_frames x num_cepstral] */
int ss_mfcc(const ss_config *cfg, const float *x, size_t n_samples, float *out);
/* speechsauce::feature::mfe -> (Array2<f32>, Array1<f32>)  (feature.rs:200-233)
 * feat: [n_frames x num_filters], energy: [n_frames] */
int ss_mfe(const ss_config *cfg, const float *x, size_t n_samples, float *feat, float *energy);
/* mel_spectrogram1 (channels = 1) / mel_spectrogram2 (feature.rs:151-174); x: [channels x n_samples],
 * out: [channels x num_filters x rows] */
int ss_mel_spectrogram(const ss_config *cfg, const float *x, size_t channels, size_t n_samples, float *out);
/* speechsauce::processing::preemphasis (processing.rs:31-53) */
int ss_preemphasis(const float *x, size_t n_samples, long shift, float cof, float *y);
/* speechsauce::functions::stft1 (channels = 1, functions.rs:199-233) / stft2 (functions.rs:86-123) -> Array2 / Array3<Complex32>:
 * x [channels x n_samples]; out: interleaved re, im  [channels x rows x (fft_points/2+1) x 2], rows = ss_stft_rows
 * (the reference slices its n_pad leading rows off, functions.rs:121: the trailing n_pad rows are zero). */
int ss_stft(const ss_config *cfg, const float *x, size_t channels, size_t n_samples, float *out);
/* speechsauce::processing::stack_frames(signal, sample_rate, frame_length, frame_stride, filter, zero_padding)
 * (processing.rs:65-129) with the config's framing switch (contract / literal / padded = zero_padding) and frame window
 * (the `filter` argument; mfcc_window switch): frames [n_frames x frame_len], sizes from ss_num_frames / ss_frame_sizes. */
int ss_stack_frames(const ss_config *cfg, const float *x, size_t n_samples, float *frames);
/* The same function with the reference's own argument list and nothing else -- no SpeechConfig, no FFT length (the reference's
 * stack_frames has no FFT dependency: 44.1 kHz x 25 ms frames of round(1102.5) = 1103 samples are fine): contract framing
 * frames[t][i] = x[t * step + i], frame_len = round(sample_rate * frame_length), step likewise (processing.rs:77-78),
 * floor((n - frame_len) / step) frames, or ceil with the tail reading appended zeros when zero_padding != 0 (:85-106).
 * `window`: frame_len floats that multiply every frame -- row 0 of the Array2 the reference's `filter(frame_len)` returns
 * (processing.rs:122-126) -- or NULL.  ss_stack_frames_shape gives the output shape without touching the device. */
int ss_stack_frames_shape(size_t n_samples, uint32_t sample_rate, float frame_length, float frame_stride, int zero_padding,
                          size_t *num_frames, size_t *frame_len);
int ss_stack_frames_signal(const float *x, size_t n_samples, uint32_t sample_rate, float frame_length, float frame_stride,
                           const float *window, int zero_padding, float *frames);
/* speechsauce::processing::power_spectrum(frames: Array2<f32>, fft_points) -> Array2<f32>  (processing.rs:179-181; fft_spectrum
 * :143-171 zero-pads rows shorter than fft_points): frames [rows x cols], cols <= the config's fft_points;
 * P [rows x (fft_points/2+1)] = |rfft(row)| / fft_points.  Only fft_points of the config is used. */
int ss_power_spectrum_frames(const ss_config *cfg, const float *frames, size_t rows, size_t cols, float *P);
/* the same stage on the frames mfe cuts from a signal (stack_frames + power_spectrum, feature.rs:203-214):
 * P [n_frames x (fft_points/2+1)] */
int ss_power_spectrum(const ss_config *cfg, const float *x, size_t n_samples, float *P);

/* batch of equal-length clips: x [batch x n_samples] with row stride ld >= n_samples.
 * out: [batch x n_frames x num_cepstral] */
int ss_mfcc_batch(const ss_config *cfg, const float *x, size_t batch, size_t n_samples, size_t ld, float *out);
int ss_mfe_batch(const ss_config *cfg, const float *x, size_t batch, size_t n_samples, size_t ld,
                 float *feat, float *energy);
/* P [batch x n_frames x (fft_points/2+1)] */
int ss_power_spectrum_batch(const ss_config *cfg, const float *x, size_t batch, size_t n_samples, size_t ld, float *P);

/* ---- hot path, device pointers (asynchronous on `stream`) ----------------------------------- */

int ss_mfcc_batch_device(const ss_config *cfg, const float *d_x, size_t batch, size_t n_samples, size_t ld,
                         float *d_out, void *stream);
/* Several independent batches per call (a loop over speechsauce::feature::mfcc, feature.rs:99-148, per clip of every batch):
 * d_x / batch / d_out are HOST arrays of n_batches entries -- device pointer of batch b's clips [batch[b] x n_samples] (row
 * stride ld), its clip count, device pointer of its output block [batch[b] x n_frames x num_cepstral].  The arrays are read
 * before the call returns (nothing keeps pointing at them); batches with batch[b] == 0 are skipped.  Where the configuration's
 * kernel takes a batch table (fft_points = 512 with the default frame shape and bank: the headline kernel) up to 8 batches share
 * ONE launch, whose persistent workgroups run over all the batches' frames -- a launch's start-up and its one-unit tail are paid
 * once per call, not once per batch; other configurations are served batch by batch on `stream`.  Results are bit-identical to
 * n_batches separate ss_mfcc_batch_device calls either way. */
int ss_mfcc_batches_device(const ss_config *cfg, size_t n_batches, const float *const *d_x, const size_t *batch, size_t n_samples,
                           size_t ld, float *const *d_out, void *stream);
/* the mel_spectrogram2 form (feature.rs:163-174 per block): block b is [channels[b] x n_samples], its output
 * [channels[b] x num_filters x rows]; served block by block on `stream` */
int ss_mel_spectrogram_batches_device(const ss_config *cfg, size_t n_batches, const float *const *d_x, const size_t *channels,
                                      size_t n_samples, size_t ld, float *const *d_out, void *stream);
int ss_mfe_batch_device(const ss_config *cfg, const float *d_x, size_t batch, size_t n_samples, size_t ld,
                        float *d_feat, float *d_energy, void *stream);
int ss_mel_spectrogram_device(const ss_config *cfg, const float *d_x, size_t channels, size_t n_samples,
                              size_t ld, float *d_out, void *stream);
int ss_preemphasis_device(const float *d_x, size_t n_samples, long shift, float cof, float *d_y, void *stream);
/* power_spectrum over the frames of each clip: [batch x n_frames x (fft_points/2+1)] (processing.rs:179-181) */
int ss_power_spectrum_batch_device(const ss_config *cfg, const float *d_x, size_t batch, size_t n_samples,
                                   size_t ld, float *d_P, void *stream);
/* power_spectrum of a frames matrix [rows x cols] with row stride ld: [rows x (fft_points/2+1)] */
int ss_power_spectrum_frames_device(const ss_config *cfg, const float *d_frames, size_t rows, size_t cols, size_t ld,
                                    float *d_P, void *stream);
/* stft2 (functions.rs:86-123): interleaved re,im  [channels x rows x (fft_points/2+1) x 2] */
int ss_stft_device(const ss_config *cfg, const float *d_x, size_t channels, size_t n_samples, size_t ld,
                   float *d_out, void *stream);
/* ---- ss_mel_spectrogram* / ss_stft* fed signed 16-bit PCM ----
 * The STFT path's share of the PCM forms (the MFCC / mfe ones are below): ss_mel_spectrogram_device / ss_stft_device /
 * ss_mel_spectrogram / ss_stft with the samples as int16 and a scale behind the sample-layout arguments: sample s = (float)pcm * scale,
 * converted on load.  Everything else is the float forms' contract, word for word -- shapes, errors, channels == 0, the trailing
 * n_pad zero rows.  ld is in samples, not bytes.
 *   scale: a power of two in [2^-64, 2^64], otherwise SS_ERR_ARG before anything runs -- 2^-15 for normalised audio, 1.0 for
 *   integer-valued floats.  With a power of two the product is exact, so fusing it into what follows changes no bit.
 *   Equivalence: the output is bit for bit what the float form returns on x_f[k] = (float)pcm[k] * scale, for every configuration
 *   the float form accepts.
 *   Kernels: the PCM build of the kernel the float call picks, where it has one -- ss_mel_c1024i<w12,...> (mel output of the
 *   2048-point shape where the float call's own rule picks the twelve-wave build) and ss_front_generic_i16<...> (every configuration
 *   the generic kernel serves, mel and stft output).  The eight-wave 2048-point family (small calls, stft output, banks past bin 512)
 *   and the 512 / 1024 / 4096-point mel kernels run behind one conversion launch into a stream-ordered temporary;
 *   ss_last_kernel_name() then reports the float kernel.  That path allocates and frees in stream order and is not offered for stream
 *   capture.
 *   Alignment: the device buffer needs 2-byte alignment only -- an odd ld and an odd base offset are fine.
 *   Host forms: the samples cross the link as int16 (half the bytes of the float forms); no alignment rule. */
int ss_mel_spectrogram_i16_device(const ss_config *cfg, const int16_t *d_x, size_t channels, size_t n_samples, size_t ld, float scale,
                                  float *d_out, void *stream);
int ss_stft_i16_device(const ss_config *cfg, const int16_t *d_x, size_t channels, size_t n_samples, size_t ld, float scale, float *d_out,
                       void *stream);
int ss_mel_spectrogram_i16(const ss_config *cfg, const int16_t *x, size_t channels, size_t n_samples, float scale, float *out);
int ss_stft_i16(const ss_config *cfg, const int16_t *x, size_t channels, size_t n_samples, float scale, float *out);
/* stack_frames over a batch of clips: frames [batch x n_frames x frame_len] */
int ss_stack_frames_device(const ss_config *cfg, const float *d_x, size_t batch, size_t n_samples, size_t ld,
                           float *d_frames, void *stream);

/* ---- packed variable-length clips (a loop over speechsauce::feature::mfcc / mfe, feature.rs:99-148 / :200-233, per clip) ----
 * Clips of different lengths packed end to end in one float buffer: clip b is x[so[b] : so[b+1]], so = sample_offsets, n_clips + 1
 * non-decreasing entries with so[0] = 0 (the cu_seqlens convention).  Features are packed in clip order: clip b owns rows
 * fo[b] .. fo[b+1] of [total_frames x num_cepstral] (mfcc) or [total_frames x num_filters] + [total_frames] (mfe), fo =
 * frame_offsets.  Per clip, every result is what ss_mfcc / ss_mfe returns for that clip alone: its own frame count T_b and DCT
 * scaling (n = T_b * M, feature.rs:126-131), its [0,0] element, pre-emphasis modulo its own length, literal framing's T_b > 2 rule,
 * centred / padded framing at its own edges.  n_clips == 0 is SS_OK with nothing launched.
 * Every call is ONE launch.  MFCC of the headline shape (fft_points 512 with the default frame shape and bank, contract framing,
 * reference DCT, no window / pre-emphasis) runs on the varlen build of that shape's dedicated kernel: per clip the same bits as
 * ss_mfcc_batch_device.  Every other configuration, and mfe, runs on the varlen build of the generic kernel (any fft_points, chirp-z
 * included; windows, pre-emphasis, every framing, ortho DCT, spectrum_exponent 2, librosa banks): per clip the same bits as the
 * generic kernel's equal-length path.  The dedicated 256 / 1024 / 2048 / 4096-point kernels have no varlen builds. */
/* host only, no device needed: fo[0..n_clips] for clips x[so[b] : so[b+1]]; SS_ERR_SHORT_SIGNAL names the first clip with zero
 * frames (ss_last_error_string), SS_ERR_ARG for decreasing offsets / so[0] != 0 / a clip of more than 2^31 - 1 samples */
int ss_packed_frame_offsets(const ss_params *p, size_t n_clips, const int64_t *sample_offsets, int64_t *frame_offsets);
/* host pointers (H2D, one device call, D2H); sample_offsets is a host array.  out: [fo[n_clips] x num_cepstral] */
int ss_mfcc_packed(const ss_config *cfg, const float *x, size_t n_clips, const int64_t *sample_offsets, float *out);
int ss_mfe_packed(const ss_config *cfg, const float *x, size_t n_clips, const int64_t *sample_offsets, float *feat, float *energy);

/* ---- the one-shot MFCC / mfe calls fed signed 16-bit PCM ----
 * Speech corpora and decoded WAV files are int16.  These eight entry points are ss_mfcc_batch* / ss_mfe_batch* / ss_mfcc_packed* /
 * ss_mfe_packed* with the samples as int16 and a scale behind the sample-layout arguments: sample s = (float)pcm * scale, converted
 * on load.  Everything else is the float forms' contract, word for word -- shapes, errors, empty batches, the packed tables'
 * containment and the SS_ERR_DEVICE reporting of the packed device forms.  ld and the offsets are in samples, not bytes.
 *   scale: a power of two in [2^-64, 2^64], otherwise SS_ERR_ARG before anything runs -- 2^-15 for normalised audio, 1.0 for
 *   integer-valued floats.  With a power of two the product is exact, so fusing it into what follows changes no bit.
 *   Equivalence: every output (features, energies) is bit for bit what the float form returns on x_f[k] = (float)pcm[k] * scale,
 *   for every configuration the float form accepts.
 *   Kernels: the PCM build of the kernel the float call picks, where it has one -- ss_mfcc_c256i<...> (the 512-point kernel's
 *   contract-framing builds without fused pre-emphasis), ss_mfcc_c256vi<...> (its packed build), ss_front_generic_i16<...> /
 *   ss_front_generic_varleni<...> (every configuration the generic kernel serves).  The equal-length calls on every other dedicated
 *   kernel (256 / 1024 / 2048 / 4096 points, the 512-point builds with centred frames, fused pre-emphasis, whole-spectrum banks or
 *   more than 48 filters) run that kernel behind one conversion launch into a stream-ordered temporary; ss_last_kernel_name() then
 *   reports the float kernel.  That path allocates and frees in stream order and is not offered for stream capture; the PCM builds
 *   are single launches and capture like the float calls.
 *   Alignment: the buffer needs 2-byte alignment only -- an odd ld, an odd base offset and clip offsets of either parity are fine.
 *   Host forms: the samples cross the link as int16 (half the bytes of the float forms); the 16 MB chunks and the 1 MB small-call
 *   threshold of the batch forms are in bytes. */
int ss_mfcc_batch_i16_device(const ss_config *cfg, const int16_t *d_x, size_t batch, size_t n_samples, size_t ld, float scale,
                             float *d_out, void *stream);
int ss_mfe_batch_i16_device(const ss_config *cfg, const int16_t *d_x, size_t batch, size_t n_samples, size_t ld, float scale,
                            float *d_feat, float *d_energy, void *stream);
int ss_mfcc_packed_i16_device(const ss_config *cfg, const int16_t *d_x, size_t n_clips, const int64_t *d_sample_offsets, float scale,
                              const int64_t *d_frame_offsets, size_t total_frames, float *d_out, void *stream);
int ss_mfe_packed_i16_device(const ss_config *cfg, const int16_t *d_x, size_t n_clips, const int64_t *d_sample_offsets, float scale,
                             const int64_t *d_frame_offsets, size_t total_frames, float *d_feat, float *d_energy, void *stream);
int ss_mfcc_batch_i16(const ss_config *cfg, const int16_t *x, size_t batch, size_t n_samples, size_t ld, float scale, float *out);
int ss_mfe_batch_i16(const ss_config *cfg, const int16_t *x, size_t batch, size_t n_samples, size_t ld, float scale, float *feat,
                     float *energy);
int ss_mfcc_packed_i16(const ss_config *cfg, const int16_t *x, size_t n_clips, const int64_t *sample_offsets, float scale, float *out);
int ss_mfe_packed_i16(const ss_config *cfg, const int16_t *x, size_t n_clips, const int64_t *sample_offsets, float scale, float *feat,
                      float *energy);
/* device pointers, asynchronous on `stream`, graph-capturable: d_sample_offsets / d_frame_offsets are DEVICE arrays of n_clips + 1
 * entries (fo from ss_packed_frame_offsets, or computed by the caller on the device); total_frames = the rows d_out holds.  The
 * kernel checks the tables against each other: a clip whose rows are not the T_b frames its samples give, or that end past
 * total_frames, is skipped (nothing is written outside d_out / d_energy) and the config's device error word is raised -- the next
 * call on the config (or ss_config_device_status) returns SS_ERR_DEVICE. */
int ss_mfcc_packed_device(const ss_config *cfg, const float *d_x, size_t n_clips, const int64_t *d_sample_offsets,
                          const int64_t *d_frame_offsets, size_t total_frames, float *d_out, void *stream);
int ss_mfe_packed_device(const ss_config *cfg, const float *d_x, size_t n_clips, const int64_t *d_sample_offsets,
                         const int64_t *d_frame_offsets, size_t total_frames, float *d_feat, float *d_energy, void *stream);

/* ---- packed variable-length clips, STFT path (a loop over speechsauce::feature::mel_spectrogram / functions::stft2 per clip) ----
 * Sample offsets as above (so[0] = 0, non-decreasing, n_clips + 1 entries).  Clip b has R_b = ceil(n_b / hop) rows (f32, as
 * ss_stft_rows computes them); ro = row_offsets, ro[b+1] - ro[b] = R_b.  mel: clip b's block [num_filters x R_b] (the (n_mels, time)
 * layout of ss_mel_spectrogram) is contiguous and starts at out + num_filters * ro[b].  stft: [ro[n_clips] x (fft_points/2+1) x 2]
 * interleaved re / im, clip b owns rows ro[b] .. ro[b+1].  Per clip, every result is what ss_mel_spectrogram / ss_stft returns for
 * that clip alone: zero initial state, the zero padding of a partial last hop, its last n_pad rows exact zeros (functions.rs:121),
 * every switch and bank of the config.  n_clips == 0 is SS_OK with nothing launched; a config without an STFT path
 * (fft_points < 2 * hop, functions.rs:136) is SS_ERR_BAD_CONFIG.
 * Every call is ONE launch.  mel output of the 2048-point shape with a bank within bins 0..512 (cfg3: hop 512, 128 mels) runs on the
 * packed build of the twelve-wave kernel: per clip the same bits as ss_mel_spectrogram_device on that clip where the twelve-wave
 * build serves it.  Every other configuration (any fft_points, chirp-z included; every bank; a 2048-point bank past bin 512) and all
 * stft output run on the packed build of the generic kernel: per clip the same bits as the generic kernel's equal-length path.  The
 * dedicated 512 / 1024 / 4096-point mel kernels and the 2048-point stft build have no packed builds. */
/* host only, no device needed: ro[0..n_clips] for clips x[so[b] : so[b+1]]; SS_ERR_ARG for decreasing offsets / so[0] != 0 / an
 * empty clip (named in ss_last_error_string) / a clip of more than 2^31 - 1 samples */
int ss_packed_row_offsets(const ss_params *p, size_t n_clips, const int64_t *sample_offsets, int64_t *row_offsets);
/* host pointers (H2D, one device call, D2H); sample_offsets is a host array.  out: num_filters * ro[n_clips] floats (mel) /
 * ro[n_clips] * (fft_points/2+1) * 2 floats (stft) */
int ss_mel_spectrogram_packed(const ss_config *cfg, const float *x, size_t n_clips, const int64_t *sample_offsets, float *out);
int ss_stft_packed(const ss_config *cfg, const float *x, size_t n_clips, const int64_t *sample_offsets, float *out);
/* device pointers, asynchronous on `stream`, graph-capturable: d_sample_offsets / d_row_offsets are DEVICE arrays of n_clips + 1
 * entries (ro from ss_packed_row_offsets, or computed by the caller on the device); total_rows = the rows d_out holds.  The kernel
 * recomputes every R_b from the sample offsets with the host's bits: a clip whose rows disagree with ro, or that end past
 * total_rows, is skipped (nothing is written outside d_out) and the config's device error word is raised -- the next call on the
 * config (or ss_config_device_status) returns SS_ERR_DEVICE. */
int ss_mel_spectrogram_packed_device(const ss_config *cfg, const float *d_x, size_t n_clips, const int64_t *d_sample_offsets,
                                     const int64_t *d_row_offsets, size_t total_rows, float *d_out, void *stream);
int ss_stft_packed_device(const ss_config *cfg, const float *d_x, size_t n_clips, const int64_t *d_sample_offsets,
                          const int64_t *d_row_offsets, size_t total_rows, float *d_out, void *stream);
/* The same four fed signed 16-bit PCM: sample s = (float)pcm * scale, scale a power of two in [2^-64, 2^64] (else SS_ERR_ARG before
 * anything runs), the offsets in samples.  Every output is bit for bit what the float form returns on x_f[k] = (float)pcm[k] * scale;
 * everything else -- errors, n_clips == 0, the tables' containment and the SS_ERR_DEVICE reporting, capturability of the device
 * forms -- is the float forms' contract.  Each float call picks one of two kernels and both have PCM builds, so every call is ONE
 * launch and nothing converts first: ss_mel_c1024vi<...> (the packed twelve-wave build) / ss_front_generic_varrowsi<...> (everything
 * else, all stft output).  The device buffer needs 2-byte alignment only (clip offsets of either parity); the host forms stage the
 * buffer as int16 and have no alignment rule. */
int ss_mel_spectrogram_packed_i16_device(const ss_config *cfg, const int16_t *d_x, size_t n_clips, const int64_t *d_sample_offsets, float scale,
                                         const int64_t *d_row_offsets, size_t total_rows, float *d_out, void *stream);
int ss_stft_packed_i16_device(const ss_config *cfg, const int16_t *d_x, size_t n_clips, const int64_t *d_sample_offsets, float scale,
                              const int64_t *d_row_offsets, size_t total_rows, float *d_out, void *stream);
int ss_mel_spectrogram_packed_i16(const ss_config *cfg, const int16_t *x, size_t n_clips, const int64_t *sample_offsets, float scale, float *out);
int ss_stft_packed_i16(const ss_config *cfg, const int16_t *x, size_t n_clips, const int64_t *sample_offsets, float scale, float *out);

/* ---- log-mel spectrogram: ss_mel_spectrogram* with librosa's power_to_db per clip, converted in the mel kernels' epilogue ----
 * Eight entry points, each its mel counterpart with `float ref, float amin, float top_db` in front of the output pointer.  Shapes,
 * layouts ([channels x num_filters x rows]; packed: clip b's [num_filters x R_b] block at out + num_filters * ro[b]), errors and edge
 * cases are the mel calls' own: channels == 0 / n_clips == 0 is SS_OK with nothing launched, the packed tables' containment and the
 * SS_ERR_DEVICE reporting are unchanged, pcm scale as in the _i16 mel forms.  amin must be > 0 and ref must not be NaN, else
 * SS_ERR_ARG before anything runs (|ref| is used, as in ss_power_to_db).
 *   Contract: per clip (channel), every output is bit for bit what the two-step path returns -- the mel call on the same input, then
 *   ss_power_to_db_packed_device over its result with every clip as its own segment (cols = num_filters, offsets = the row offsets)
 *   and the same ref / amin / top_db.  Element: fmaf(10, log10f(fmaxf(amin, S)), -ref_db), ref_db = 10 log10(max(amin, |ref|)) formed
 *   on the host.
 *   top_db: the floor is PER CLIP -- max(that clip's dB values) - top_db; top_db < 0 switches it off.  The trailing n_pad zero rows
 *   (functions.rs:121) come out as 10 log10(amin) - ref_db and take part in the maximum, as in the two-step path.  This is NOT what
 *   ss_power_to_db_device does on a multi-channel block: that call takes ONE maximum over the whole block.
 *   Launches: the twelve-wave 2048-point mel kernel (dense where the mel call's own rule picks it, packed always) and the generic
 *   kernel (every fft_points, chirp-z included; dense and packed) have dB builds, float and PCM: the conversion costs no launch and no
 *   pass over the block.  top_db < 0: ONE launch, nothing allocated.  Otherwise the launch, then one floor pass; the per-clip maxima
 *   are a stream-ordered block of n_clips ints, set up by one small launch in front (a kernel, so that a captured call holds no
 *   memset node).  The floor pass leaves alone every clip the packed table check skipped.  Where the mel
 *   call runs a kernel without a dB build -- the eight-wave 2048-point builds, the dedicated 512 / 1024 / 4096-point mel kernels --
 *   that kernel runs as in the mel call and one in-place pass converts the block: same bits, one launch more.
 *   ss_last_kernel_name(): a dB build carries `db` in its template list (ss_mel_c1024v<w12,mel6321,db>, ss_front_generic_varrows<9,db>);
 *   the composed path reports the mel kernel's name followed by "+db" (ss_mel_c256+db).
 *   Kernel selection of every other call is untouched.  The device forms are linear chains on `stream` and capture like the mel
 *   calls (the PCM conversion fallback of the dense _i16 form excepted, as there).  No streaming / pool forms: a stream has no clip
 *   maximum. */
int ss_log_mel_spectrogram(const ss_config *cfg, const float *x, size_t channels, size_t n_samples, float ref, float amin, float top_db,
                           float *out);
int ss_log_mel_spectrogram_device(const ss_config *cfg, const float *d_x, size_t channels, size_t n_samples, size_t ld, float ref, float amin,
                                  float top_db, float *d_out, void *stream);
int ss_log_mel_spectrogram_i16(const ss_config *cfg, const int16_t *x, size_t channels, size_t n_samples, float scale, float ref, float amin,
                               float top_db, float *out);
int ss_log_mel_spectrogram_i16_device(const ss_config *cfg, const int16_t *d_x, size_t channels, size_t n_samples, size_t ld, float scale,
                                      float ref, float amin, float top_db, float *d_out, void *stream);
int ss_log_mel_spectrogram_packed(const ss_config *cfg, const float *x, size_t n_clips, const int64_t *sample_offsets, float ref, float amin,
                                  float top_db, float *out);
int ss_log_mel_spectrogram_packed_device(const ss_config *cfg, const float *d_x, size_t n_clips, const int64_t *d_sample_offsets,
                                         const int64_t *d_row_offsets, size_t total_rows, float ref, float amin, float top_db, float *d_out,
                                         void *stream);
int ss_log_mel_spectrogram_packed_i16(const ss_config *cfg, const int16_t *x, size_t n_clips, const int64_t *sample_offsets, float scale, float ref,
                                      float amin, float top_db, float *out);
int ss_log_mel_spectrogram_packed_i16_device(const ss_config *cfg, const int16_t *d_x, size_t n_clips, const int64_t *d_sample_offsets, float scale,
                                             const int64_t *d_row_offsets, size_t total_rows, float ref, float amin, float top_db, float *d_out,
                                             void *stream);

/* ---- streaming STFT / mel spectrogram with carried state (functions.rs:86-170, config.rs:126,162) ----
 * The reference keeps the last S = fft_points - frame_size samples in SpeechConfig::analysis_mem (config.rs:162) and opens every
 * stft1 / stft2 / mel_spectrogram call with them (frame_analysis, functions.rs:137-160), so audio fed chunk by chunk gives frames
 * whose window reaches back into earlier chunks.  Here the config stays immutable and the state lives in a caller-owned buffer:
 * [n_streams x S] floats, contiguous, updated in place by every call.  All zeros is a fresh stream (what a new SpeechConfig
 * gives); zeroing a row resets that stream.  Streams are independent: stream s behaves like its own SpeechConfig fed through
 * stft1 / mel_spectrogram1 (stft2's hand-over of channel c - 1's tail to channel c, SURVEY Q6, is not reproduced).
 * H = frame_size (config.rs:154), W = fft_points, n_pad = W / H - 1 (functions.rs:96); the STFT path needs W >= 2H.
 *   SS_STREAM_CONTINUOUS: n_samples a multiple of H (else SS_ERR_ARG, state untouched).  R = n_samples / H rows, all real: row g
 *     of a stream, counted in hops since its reset, is wnorm * rfft(window * s[(g+1)H - W : (g+1)H]) with zeros before the
 *     stream's start (functions.rs:137-169).  Consecutive calls concatenate to the same rows however the stream was cut; they
 *     equal the real rows of the one-shot ss_stft / ss_mel_spectrogram on zeros(n_pad * H) ++ s.
 *   SS_STREAM_REFERENCE: exactly what stft1 / mel_spectrogram1 return on a SpeechConfig that has seen the earlier chunks:
 *     ceil(n / H) rows (functions.rs:97), row i the frame ending at this call's chunk i + n_pad, the trailing n_pad rows exact
 *     zeros (:121); a partial last chunk is zero-padded to H and those zeros enter the state (:112-117, :158-160).  Any
 *     n_samples >= 1; real_rows may be 0 (the state still advances).
 * Outputs as the stateless calls: mel [n_streams x num_filters x R], stft [n_streams x R x (W/2+1) x 2].  Every switch and bank of
 * the config applies.  Arguments as ss_stft_device: n_streams == 0 is SS_OK with nothing launched; null buffers, ld < n_samples,
 * n_samples == 0, more than 2^31 - 1 samples or streams, and a state range that overlaps x or out are SS_ERR_ARG; a config with
 * no STFT path is SS_ERR_BAD_CONFIG.  A rejected call leaves the state as it was. */
enum { SS_STREAM_REFERENCE = 0, SS_STREAM_CONTINUOUS = 1 };
/* host only, no device needed: S = fft_points - frame_size (config.rs:162) */
int ss_stream_state_len(const ss_params *p, size_t *state_len);
/* host only: the rows a call of n_samples returns and how many of them are real (the rest are the zeros of functions.rs:121) */
int ss_stream_rows(const ss_params *p, int mode, size_t n_samples, size_t *rows, size_t *real_rows);
/* host pointers, synchronous: one upload of x and state, the device call, one download of out and state */
int ss_stft_stream(const ss_config *cfg, int mode, const float *x, size_t n_streams, size_t n_samples, size_t ld, float *state,
                   float *out);
int ss_mel_spectrogram_stream(const ss_config *cfg, int mode, const float *x, size_t n_streams, size_t n_samples, size_t ld,
                              float *state, float *out);
/* device pointers, asynchronous on `stream`, graph-capturable (two stream-ordered launches, a linear chain: the rows, then the
 * state advance) */
int ss_stft_stream_device(const ss_config *cfg, int mode, const float *d_x, size_t n_streams, size_t n_samples, size_t ld,
                          float *d_state, float *d_out, void *stream);
int ss_mel_spectrogram_stream_device(const ss_config *cfg, int mode, const float *d_x, size_t n_streams, size_t n_samples, size_t ld,
                                     float *d_state, float *d_out, void *stream);

/* ---- streaming MFCC / mfe with carried frame state (feature.rs:99-233 over live audio) ----
 * The reference's mfcc / mfe keep no state; these entry points give a live stream one new row per hop, with no recomputation of
 * overlapping frames.  flen / step as ss_frame_sizes; sh = preemph_shift if preemph_coef != 0, else 0.  Every stream carries the
 * last S = max(flen + sh - step, 0) samples it was fed in a caller-owned buffer: [n_streams x S] floats, contiguous, updated in place
 * by every call.  All zeros is a fresh stream; zeroing a row resets that stream.  S == 0 is legal (the state pointer may then be
 * NULL and no state advance is launched).
 *   Chunks: n_samples a multiple of step (else SS_ERR_ARG, state untouched); R = n_samples / step rows per stream.  Row g of a
 *   stream, counted in hops since its reset, is the frame s[(g+1) step - flen : (g+1) step] of the stream's samples s with zeros
 *   before its start, through every per-frame stage of the config: pre-emphasis y[n] = s[n] - c s[n - sh] (same zeros; no circular
 *   wrap: a stream has no end), mfcc_window, fft_points (chirp-z included), spectrum_exponent, the bank, dct2_gain, dc_elimination,
 *   zero handling.  Consecutive calls concatenate to the same rows however the stream was cut.
 *   Framing: SS_FRAMING_CONTRACT and SS_FRAMING_PADDED stream alike (they differ only at a clip's end); SS_FRAMING_LITERAL and
 *   SS_FRAMING_CENTER are SS_ERR_BAD_CONFIG, from ss_frame_stream_state_len as well.
 *   DCT scaling: SS_DCT_REFERENCE scales by n = T * M (feature.rs:126-131), and T is the caller's norm_frames (>= 1; 0 is SS_ERR_ARG;
 *   typically the frame count of the model's input window).  Every streamed row is scaled as rows t >= 1 of the one-shot call are:
 *   column 0 unscaled (times dct2_gain), columns 1.. times dct2_gain / sqrtf(2n), with the host's bits.  The one-shot [0,0] factor
 *   belongs to a clip's first frame, and a stream has no first frame: it is never applied.  With dc_elimination on (the default)
 *   column 0 is ln(energy) either way.  SS_DCT_ORTHO ignores norm_frames.
 *   One-shot equivalence: let G be the rows fed since reset and sh <= step.  The concatenated MFCC rows equal rows 1 .. G of
 *   ss_mfcc on zeros(flen) ++ s ++ zeros(step) (exactly G + 1 frames) on a config with norm_frames = G + 1 frames, and likewise the
 *   mfe features and energies (the trailing zeros make the one-shot's circular pre-emphasis wrap read zeros).  Where both calls run
 *   the same kernel family, bit for bit: the default 512-point MFCC / mfe shape runs on streaming builds of the dedicated kernel
 *   (ss_mfcc_c256s), everything else on the streaming build of the generic kernel (the other dedicated kernels -- 256 / 1024 /
 *   2048 / 4096 points -- have no streaming build).
 * Outputs: MFCC [n_streams x R x num_cepstral]; mfe feat [n_streams x R x num_filters], energy [n_streams x R].  Arguments as
 * ss_stft_stream_device: n_streams == 0 is SS_OK with nothing launched; null buffers, ld < n_samples, n_samples == 0, more than
 * 2^31 - 1 samples or streams, and a state range that overlaps x or an output are SS_ERR_ARG.  A rejected call leaves the state as
 * it was. */
/* host only, no device: S = max(flen + sh - step, 0); SS_ERR_BAD_CONFIG for literal / centred framing */
int ss_frame_stream_state_len(const ss_params *p, size_t *state_len);
/* host only: rows = n_samples / step; SS_ERR_ARG if n_samples is 0 or not a multiple of step */
int ss_frame_stream_rows(const ss_params *p, size_t n_samples, size_t *rows);
/* host pointers, synchronous: one upload of x and state, the device call, one download of the outputs and state */
int ss_mfcc_stream(const ss_config *cfg, const float *x, size_t n_streams, size_t n_samples, size_t ld, uint32_t norm_frames,
                   float *state, float *out);
int ss_mfe_stream(const ss_config *cfg, const float *x, size_t n_streams, size_t n_samples, size_t ld, float *state, float *feat,
                  float *energy);
/* device pointers, asynchronous on `stream`, graph-capturable: two stream-ordered launches (the rows, then the state advance) */
int ss_mfcc_stream_device(const ss_config *cfg, const float *d_x, size_t n_streams, size_t n_samples, size_t ld, uint32_t norm_frames,
                          float *d_state, float *d_out, void *stream);
int ss_mfe_stream_device(const ss_config *cfg, const float *d_x, size_t n_streams, size_t n_samples, size_t ld, float *d_state,
                         float *d_feat, float *d_energy, void *stream);

/* ---- ragged streaming MFCC / mfe over a pool of stream states ----
 * The streaming calls above take a dense chunk block: every stream of the state block takes part, each with the same number of
 * hops.  A server holds a pool of open streams of which, in any tick, only some have new audio, and those a hop count of their
 * own.  These entry points serve such a tick in one call.
 *   Pool: a caller-owned block [pool_streams x S] of floats, S = ss_frame_stream_state_len -- the state block of the calls above,
 *   row for row (all zeros = fresh stream, zeroing a row resets it; S == 0 allows a NULL pool).
 *   Entries: a call serves n_active entries.  Entry i's chunk is x[so[i] : so[i+1]] of one packed buffer (so: n_active + 1
 *   non-decreasing int64 sample offsets, so[0] = 0, as ss_mfcc_packed); its length n_i is a whole number of hops R_i = n_i / step,
 *   and R_i = 0 is legal: no rows, the state row untouched (a captured graph of fixed n_active serves a changing set of streams
 *   that way).  Its state is pool row slots[i] (int32, 0 <= slots[i] < pool_streams, distinct within a call).  Its rows are rows
 *   ro[i] .. ro[i+1] of the packed outputs (ro: n_active + 1 row offsets, ro[0] = 0, ro[i+1] - ro[i] = R_i; from
 *   ss_frame_stream_packed_row_offsets or computed by the caller on the device): MFCC [total_rows x num_cepstral]; mfe feat
 *   [total_rows x num_filters], energy [total_rows].  total_rows is the rows the outputs hold (>= ro[n_active]; rows past it are
 *   left alone).
 *   Equivalence: per entry the rows, and the pool row afterwards, are what ss_mfcc_stream_device / ss_mfe_stream_device give for
 *   that stream alone (n_streams = 1, that chunk, that state row, the same norm_frames), bit for bit, wherever the entry stands in
 *   the call.  Everything the dense streaming contract says carries over: the per-frame stages, pre-emphasis reading zeros / the
 *   state and never wrapping, norm_frames, no [0,0] factor, contract and padded framing alike, literal / centred framing
 *   SS_ERR_BAD_CONFIG.  Pool rows not named in `slots` are neither read nor written.
 *   Kernels: the default 512-point MFCC / mfe shape runs on the ragged streaming builds of the dedicated kernel, reported by
 *   ss_last_kernel_name() as ss_mfcc_c256sp<10,exact,bank421,sym> / ss_mfcc_c256sp<10,exact,bank421,mfe>; every other
 *   configuration the dense generic streaming build serves runs on ss_front_generic_fstreamp<LOG2C[,chirpz]>.  A second
 *   stream-ordered launch (ss_stream_advance_packed) moves the named pool rows on; it is skipped where S == 0.  The device forms
 *   are a linear chain of these two launches whose grids depend on n_active and total_rows only: capturable, and replayable with
 *   other table contents.
 *   Containment: the device forms never see the tables on the host.  Both kernels decode every entry with one shared function; an
 *   entry is skipped -- no row written, its pool row untouched -- unless so[i] >= 0, 0 <= n_i <= 2^31 - 1, n_i % step == 0,
 *   ro[i] >= 0, ro[i+1] - ro[i] == n_i / step, ro[i+1] <= total_rows and 0 <= slots[i] < pool_streams.  Whatever the tables hold,
 *   nothing is read or written outside x's entry ranges, rows [0, total_rows) of the outputs and rows [0, pool_streams) of the
 *   pool.  A skipped entry raises the config's device error word: the call itself returns SS_OK, the next call on the config (or
 *   ss_config_device_status) returns SS_ERR_DEVICE once.
 *   Duplicate slots in a device-form call are a caller error that is NOT detected: the rows and the pool rows of the entries
 *   that share a slot are unspecified; everything stays inside the pool.  The host-pointer forms reject them.
 * Arguments: n_active == 0 is SS_OK with nothing launched.  SS_ERR_ARG, pool and outputs untouched: null buffers (the pool may be
 * NULL iff S == 0), n_active, pool_streams or total_rows >= 2^31, norm_frames == 0 with SS_DCT_REFERENCE, a pool range that
 * overlaps an output.  The host-pointer forms also check the tables before they touch the device -- so[0] != 0, a decreasing
 * pair, a chunk that is not whole hops, a slot outside the pool, a slot named twice; ss_last_error_string() names the first bad
 * entry -- and move only what the call touches: x, the tables and the n_active named pool rows up, the outputs and those rows
 * down; the caller's pool is written only after everything before it succeeded. */
/* host only, no device: ro[0] = 0, ro[i+1] = ro[i] + (so[i+1] - so[i]) / step.  SS_ERR_ARG: so[0] != 0, a decreasing pair, a chunk
 * that is not whole hops or longer than 2^31 - 1 samples; SS_ERR_BAD_CONFIG for literal / centred framing */
int ss_frame_stream_packed_row_offsets(const ss_params *p, size_t n_active, const int64_t *sample_offsets, int64_t *row_offsets);
/* device pointers, asynchronous on `stream`, graph-capturable: a linear chain of two launches (the rows, then the pool advance) */
int ss_mfcc_stream_packed_device(const ss_config *cfg, const float *d_x, size_t n_active, const int64_t *d_sample_offsets,
                                 const int64_t *d_row_offsets, size_t total_rows, const int32_t *d_slots, size_t pool_streams,
                                 uint32_t norm_frames, float *d_pool, float *d_out, void *stream);
int ss_mfe_stream_packed_device(const ss_config *cfg, const float *d_x, size_t n_active, const int64_t *d_sample_offsets,
                                const int64_t *d_row_offsets, size_t total_rows, const int32_t *d_slots, size_t pool_streams,
                                float *d_pool, float *d_feat, float *d_energy, void *stream);
/* host pointers, synchronous; the tables are host arrays; out: [ro[n_active] x num_cepstral] (feat / energy likewise) */
int ss_mfcc_stream_packed(const ss_config *cfg, const float *x, size_t n_active, const int64_t *sample_offsets,
                          const int32_t *slots, size_t pool_streams, uint32_t norm_frames, float *pool, float *out);
int ss_mfe_stream_packed(const ss_config *cfg, const float *x, size_t n_active, const int64_t *sample_offsets,
                         const int32_t *slots, size_t pool_streams, float *pool, float *feat, float *energy);

/* ---- the same pool fed signed 16-bit PCM ----
 * Live audio arrives as int16 (RTP, WAV, capture devices).  These four entry points take the packed chunks as int16 and convert
 * on load: stream sample s = (float)pcm * scale.  Everything else is the float pool's contract above, word for word -- entries,
 * R_i = 0, slots, total_rows, containment and the error word, capturability as a two-launch linear chain whose grids depend on
 * n_active and total_rows only, the host forms' table checks and the rule that the caller's pool is written only after everything
 * before it succeeded.  Offsets are in samples, not bytes.  The pool stays float: a stream may be fed PCM on one call and floats
 * on the next.
 *   scale: a power of two in [2^-64, 2^64], otherwise SS_ERR_ARG -- 2^-15 for normalised audio, 1.0 for integer-valued floats
 *   (the python_speech_features habit).  With a power of two the product is exact, so fusing it into what follows changes no bit.
 *   Equivalence: per entry the rows, and the pool row afterwards, are bit for bit those of ss_mfcc_stream_packed_device /
 *   ss_mfe_stream_packed_device on the float buffer x_f[k] = (float)pcm[k] * scale with the same tables, the same pool and the
 *   same norm_frames.
 *   Kernels: the float call's kernel family with a PCM loader, by the same selection rule -- ss_mfcc_c256spi<10,exact,bank421,sym>
 *   / ss_mfcc_c256spi<10,exact,bank421,mfe> for the default 512-point shape, ss_front_generic_fstreampi<LOG2C[,chirpz]> for every
 *   other configuration, then ss_stream_advance_packed_i16 (skipped where S == 0).
 *   Alignment: d_x must be 4-byte aligned in the device forms (a sample pair is one dword), SS_ERR_ARG otherwise; the host forms
 *   stage the buffer and have no such rule.
 * The scale and alignment checks come before any launch and before the pool or the outputs are touched. */
int ss_mfcc_stream_packed_i16_device(const ss_config *cfg, const int16_t *d_x, size_t n_active, const int64_t *d_sample_offsets,
                                     const int64_t *d_row_offsets, size_t total_rows, const int32_t *d_slots, size_t pool_streams,
                                     float scale, uint32_t norm_frames, float *d_pool, float *d_out, void *stream);
int ss_mfe_stream_packed_i16_device(const ss_config *cfg, const int16_t *d_x, size_t n_active, const int64_t *d_sample_offsets,
                                    const int64_t *d_row_offsets, size_t total_rows, const int32_t *d_slots, size_t pool_streams,
                                    float scale, float *d_pool, float *d_feat, float *d_energy, void *stream);
int ss_mfcc_stream_packed_i16(const ss_config *cfg, const int16_t *x, size_t n_active, const int64_t *sample_offsets,
                              const int32_t *slots, size_t pool_streams, float scale, uint32_t norm_frames, float *pool, float *out);
int ss_mfe_stream_packed_i16(const ss_config *cfg, const int16_t *x, size_t n_active, const int64_t *sample_offsets,
                             const int32_t *slots, size_t pool_streams, float scale, float *pool, float *feat, float *energy);

/* ---- ragged streaming STFT / mel spectrogram over a pool of stream states ----
 * The frame-path pool above, carried over to the STFT path (ss_stft_stream* / ss_mel_spectrogram_stream*), SS_STREAM_CONTINUOUS
 * only: SS_STREAM_REFERENCE's partial chunks and trailing n_pad zero rows have no meaning for a live pool.  H = the hop of
 * ss_stft_sizes, W = fft_points, S = ss_stream_state_len = W - H; a config without an STFT path (W < 2H) is SS_ERR_BAD_CONFIG.
 *   Pool: a caller-owned block [pool_streams x S] of floats -- the state block of ss_*_stream_device, row for row (all zeros =
 *   fresh stream, zeroing a row resets it).
 *   Entries: a call serves n_active entries.  Entry i's chunk is x[so[i] : so[i+1]] of one packed buffer (so: n_active + 1
 *   non-decreasing int64 sample offsets, so[0] = 0); its length n_i is a whole number of hops R_i = n_i / H, and R_i = 0 is legal:
 *   no rows, the state row untouched.  Its state is pool row slots[i] (int32, 0 <= slots[i] < pool_streams, distinct within a
 *   call).  Its rows are rows ro[i] .. ro[i+1] of the packed row space (ro: n_active + 1 row offsets, ro[0] = 0, ro[i+1] - ro[i] =
 *   R_i; from ss_stream_packed_row_offsets or computed by the caller on the device).
 *   Outputs: mel -- entry i's block [num_filters x R_i] is contiguous at out + num_filters * ro[i] (the layout of
 *   ss_mel_spectrogram_packed, and of the dense stream with n_streams = 1); stft -- [total_rows x (W/2+1) x 2], entry i owns rows
 *   ro[i] .. ro[i+1].  total_rows is the rows the output holds (>= ro[n_active]; rows at or past ro[n_active] are left alone).
 *   Equivalence: per entry the rows, and the pool row afterwards, are what ss_mel_spectrogram_stream_device /
 *   ss_stft_stream_device give in SS_STREAM_CONTINUOUS mode for that stream alone (n_streams = 1, that chunk, that state row),
 *   wherever the entry stands in the call and whatever else shares the call -- bit for bit where both run the same kernel family
 *   and build (below).  Every switch and bank of the config applies.  Pool rows not named in `slots` are neither read nor written.
 *   Kernels: mel output on a 2048-point configuration whose bank fits the dedicated kernel's twelve-wave build runs on its ragged
 *   streaming build, reported by ss_last_kernel_name() as ss_mel_c1024sp<w12,mel6321> / ss_mel_c1024sp<w12> -- always twelve
 *   waves, so that an entry's bits do not depend on what shares the call.  The dense stream picks eight or twelve waves by its
 *   unit count, and the two builds round a few FMAs differently in the last bit: the pool equals the dense stream bit for bit
 *   where that one runs ss_mel_c1024s<w12...> too; a lone small dense call picks eight waves and agrees to that last-bit rounding
 *   only.  Everything else the dense generic streaming build serves -- any fft_points, chirp-z included; every bank; all stft
 *   output -- runs on ss_front_generic_streamp<LOG2C[,chirpz]> with the bits of ss_front_generic_stream<...>.  A second
 *   stream-ordered launch (ss_stream_advance_packed, the frame pool's) moves the named pool rows on.  The device forms are a linear
 *   chain of these two launches whose grids depend on n_active and total_rows only: capturable, and replayable with other table
 *   contents.
 *   Containment: exactly the frame pool's.  The device forms never see the tables on the host.  Both kernels decode every entry
 *   with one shared function (the frame pool's); an entry is skipped -- no row written, its pool row untouched -- unless
 *   so[i] >= 0, 0 <= n_i <= 2^31 - 1, n_i % H == 0, ro[i] >= 0, ro[i+1] - ro[i] == n_i / H, ro[i+1] <= total_rows and
 *   0 <= slots[i] < pool_streams.  Whatever the tables hold, nothing is read or written outside x's entry ranges, rows
 *   [0, total_rows) of the output and rows [0, pool_streams) of the pool.  A skipped entry raises the config's device error word:
 *   the call itself returns SS_OK, the next call on the config (or ss_config_device_status) returns SS_ERR_DEVICE once.
 *   Duplicate slots in a device-form call are a caller error that is NOT detected: the rows and the pool rows of the entries
 *   that share a slot are unspecified; everything stays inside the pool.  The host-pointer forms reject them.
 * Arguments: n_active == 0 is SS_OK with nothing launched.  SS_ERR_ARG, pool and output untouched: null buffers, n_active,
 * pool_streams or total_rows >= 2^31, pool_streams == 0, a pool range that overlaps x or the output (the device forms know x by
 * its first sample; the host forms check its whole range).  The host-pointer forms also check the tables before they touch the
 * device -- so[0] != 0, a decreasing pair, a chunk that is not whole hops, a slot outside the pool, a slot named twice;
 * ss_last_error_string() names the first bad entry -- and move only what the call touches: x, the tables and the n_active named
 * pool rows up, the output and those rows down; the caller's pool is written only after everything before it succeeded. */
/* host only, no device: ro[0] = 0, ro[i+1] = ro[i] + (so[i+1] - so[i]) / H.  SS_ERR_ARG: so[0] != 0, a decreasing pair, a chunk
 * that is not whole hops or longer than 2^31 - 1 samples; SS_ERR_BAD_CONFIG for a config with no STFT path */
int ss_stream_packed_row_offsets(const ss_params *p, size_t n_active, const int64_t *sample_offsets, int64_t *row_offsets);
/* device pointers, asynchronous on `stream`, graph-capturable: a linear chain of two launches (the rows, then the pool advance) */
int ss_mel_spectrogram_stream_packed_device(const ss_config *cfg, const float *d_x, size_t n_active, const int64_t *d_sample_offsets,
                                            const int64_t *d_row_offsets, size_t total_rows, const int32_t *d_slots,
                                            size_t pool_streams, float *d_pool, float *d_out, void *stream);
int ss_stft_stream_packed_device(const ss_config *cfg, const float *d_x, size_t n_active, const int64_t *d_sample_offsets,
                                 const int64_t *d_row_offsets, size_t total_rows, const int32_t *d_slots, size_t pool_streams,
                                 float *d_pool, float *d_out, void *stream);
/* host pointers, synchronous; the tables are host arrays; out: num_filters * ro[n_active] floats (mel) /
 * ro[n_active] * (fft_points/2+1) * 2 floats (stft) */
int ss_mel_spectrogram_stream_packed(const ss_config *cfg, const float *x, size_t n_active, const int64_t *sample_offsets,
                                     const int32_t *slots, size_t pool_streams, float *pool, float *out);
int ss_stft_stream_packed(const ss_config *cfg, const float *x, size_t n_active, const int64_t *sample_offsets,
                          const int32_t *slots, size_t pool_streams, float *pool, float *out);
/* The same pool fed signed 16-bit PCM chunks: chunk sample s = (float)pcm * scale, scale a power of two in [2^-64, 2^64] (else
 * SS_ERR_ARG before anything is launched or touched), behind the sample-layout arguments; the offsets stay in samples.  The pool
 * stays float, so a stream may be fed PCM on one tick and floats on the next.  Every output row, and every pool row afterwards, is
 * bit for bit what the float form leaves on x_f[k] = (float)pcm[k] * scale; everything else -- errors, R_i = 0 entries, slots,
 * total_rows, containment and the error word, the duplicate-slot rules, capturability as a two-launch linear chain -- is the float
 * forms' contract.  Kernels: ss_mel_c1024spi<...> (the ragged streaming twelve-wave build) or ss_front_generic_streampi<...>
 * (everything else, all stft output), then ss_stream_advance_packed_i16 -- the frame pool's; no call converts first.
 *   Alignment: the device forms take a 4-byte aligned d_x only (else SS_ERR_ARG), as the frame pool's _i16 forms; the host forms
 *   stage the buffer and have no alignment rule.  The pool / x / output overlap checks work in bytes of the int16 buffer. */
int ss_mel_spectrogram_stream_packed_i16_device(const ss_config *cfg, const int16_t *d_x, size_t n_active, const int64_t *d_sample_offsets,
                                                const int64_t *d_row_offsets, size_t total_rows, const int32_t *d_slots,
                                                size_t pool_streams, float scale, float *d_pool, float *d_out, void *stream);
int ss_stft_stream_packed_i16_device(const ss_config *cfg, const int16_t *d_x, size_t n_active, const int64_t *d_sample_offsets,
                                     const int64_t *d_row_offsets, size_t total_rows, const int32_t *d_slots, size_t pool_streams,
                                     float scale, float *d_pool, float *d_out, void *stream);
int ss_mel_spectrogram_stream_packed_i16(const ss_config *cfg, const int16_t *x, size_t n_active, const int64_t *sample_offsets,
                                         const int32_t *slots, size_t pool_streams, float scale, float *pool, float *out);
int ss_stft_stream_packed_i16(const ss_config *cfg, const int16_t *x, size_t n_active, const int64_t *sample_offsets,
                              const int32_t *slots, size_t pool_streams, float scale, float *pool, float *out);

/* ss_stack_frames_signal on device pointers (d_window: frame_len floats in device memory, or NULL) */
int ss_stack_frames_signal_device(const float *d_x, size_t n_samples, uint32_t sample_rate, float frame_length, float frame_stride,
                                  const float *d_window, int zero_padding, float *d_frames, void *stream);

/* ---- post-processing on the feature matrix (row-major [rows x cols] f32) ---------- */

/* speechsauce::processing::cmvn(ArrayView2<f32>, variance_normalization) -> Array2<f32>  (processing.rs:265-300):
 * subtract the column means; optionally divide by (population std + 2^-30).  The std is the deviation about the column's mean,
 * evaluated in f64 as sqrt(sum((x - K)^2) / rows - (mean - K)^2) with K the column's first row: both terms are of the order of the
 * column's spread, so a column that moves by a few ulps around a large offset (a log-mel band at its floor) is normalised as the
 * two-pass definition says; only a first row that lies more than about 1e6 spreads from the rest costs digits.  A column that
 * holds a NaN or an infinity comes out non-finite in every row (as the reference's does); the other columns are not touched. */
int ss_cmvn(const float *vec, size_t rows, size_t cols, int variance_normalization, float *out);
/* the same for `batch` matrices stored back to back ([batch x rows x cols], e.g. the block ss_mfcc_batch_device wrote) */
int ss_cmvn_batch_device(const float *d_vec, size_t batch, size_t rows, size_t cols, int variance_normalization,
                         float *d_out, void *stream);
/* speechsauce::processing::cmvnw(Array2<f32>, win_size = 301, variance_normalization)  (processing.rs:315-371):
 * sliding-window normalisation over win_size rows of the symmetric-padded matrix (np.pad 'symmetric', util.rs:108-115).
 * SS_ERR_BAD_CONFIG for an even win_size (the reference asserts).
 * The window sums slide over the rows in f64 (add the row that enters, subtract the row that leaves).  Domain: a finite value
 * more than about 1e7 times the spread of the rows around it leaves a rounding residue of its square in those sums for the rest
 * of its chunk of rows (1e8 in N(1, 3) data: up to 6e-4 of an element at win_size 3; 1e12: garbage); up to 1e6 times the spread
 * the rows behind it are unaffected (tested).  A NaN or an infinity makes exactly the rows non-finite whose window holds it --
 * within (win_size - 1) / 2 rows of it, twice that with variance normalisation, as in the reference: a window that holds a NaN
 * gives NaN, never a number, and sums that are not finite after a step are formed afresh from the window, so the rows behind the
 * value are normalised as if it had never been there.  Finite input never takes that path. */
int ss_cmvnw(const float *vec, size_t rows, size_t cols, size_t win_size, int variance_normalization, float *out);
int ss_cmvnw_batch_device(const float *d_vec, size_t batch, size_t rows, size_t cols, size_t win_size,
                          int variance_normalization, float *d_out, void *stream);
/* speechsauce::processing::derivative_extraction(&Array2<f32>, delta_windows)  (processing.rs:222-254): edge-padded
 * differences along the FEATURE axis, sum_R (R f[c+R] - f[c-R]) / sum_R 2R^2 (the reference's literal arithmetic).
 * Rows are independent, so a [batch x rows x cols] block is passed as batch*rows rows. */
int ss_derivative_extraction(const float *feat, size_t rows, size_t cols, size_t delta_windows, float *out);
int ss_derivative_extraction_device(const float *d_feat, size_t rows, size_t cols, size_t delta_windows, float *d_out,
                                    void *stream);
/* speechsauce::feature::extract_derivative_feature(Array2<f32>) -> Array3<f32>  (feature.rs:253-269):
 * cube [rows x cols x 3] = (feature, derivative_extraction(feature, 2), derivative_extraction(that, 2)) */
int ss_extract_derivative_feature(const float *feat, size_t rows, size_t cols, float *cube);
int ss_extract_derivative_feature_device(const float *d_feat, size_t rows, size_t cols, float *d_cube, void *stream);

/* lmfe (feature.rs:242-245, README.md:14 "log mel filterbank energies"): ln of mfe's zero-handled energies, [frames x
 * num_filters].  d_energy may be NULL (the frame energies mfe also produces are then kept in a stream-ordered temporary). */
int ss_lmfe(const ss_config *cfg, const float *x, size_t n_samples, float *feat);
int ss_lmfe_batch(const ss_config *cfg, const float *x, size_t batch, size_t n_samples, size_t ld, float *feat);
int ss_lmfe_batch_device(const ss_config *cfg, const float *d_x, size_t batch, size_t n_samples, size_t ld,
                         float *d_feat, float *d_energy, void *stream);
/* in-place natural logarithm of n device floats (the element-wise pass of lmfe; util.rs:372-381) */
int ss_ln_device(float *d_x, size_t n, void *stream);
/* librosa.power_to_db (the reference's stated remaining work, README.md:44-46): 10 log10(max(amin, S)) - 10 log10(max(amin,
 * |ref|)), then floored at max(result) - top_db; top_db < 0 switches the floor off.  amin > 0. */
int ss_power_to_db(const float *s, size_t n, float ref, float amin, float top_db, float *out);
int ss_power_to_db_device(const float *d_s, size_t n, float ref, float amin, float top_db, float *d_out, void *stream);

/* ---- post-processing of packed variable-length clips (a loop over processing::cmvn / cmvnw, feature::lmfe, power_to_db per clip) ----
 * The normalising steps behind the packed calls above.  A segment table is the offsets array those calls return: `offsets`,
 * n_clips + 1 non-decreasing entries with offsets[0] = 0 (fo of ss_packed_frame_offsets, ro of ss_packed_row_offsets); clip b owns
 * rows offsets[b] .. offsets[b+1] of a row-major [total_rows x cols] float block.  Per clip, every result is what the one-matrix
 * call returns for that clip alone:
 *   cmvn_packed         ss_cmvn on the clip's rows: its own column means and population std (+ 2^-30), the std evaluated as in
 *                       ss_cmvn about the CLIP's first row of the column, so it depends on the clip's own rows only.
 *   cmvnw_packed        ss_cmvnw on the clip's rows: the np.pad 'symmetric' reflection happens at the clip's own first and last row
 *                       (period 2 * rows_b: a window wider than the clip wraps inside the clip, never into a neighbour).  An even
 *                       win_size is SS_ERR_BAD_CONFIG.
 *   power_to_db_packed  clip b's segment is elements cols * offsets[b] .. cols * offsets[b+1] -- the layout of the frame blocks and of
 *                       the [num_filters x R_b] mel blocks of ss_mel_spectrogram_packed (cols = num_filters, offsets = ro).  The
 *                       arithmetic of ss_power_to_db_device, with the top_db floor of an element at max(its own clip's result) -
 *                       top_db; top_db < 0 switches the floor off.
 *   lmfe_packed         ss_mfe_packed* followed by the in-place ln (feature.rs:242-245); d_energy may be NULL as in
 *                       ss_lmfe_batch_device.  Tables and errors as ss_mfe_packed_device (after SS_ERR_DEVICE the block's contents are
 *                       unspecified).
 * n_clips == 0 is SS_OK with nothing launched (for the three config-free calls also on a host without a device); an empty segment
 * writes nothing; null buffers, cols == 0, total_rows / cols / n_clips >= 2^31 are SS_ERR_ARG.
 * Host-pointer forms (synchronous; offsets is a host array) check the table before they touch the device: offsets[0] != 0, a
 * decreasing pair, offsets[n_clips] > total_rows are SS_ERR_ARG with the first bad clip named in ss_last_error_string.  Rows past
 * offsets[n_clips] are left as they were.
 * Device forms (asynchronous on `stream`, d_offsets a DEVICE array that only the kernels read) are graph-capturable as a linear
 * chain: cmvn one launch and no scratch; cmvnw one launch, with variance normalisation two and a stream-ordered scratch block;
 * power_to_db two launches and one stream-ordered word per clip.  The launch count does not depend on n_clips.  They have no
 * config to carry an error word, so their contract for a bad table is containment: a segment that is reversed, starts below 0 or
 * ends past total_rows is skipped, no kernel reads or writes outside [0, total_rows) x cols whatever the table holds, and rows
 * that belong to no valid segment are left unwritten.  (Valid segments that overlap -- possible only in a table that is not
 * monotone -- race with each other inside the block.)
 * Results are bit-reproducible (f64 accumulators in a fixed order, no float atomics) and position independent: the bits of clip
 * b's output depend on clip b's rows and the scalar arguments only, not on the clip's place in the block or on its neighbours. */
int ss_cmvn_packed(const float *vec, size_t n_clips, const int64_t *offsets, size_t total_rows, size_t cols,
                   int variance_normalization, float *out);
int ss_cmvnw_packed(const float *vec, size_t n_clips, const int64_t *offsets, size_t total_rows, size_t cols, size_t win_size,
                    int variance_normalization, float *out);
int ss_power_to_db_packed(const float *s, size_t n_clips, const int64_t *offsets, size_t total_rows, size_t cols, float ref,
                          float amin, float top_db, float *out);
/* feat: [fo[n_clips] x num_filters], fo = ss_packed_frame_offsets of sample_offsets */
int ss_lmfe_packed(const ss_config *cfg, const float *x, size_t n_clips, const int64_t *sample_offsets, float *feat);
int ss_cmvn_packed_device(const float *d_vec, size_t n_clips, const int64_t *d_offsets, size_t total_rows, size_t cols,
                          int variance_normalization, float *d_out, void *stream);
int ss_cmvnw_packed_device(const float *d_vec, size_t n_clips, const int64_t *d_offsets, size_t total_rows, size_t cols,
                           size_t win_size, int variance_normalization, float *d_out, void *stream);
int ss_power_to_db_packed_device(const float *d_s, size_t n_clips, const int64_t *d_offsets, size_t total_rows, size_t cols,
                                 float ref, float amin, float top_db, float *d_out, void *stream);
int ss_lmfe_packed_device(const ss_config *cfg, const float *d_x, size_t n_clips, const int64_t *d_sample_offsets,
                          const int64_t *d_frame_offsets, size_t total_frames, float *d_feat, float *d_energy, void *stream);

/* ---- causal sliding-window CMVN over a pool of stream states (the causal counterpart of processing::cmvnw, processing.rs:315-371) ----
 * The rows ss_mfcc_stream_packed* / ss_mfe_stream_packed* return are unnormalised; ss_cmvn needs the whole clip and ss_cmvnw centres
 * its window on the row, which a live stream cannot give.  These calls normalise every row over the TRAILING window of its own
 * stream, with the window carried from tick to tick in a pool of the same shape as the frame pool's.
 *   Definition (the reference crate has no causal variant: this is the specification): for one stream with rows x[0], x[1], ...
 *   counted since its reset, win = win_size >= 1 (any parity: a causal window has no centre), per column
 *     n_t = min(t + 1, win),  W_t = rows x[t - n_t + 1 .. t] (the row itself is the newest member),  mean_t = sum(W_t) / n_t
 *     out[t] = x[t] - mean_t                                    variance_normalization == 0
 *     out[t] = (x[t] - mean_t) / (std_t + 2^-30)                variance_normalization != 0
 *     std_t  = sqrt(sum((W_t - mean_t)^2) / n_t)                the population deviation about the window's mean; the eps of
 *                                                               processing.rs:324.  Evaluated in one walk of the window as
 *                                                               sqrt(max(sum((W_t - x[t])^2) / n_t - (mean_t - x[t])^2, 0)):
 *                                                               the squares are taken about the row itself, a member of the
 *                                                               window, so a window that moves by a few ulps around a large
 *                                                               offset keeps its digits (about the origin it would not, and
 *                                                               the bound below would fail).  A NaN passes the max.
 *   No padding at the start: the first rows use the rows that exist (as Kaldi's online CMVN).  win = 1 gives exact zeros; a column
 *   that is constant over the window gives exact zeros; with variance normalisation |out| <= sqrt(n_t).
 *   Arithmetic: both sums of every element (of the values, and with variance normalisation of their squared distances from x[t])
 *   are formed afresh in f64, oldest row first, from the f32 values -- never a running sum carried between rows or calls -- then
 *   static_cast<float>((double(x) - mean) * inv), inv = 1 / (std + 2^-30) or 1.  So a row's bits depend on its window's values
 *   only: not on how the stream was cut into calls, on the entry's place in the call or on its slot.
 *   Pool: a caller-owned block [pool_streams x L] of floats, L = ss_cmvn_stream_state_len = (win_size - 1) * cols + 1.  Floats
 *   0 .. (win_size - 1) * cols - 1 of a row are the stream's last win_size - 1 raw rows, oldest first, right-aligned (the newest row
 *   at the end, unused leading rows zero); the last float is the number of valid history rows, min(rows seen, win_size - 1), as a
 *   float.  All zeros = fresh stream, zeroing a row resets it.  A count word that is not an integer in [0, win_size - 1] (NaN
 *   included) is read as 0: garbage in the state never widens a read.
 *   Entries: vec / out are row-major [total_rows x cols]; entry i owns rows ro[i] .. ro[i+1] of both and pool row slots[i] --
 *   exactly the row_offsets and slots of an ss_mfcc_stream_packed* / ss_mfe_stream_packed* call, so the two calls chain on the same
 *   device tables.  R_i = 0 is legal: no row written, the pool row untouched bit for bit.  Rows past ro[n_active] and pool rows
 *   not named are neither read nor written.
 *   Device form: one launch (ss_cmvn_stream_packed_kernel, one workgroup per entry, which normalises the entry's rows and then
 *   moves its pool row on), asynchronous on `stream`, no scratch, graph-capturable as a single kernel node whose grid depends on
 *   n_active only.
 *   Containment: there is no config, so no error word.  An entry is skipped -- no row written, its pool row untouched -- unless
 *   0 <= ro[i] <= ro[i+1] <= total_rows and 0 <= slots[i] < pool_streams.  Whatever the tables and the pool's count words hold,
 *   nothing is read or written outside [0, total_rows) x cols of vec / out and [0, pool_streams) x L of the pool.  Duplicate slots
 *   in a device-form call are a caller error that is NOT detected: the rows and pool rows of those entries are unspecified;
 *   everything stays inside the pool.  The host-pointer form rejects them.
 * Arguments: n_active == 0 is SS_OK with nothing launched, also on a host without a device.  SS_ERR_ARG, decided before the device
 * is touched, pool and out untouched: null buffers (the pool too, also where win_size == 1 and L == 1); cols == 0, win_size == 0;
 * n_active, pool_streams, total_rows, cols or L >= 2^31, win_size > 2^24 (the count word must stay an exact float); pool_streams
 * == 0; out overlapping vec (an in-place call is NOT offered: later rows of an entry need the raw earlier rows); the pool range
 * overlapping vec or out.  The host-pointer form also checks the tables before it touches the device -- ro[0] != 0, a decreasing
 * pair, a slot outside the pool, a slot named twice; ss_last_error_string() names the first bad entry -- and moves only what the
 * call touches: vec, the tables and the n_active named pool rows up, out and those rows down; the caller's pool is written only
 * after everything before it succeeded. */
/* host only, no device: L = (win_size - 1) * cols + 1.  SS_ERR_ARG: cols == 0, win_size == 0, L >= 2^31, win_size > 2^24 */
int ss_cmvn_stream_state_len(size_t cols, size_t win_size, size_t *state_len);
/* device pointers, asynchronous on `stream`, graph-capturable: one launch whatever n_active is */
int ss_cmvn_stream_packed_device(const float *d_vec, size_t n_active, const int64_t *d_row_offsets, size_t total_rows,
                                 const int32_t *d_slots, size_t pool_streams, size_t cols, size_t win_size,
                                 int variance_normalization, float *d_pool, float *d_out, void *stream);
/* host pointers, synchronous; row_offsets / slots are host arrays; vec / out: [ro[n_active] x cols] */
int ss_cmvn_stream_packed(const float *vec, size_t n_active, const int64_t *row_offsets, const int32_t *slots,
                          size_t pool_streams, size_t cols, size_t win_size, int variance_normalization, float *pool, float *out);

/* ---- grouped CMVN: per-speaker and global statistics of packed rows, accumulated, merged, stored and applied ----
 * ss_cmvn_packed* normalises a clip by its own statistics, ss_cmvnw_packed* and the pool above by a sliding window.  These calls
 * are the other two normalisations in use: PER-SPEAKER CMVN (Kaldi's compute-cmvn-stats --spk2utt followed by apply-cmvn
 * --utt2spk: one set of column statistics over all of a speaker's utterances) and GLOBAL CMVN (WeNet global_cmvn, ESPnet
 * global_mvn, apply-cmvn with a stats file: statistics accumulated over a training set batch by batch, stored, and applied
 * unchanged at inference, live streams included).  The reference crate has neither: this comment is the specification.
 *   Statistics block: a group's statistics are one row of ss_cmvn_stats_len(cols) = 2 * cols + 1 doubles
 *       [ n | mean[cols] | var[cols] ]
 *   n the number of rows seen, held as a double; var the POPULATION variance.  All zeros = a fresh group; an n that is not finite
 *   or is below 1 is read as 0 (fresh), as the pools read a bad count word.  The block of a call is [n_groups x stats_len],
 *   caller-owned, updated in place.  clip_group is an int32 table [n_clips]: clip b belongs to group clip_group[b]; NULL means
 *   group 0 for every clip (global CMVN); -1 leaves a clip out.
 *   Per-clip statistics: clip b of T rows has exactly the statistics ss_cmvn_packed* forms: chunks = min(64, ceil(T / 32)) serial
 *   f64 sums of ceil(T / chunks) rows each, added in chunk order, the squares taken about the clip's own first row K of the column;
 *   mean_b = s1 / T, var_b = max(s2 / T - (mean_b - K)^2, 0).  mean_b is bit for bit the mean ss_cmvn_packed* subtracts.
 *   Merge: a group's row is the left fold of its clips into the prior row, in ascending clip index, in f64, every operation
 *   rounded on its own (no fused multiply-add), in this order (na, ma, va the row; nb = T, mb, vb the clip):
 *       n = na + nb;  wa = na / n;  wb = nb / n;  d = mb - ma;
 *       mean = ma + d * wb;
 *       var  = (wa * va + wb * vb) + (d * d) * (wa * wb);
 *   For na == 0 the clip's statistics are copied.  An empty or skipped clip takes no step.  This is Chan's merge in variance form:
 *   both terms of var are of the order of the spread squared, so a column that barely moves around a large offset keeps its
 *   digits.  It is a strict left fold: the bits do not depend on how the clips were cut into calls (two calls over a split of the
 *   clips equal one call), on the other groups' clips or on a clip's place in the block.  A group with no valid clip in a call
 *   keeps its row bit for bit.
 *   Apply: out = (float)(((double)x - mean_g) * inv_g), inv_g = 1 / (sqrt(var_g) + 2^-30) with variance normalisation and 1
 *   without: the finishing arithmetic of ss_cmvn_packed*.  out == vec is allowed (the call is element-wise); a partial overlap is
 *   SS_ERR_ARG.  A clip whose group has n < 1 is skipped.
 *   ss_cmvn_grouped_packed* is the per-speaker CMVN of one batch: statistics from fresh plus apply in one call on a stream-ordered
 *   scratch block; bit for bit ss_cmvn_stats_packed* on a zeroed block followed by ss_cmvn_apply_packed*.
 *   Device forms: asynchronous on `stream`, the tables are DEVICE arrays that only the kernels read, graph-capturable as a linear
 *   chain, and a captured graph replays over changed tables.  The launch count does not depend on n_clips or n_groups: statistics
 *   two kernels and one scratch block [n_clips x 2 cols] of doubles, apply one kernel, the combined call three kernels and a
 *   memset.  No float atomics: results are bit-reproducible.  The scratch is a stream-ordered allocation, except inside a stream
 *   capture: there it is one plain device block per device, which every statistics or combined call OUTSIDE a capture grows to
 *   its own scratch size.  So run the call once with the capture's sizes (or larger) before capturing it, as a warm-up does; a
 *   captured call that finds the block too small is SS_ERR_HIP with nothing put on the stream.  Graphs that hold a statistics or
 *   combined call share the block: replay them one after the other, not concurrently.  (Apply has no scratch.)
 *   Containment (device forms): a clip is skipped if its segment is reversed, starts below 0 or ends past total_rows, or if its
 *   group id lies outside [0, n_groups); under apply also if its group has n < 1.  A skipped clip contributes nothing and its rows
 *   are left unwritten; no address outside the blocks is formed whatever the tables hold.  The apply kernel finds the clip of a
 *   row by binary search in d_offsets: where the table is not non-decreasing, rows of otherwise valid clips may be left
 *   unwritten too (never written wrongly, never outside the block).
 *   Arguments: n_clips == 0 is SS_OK with nothing launched, also on a host without a device.  SS_ERR_ARG: null vec / offsets /
 *   stats / out; cols == 0; n_groups == 0; total_rows, n_clips or n_groups >= 2^31, cols >= 2^30; the statistics block overlapping
 *   vec (stats) or out (apply); out overlapping vec other than out == vec.  Host-pointer forms (synchronous) check the tables
 *   before they touch the device -- offsets[0] != 0, a decreasing pair, a clip past total_rows, a group id below -1 or >= n_groups
 *   -- and name the first bad clip in ss_last_error_string(); rows of clips that are left out keep the caller's bytes.
 *   The stream pools need no state for this: a pool tick's output is a packed block with its row_offsets, so
 *   ss_cmvn_apply_packed_device(d_rows, n_active, d_row_offsets, total_rows, cols, NULL or a per-entry speaker table, ...) is the
 *   online global (or per-speaker) CMVN of the tick, and can be captured behind the tick's call.
 *   Kaldi interchange (host only, f64): one row converts to and from Kaldi's [2 x (cols + 1)] accumulator, row 0 = sum x | count,
 *   row 1 = sum x^2 | 0 -- the layout of cmvn.ark and of WeNet's mean_stat / var_stat / frame_num.  to_kaldi: sum x = n * mean,
 *   sum x^2 = n * (var + mean^2).  from_kaldi: mean = sum x / n, var = max(sum x^2 / n - mean^2, 0); count < 1 (or not finite)
 *   gives a fresh row.  Only from_kaldi carries Kaldi's own one-pass conditioning (the difference of two numbers of the order of
 *   mean^2); rows formed by ss_cmvn_stats_packed* do not, and to_kaldi followed by from_kaldi loses what the accumulator form
 *   cannot hold.
 *   Not offered: weighted frames, --norm-means=false, 16-bit rows, a decaying or online-updating global statistic. */
/* host only, no device: *len = 2 * cols + 1.  SS_ERR_ARG: cols == 0, cols >= 2^30 */
int ss_cmvn_stats_len(size_t cols, size_t *len);
int ss_cmvn_stats_to_kaldi(const double *stats, size_t cols, double *kaldi);
int ss_cmvn_stats_from_kaldi(const double *kaldi, size_t cols, double *stats);
int ss_cmvn_stats_packed_device(const float *d_vec, size_t n_clips, const int64_t *d_offsets, size_t total_rows, size_t cols,
                                const int32_t *d_clip_group, size_t n_groups, double *d_stats, void *stream);
int ss_cmvn_apply_packed_device(const float *d_vec, size_t n_clips, const int64_t *d_offsets, size_t total_rows, size_t cols,
                                const int32_t *d_clip_group, size_t n_groups, const double *d_stats, int variance_normalization,
                                float *d_out, void *stream);
int ss_cmvn_grouped_packed_device(const float *d_vec, size_t n_clips, const int64_t *d_offsets, size_t total_rows, size_t cols,
                                  const int32_t *d_clip_group, size_t n_groups, int variance_normalization, float *d_out,
                                  void *stream);
int ss_cmvn_stats_packed(const float *vec, size_t n_clips, const int64_t *offsets, size_t total_rows, size_t cols,
                         const int32_t *clip_group, size_t n_groups, double *stats);
int ss_cmvn_apply_packed(const float *vec, size_t n_clips, const int64_t *offsets, size_t total_rows, size_t cols,
                         const int32_t *clip_group, size_t n_groups, const double *stats, int variance_normalization, float *out);
int ss_cmvn_grouped_packed(const float *vec, size_t n_clips, const int64_t *offsets, size_t total_rows, size_t cols,
                           const int32_t *clip_group, size_t n_groups, int variance_normalization, float *out);

/* ---- time-axis delta features (Kaldi's add-deltas) on packed clips and over a pool of stream states ----
 * ss_derivative_extraction* above mirror the reference, which differences along the FEATURE axis.  These calls append the
 * regression deltas over neighbouring FRAMES that HTK, Kaldi add-deltas, python_speech_features.delta and
 * torchaudio.functional.compute_deltas(mode="replicate") mean.  The reference crate has none: this is the specification.
 *   Parameters: order in {1, 2}, window >= 1, lag L = order * window <= 32.
 *   Taps (integers): k0 = [1], ko = k(o-1) convolved with [-window, .., -1, 0, 1, .., window]; Do = (2 * sum n^2, n = 1..window)^o.
 *   order 1, window 2: [-2,-1,0,1,2] / 10; order 2, window 2: [4,4,1,-4,-10,-4,1,4,4] / 100.
 *   One clip or stream with rows x[0 .. T-1], per column, for o = 1 .. order:
 *     acc = +0.0 (f64); for j = -o*window .. +o*window ascending, taps with ko[j] == 0 skipped:
 *         acc = acc + double(ko[j]) * double(x[clamp(t + j, 0, T - 1)])
 *     do[t] = float(acc * invo),  invo = 1.0 / double(Do) formed once on the host
 *   The clamp is on the RAW row index (edge replication of the clip itself): the second delta is the composite filter on the raw
 *   rows, not the first delta applied to an edge-padded first delta (the two differ within 2 * window rows of a clip's ends).
 *   Every product is exact in f64, so the bits depend on the summation order only (not on FMA contraction), there is no f64
 *   division on the device, a constant column gives exact +0.0, and a NaN / Inf at row t reaches exactly the outputs whose
 *   non-zero taps cover row t (the first delta of row t itself stays finite: its centre tap is zero).
 *   Output row: [ x[t] | d1[t] | d2[t] ], (order + 1) * cols floats (Kaldi's layout); the static block is a bit copy.
 * Packed clips (ss_add_deltas_packed*): vec is [total_rows x cols], out is [total_rows x (order + 1) * cols], clip b owns rows
 * offsets[b] .. offsets[b+1] of both.  Contract, containment and argument rules are those of ss_cmvn_packed*: the table is a device
 * array that only the kernel reads; a segment that is reversed, starts below 0 or ends past total_rows is skipped; nothing outside
 * [0, total_rows) is touched; rows in no valid segment are left unwritten; one launch (ss_add_deltas_packed_kernel) whatever the
 * clip count; a clip's bits depend on its own rows and the scalars only.  A dense matrix is n_clips == 1.  n_clips == 0 is SS_OK
 * without a device.  SS_ERR_ARG, decided before the device is touched: null buffers, cols == 0, n_clips / total_rows / cols >=
 * 2^31, order outside {1, 2}, window == 0, L > 32, out overlapping vec.  The host form checks the table first and names the first
 * bad clip. */
int ss_add_deltas_packed_device(const float *d_vec, size_t n_clips, const int64_t *d_offsets, size_t total_rows, size_t cols,
                                size_t order, size_t window, float *d_out, void *stream);
int ss_add_deltas_packed(const float *vec, size_t n_clips, const int64_t *offsets, size_t total_rows, size_t cols, size_t order,
                         size_t window, float *out);
/* Pool of stream states, fixed latency L (ss_add_deltas_stream_*): deltas need L rows of look-ahead, so a live stream gets its
 * rows L rows late.  Pool: a caller-owned block [pool_streams x len] of floats, len = ss_add_deltas_stream_state_len = 2L * cols
 * + 1, laid out as the CMVN pool: the stream's last 2L raw rows, oldest first, right-aligned, zeros in front, then the count word
 * min(rows seen, 2L) as a float.  All zeros = fresh stream.  A count word that is not an integer in [0, 2L] (NaN included) is
 * read as 0.
 *   Entry i owns rows ro[i] .. ro[i+1] of vec [total_rows x cols] and of out [total_rows x (order + 1) * cols], and pool row
 *   slots[i]: it brings R_i raw rows and gets exactly R_i output rows, so the row_offsets / slots of the feature call and of
 *   ss_cmvn_stream_packed* are reused unchanged.  Output row k of the entry is the feature row of stream time tau = seen + k - L
 *   (seen: rows of the stream before this call).  tau < 0 (the first L rows after a reset): the whole row is +0.0, a warm-up row.
 *   tau >= 0: the row defined above with left clamping at stream row 0 and no right clamping (row tau + L has just arrived).
 *   R_i == 0 writes nothing and leaves the pool row bit for bit.
 *   Flush (ss_add_deltas_stream_flush*): entry i gets exactly L rows, out[i*L .. (i+1)*L) of [n_active * L x (order + 1) * cols]:
 *   the stream's last rows seen - L .. seen - 1 with right clamping at the stream's last row; times below 0 are +0.0 rows.
 *   Afterwards the pool row is all zeros (a fresh stream).
 *   Invariant: however a stream is cut into calls (empty entries included), the rows of all its calls plus the flush, the first L
 *   dropped, are bit for bit ss_add_deltas_packed* on the whole clip.
 *   One launch each (ss_add_deltas_stream_kernel), one workgroup per entry, asynchronous on `stream`, no scratch, graph-capturable
 *   as a single kernel node whose grid depends on n_active only.  Containment as ss_cmvn_stream_packed*: an entry is skipped -- no
 *   row written, its pool row untouched -- unless 0 <= ro[i] <= ro[i+1] <= total_rows and 0 <= slots[i] < pool_streams (flush: the
 *   slot rule); whatever the tables and count words hold, nothing outside the blocks is read or written.  Duplicate slots in a
 *   device-form call are a caller error that is NOT detected (results of those entries unspecified, everything stays inside the
 *   pool); the host forms reject them.
 * Arguments: n_active == 0 is SS_OK with nothing launched, also without a device.  SS_ERR_ARG, decided before the device is
 * touched, pool and out untouched: null buffers; cols == 0; order outside {1, 2}, window == 0, L > 32; n_active, pool_streams,
 * total_rows, cols or len >= 2^31; pool_streams == 0; out overlapping vec; the pool overlapping vec or out.  The host forms also
 * check the tables first -- ro[0] != 0, a decreasing pair, a slot outside the pool, a slot named twice; ss_last_error_string()
 * names the first bad entry -- and move only what the call touches; the caller's pool is written only after everything before it
 * succeeded. */
/* host only, no device: len = 2 * order * window * cols + 1 */
int ss_add_deltas_stream_state_len(size_t cols, size_t order, size_t window, size_t *state_len);
int ss_add_deltas_stream_packed_device(const float *d_vec, size_t n_active, const int64_t *d_row_offsets, size_t total_rows,
                                       const int32_t *d_slots, size_t pool_streams, size_t cols, size_t order, size_t window,
                                       float *d_pool, float *d_out, void *stream);
int ss_add_deltas_stream_packed(const float *vec, size_t n_active, const int64_t *row_offsets, const int32_t *slots,
                                size_t pool_streams, size_t cols, size_t order, size_t window, float *pool, float *out);
int ss_add_deltas_stream_flush_device(size_t n_active, const int32_t *d_slots, size_t pool_streams, size_t cols, size_t order,
                                      size_t window, float *d_pool, float *d_out, void *stream);
int ss_add_deltas_stream_flush(size_t n_active, const int32_t *slots, size_t pool_streams, size_t cols, size_t order, size_t window,
                               float *pool, float *out);

/* ---- frame splicing and subsampling on packed clips and over a pool of stream states ----
 * The stage a neural acoustic model takes behind normalised rows (with or without deltas): context splicing (Kaldi splice-feats
 * --left-context --right-context), frame subsampling (Kaldi subsample-feats --n) and low frame rate, the two combined: stack m
 * frames, skip n (FunASR / Paraformer lfr_m = 7, lfr_n = 6; "stack 4 skip 3").  The reference crate has none: this comment is the
 * specification.
 *   Parameters: cols >= 1; left, right in [0, 32]; stride in [1, 32] (the bound of ss_add_deltas*' L).  W = left + 1 + right; an
 *   output row has W * cols floats.
 *   One clip or stream with raw rows x[0 .. T-1]: T_out = ceil(T / stride) (T = 0: no rows); output row k is the concatenation, for
 *   c = -left .. +right ascending, of x[clamp(k * stride + c, 0, T - 1)].  Every output float is a BIT COPY of an input float: no
 *   arithmetic touches it, so NaN payloads, -0.0, infinities and denormals come through unchanged.
 *   stride = 1 is splice-feats; left = right = 0 is subsample-feats --n=stride; left = (m-1)/2, right = m-1-left, stride = n is
 *   FunASR's apply_lfr(m, n).
 * Packed clips (ss_splice_packed*): vec is [total_rows x cols], clip b owns rows ro[b] .. ro[b+1]; out is [total_out_rows x
 * W*cols], clip b owns rows oo[b] .. oo[b+1].  Both tables are device arrays of n_clips + 1 entries that only the kernel reads; oo
 * may be the same array as ro when stride == 1.  A clip is served iff 0 <= ro[b] <= ro[b+1] <= total_rows, oo[b] >= 0, oo[b+1] -
 * oo[b] == ceil((ro[b+1] - ro[b]) / stride) and oo[b+1] <= total_out_rows; any other clip is skipped whole.  Nothing outside the
 * two blocks is read or written; rows in no served clip stay unwritten.  One launch (ss_splice_packed_kernel) whatever the clip
 * count; a clip's bits depend on its own rows and the scalars only.  n_clips == 0 is SS_OK without a device.  SS_ERR_ARG, decided
 * before the device is touched: null buffers; cols == 0; a parameter outside its range; n_clips, total_rows, total_out_rows, cols
 * or W * cols >= 2^31; out overlapping vec.  ss_splice_packed_offsets (host only) forms oo from ro: oo[0] = 0, oo[b+1] = oo[b] +
 * ceil((ro[b+1] - ro[b]) / stride); it rejects null tables, a stride outside its range, n_clips >= 2^31 and a decreasing pair
 * (nothing is written then), and out_offsets may be row_offsets.  The host form takes row_offsets alone and forms oo itself; it
 * checks the table first and names the first bad clip (the rules of ss_add_deltas_packed) and writes the rows the table covers. */
int ss_splice_packed_offsets(size_t n_clips, const int64_t *row_offsets, size_t stride, int64_t *out_offsets);
int ss_splice_packed_device(const float *d_vec, size_t n_clips, const int64_t *d_row_offsets, size_t total_rows,
                            const int64_t *d_out_offsets, size_t total_out_rows, size_t cols, size_t left, size_t right,
                            size_t stride, float *d_out, void *stream);
int ss_splice_packed(const float *vec, size_t n_clips, const int64_t *row_offsets, size_t total_rows, size_t cols, size_t left,
                     size_t right, size_t stride, float *out);
/* Pool of stream states (ss_splice_stream_*): a live stream is fed WHOLE PERIODS of `stride` rows and gets one output row per
 * period, D = right / stride periods late (integer division; right = 3, stride = 6: D = 0, the centre's right context lies inside
 * its own period; right = 5, stride = 1: D = 5).  It carries H = D * stride + left raw rows.  Pool: a caller-owned block
 * [pool_streams x len] of floats, len = ss_splice_stream_state_len = H * cols + 1, laid out as the add-deltas pool: the stream's
 * last H raw rows, oldest first, right-aligned, zeros in front, then the count word min(rows seen, H) as a float.  All zeros =
 * fresh stream.  A count word that is not an integer in [0, H] (NaN included) is read as 0.  H = 0 keeps the one count word.
 *   Entry i owns rows ro[i] .. ro[i+1] of vec [total_rows x cols] and pool row slots[i]; its R_i rows are R_i / stride whole
 *   periods (zero is legal) and its output rows are rows ro[i] / stride .. ro[i+1] / stride of out [total_rows / stride x W*cols].
 *   Every ro[i] is a multiple of stride, so the row_offsets / slots of the feature call are reused unchanged: there is no second
 *   table.  Output row k of the entry has output index m = seen / stride + k - D (seen: rows of the stream before this call).
 *   m < 0: the whole row is +0.0, a warm-up row.  m >= 0: the row defined above with left clamping at stream row 0 and no right
 *   clamping (its last row m * stride + right <= seen + (k + 1) * stride - 1 has arrived).  Afterwards the pool row is the last H
 *   rows of (history ++ entry) and the new count.  R_i == 0 writes nothing and leaves the pool row bit for bit.
 *   Flush (ss_splice_stream_flush*): entry i gets exactly D rows, out[i*D .. (i+1)*D): output indices seen / stride - D .. seen /
 *   stride - 1 with right clamping at the stream's last row; indices below 0 are +0.0 rows.  Afterwards the pool row is all zeros.
 *   D == 0: no rows, d_out may be NULL, and the pool rows are still zeroed.
 *   Invariant: however a stream of K * stride rows is cut into calls (empty entries included), the rows of all its calls plus the
 *   flush, the first D dropped, are bit for bit ss_splice_packed* on the whole clip.
 *   A stream's end: a stream whose length is not a whole number of periods is padded by the caller, who repeats its last row up
 *   to a whole period before the last call.  That gives exactly the packed call on the unpadded clip, because the clamp replicates
 *   the same row.
 *   One launch each (ss_splice_stream_kernel), one workgroup per entry, one kernel node whose grid depends on n_active only,
 *   asynchronous on `stream`, no allocation, no scratch.  Containment as ss_add_deltas_stream_*: an entry is served only if 0 <=
 *   ro[i] <= ro[i+1] <= total_rows, ro[i] and R_i are multiples of stride and 0 <= slots[i] < pool_streams (flush: the slot rule);
 *   a skipped entry has no row written and its pool row untouched.  Whatever tables and count words hold, nothing outside the
 *   blocks is touched.  Duplicate slots in a device-form call are a caller error that is NOT detected; the host forms reject them.
 * Arguments: n_active == 0 is SS_OK with nothing launched, also without a device.  SS_ERR_ARG, decided before the device is
 * touched, pool and out untouched: null buffers; cols == 0; left, right or stride outside its range; n_active, pool_streams,
 * total_rows, cols or W * cols >= 2^31 (len is never more); pool_streams == 0; out overlapping vec; the pool overlapping vec or out.  The host
 * forms also check the tables first -- ro[0] != 0, a decreasing pair, an entry that is not whole periods, a slot outside the pool,
 * a slot named twice; ss_last_error_string() names the first bad entry -- and write the caller's pool last. */
/* host only, no device: len = (right / stride * stride + left) * cols + 1, delay_rows = right / stride */
int ss_splice_stream_state_len(size_t cols, size_t left, size_t right, size_t stride, size_t *state_len, size_t *delay_rows);
int ss_splice_stream_packed_device(const float *d_vec, size_t n_active, const int64_t *d_row_offsets, size_t total_rows,
                                   const int32_t *d_slots, size_t pool_streams, size_t cols, size_t left, size_t right,
                                   size_t stride, float *d_pool, float *d_out, void *stream);
int ss_splice_stream_packed(const float *vec, size_t n_active, const int64_t *row_offsets, const int32_t *slots,
                            size_t pool_streams, size_t cols, size_t left, size_t right, size_t stride, float *pool, float *out);
int ss_splice_stream_flush_device(size_t n_active, const int32_t *d_slots, size_t pool_streams, size_t cols, size_t left,
                                  size_t right, size_t stride, float *d_pool, float *d_out, void *stream);
int ss_splice_stream_flush(size_t n_active, const int32_t *slots, size_t pool_streams, size_t cols, size_t left, size_t right,
                           size_t stride, float *pool, float *out);

/* ---- fused splice + affine transform of packed rows (Kaldi splice-feats | transform-feats) ----
 * The matrix product that always follows the splice stage -- an LDA / LDA+MLLT matrix (40 x (7 * 13), 40 x (11 * 40 + 1)), the
 * linear input projection of a low-frame-rate front end, a PCA / whitening matrix, a global CMVN folded into a diagonal affine --
 * applied to the spliced row WITHOUT the spliced block ever being written: the rows are read once and out_dim floats per output
 * row are stored.  The reference crate has none: this comment is the specification.
 *   For every served clip b and output row k < ceil(T_b / stride): s_k is the spliced row ss_splice_packed* defines (rows k * stride
 *   - left .. k * stride + right of the clip side by side, clamped to the clip's own first and last row), K = (left + 1 + right) *
 *   cols its length, K4 = 4 * ceil(K / 4).  Output element i < out_dim of the row is the strict serial chain
 *       acc = bias[i]   (+0.0f without a bias);   for k = 0, 1, .., K4 - 1 ascending: acc = fmaf(M[i][k], s[k], acc);   out = acc
 *   in f32, one rounding per step, where BOTH factors are +0.0f for K <= k < K4.  The pad steps belong to the contract: fmaf(+0, +0,
 *   -0.0) is +0.0, so they are not invisible.  One accumulator per output element runs through all of k; K is never split across
 *   accumulators, lanes or waves.  So a row's bits are a pure function of its clip's rows, the matrix and the scalars -- not of
 *   its place in the block or the launch shape -- and a NaN / Inf in a row reaches exactly the outputs whose context holds that
 *   row.  (v_mfma_f32_16x16x4_f32 of gfx950 is this chain, four steps per instruction.)
 * The handle (ss_affine): ss_affine_create takes the matrix row-major [out_dim x in_dim] with row pitch ld >= in_dim floats and a
 * bias [out_dim] or NULL, re-lays it into the kernel's operand order and keeps that copy; the caller's arrays are not needed
 * afterwards.  Creation needs no device.  Limits: 1 <= out_dim <= 256 and 1 <= in_dim <= 4096, anything else is SS_ERR_UNSUPPORTED
 * (checked first, without a device); a null matrix, a null `out` or ld < in_dim is SS_ERR_ARG.  The first device call uploads the
 * table, once, to the device that is current then (a later call under another current device is SS_ERR_ARG); after that warm call
 * nothing is allocated or copied inside a launch.  A handle may be used from several threads / streams concurrently.
 * ss_affine_dims reports (out_dim, in_dim); ss_affine_chain_len (host only) is K4 for an in_dim inside the limit.
 * Packed clips (ss_affine_splice_packed*): vec is [total_rows x cols], clip b owns rows ro[b] .. ro[b+1]; out is [total_out_rows x
 * out_dim], clip b owns rows oo[b] .. oo[b+1].  Everything else is ss_splice_packed*'s: both tables are device arrays of n_clips +
 * 1 entries that only the kernel reads (ss_splice_packed_offsets forms oo; oo may be the same array as ro when stride == 1); a
 * clip is served iff 0 <= ro[b] <= ro[b+1] <= total_rows, oo[b] >= 0, oo[b+1] - oo[b] == ceil((ro[b+1] - ro[b]) / stride) and
 * oo[b+1] <= total_out_rows; any other clip is skipped whole.  Nothing outside the two blocks is read or written; rows in no served
 * clip stay unwritten.  The clip of an output row is looked up in oo, which therefore must not decrease across the served clips (the
 * tables of ss_splice_packed_offsets, of ss_select_rows_packed_device and a pool tick's row_offsets are valid as they stand; with
 * left = right = 0 and stride = 1 the call is plain transform-feats on any packed rows, e.g. behind ss_splice_stream_packed*).
 * One launch (ss_affine_splice_kernel) whose grid depends on total_out_rows, out_dim and in_dim only, asynchronous on `stream`, no
 * allocation, no read-back, no scratch: graph-capturable after the warm call and replayable over changed table contents.
 * n_clips == 0 is SS_OK without a device.  SS_ERR_ARG, decided before the device is touched: null buffers or handle; cols == 0; left
 * or right outside [0, 32], stride outside [1, 32]; n_clips, total_rows, total_out_rows, cols or W * cols >= 2^31; in_dim != (left +
 * 1 + right) * cols; out overlapping vec.  The host form takes row_offsets alone and forms oo itself; it checks the table first and
 * names the first bad clip (the rules of ss_splice_packed) and writes the rows the table covers. */
typedef struct ss_affine ss_affine; /* opaque: the matrix in operand order and, after the first device call, its device copy */
int ss_affine_create(const float *matrix, size_t out_dim, size_t in_dim, size_t ld, const float *bias_or_null, ss_affine **out);
void ss_affine_destroy(ss_affine *t);
int ss_affine_dims(const ss_affine *t, size_t *out_dim, size_t *in_dim);
/* host only, no device: k4 = 4 * ceil(in_dim / 4) */
int ss_affine_chain_len(size_t in_dim, size_t *k4);
int ss_affine_splice_packed_device(const ss_affine *t, const float *d_vec, size_t n_clips, const int64_t *d_row_offsets,
                                   size_t total_rows, const int64_t *d_out_offsets, size_t total_out_rows, size_t cols, size_t left,
                                   size_t right, size_t stride, float *d_out, void *stream);
int ss_affine_splice_packed(const ss_affine *t, const float *vec, size_t n_clips, const int64_t *row_offsets, size_t total_rows,
                            size_t cols, size_t left, size_t right, size_t stride, float *out);

/* ---- energy voice-activity decision and voiced-row selection on packed clips and over a pool of stream states ----
 * The two stages a speaker-recognition front end (x-vector / i-vector recipes, diarisation) takes behind the feature rows: Kaldi's
 * compute-vad-energy, a per-frame speech / non-speech decision from the log-energy column, and select-voiced-frames, which drops
 * the unvoiced rows of every clip.  The reference crate has neither: this comment is the specification.
 *   Parameters: cols >= 1; energy_col < cols; energy_threshold and energy_mean_scale finite; L = frames_context in [0, 32] (the
 *   bound of ss_add_deltas*' lag); 0 < proportion_threshold < 1 (Kaldi's assertion).  Kaldi's defaults are 5.0 / 0.5 / 0 / 0.6,
 *   the x-vector recipes use 5.5 / 0.5 / 2 / 0.12.
 *   One clip of T rows, e[t] = vec[t][energy_col]:
 *     thr = (double)energy_threshold + (double)energy_mean_scale * mean, a rounded f64 product and a rounded f64 sum; mean = s1 / T
 *     in f64, where s1 is formed in exactly the order in which ss_cmvn_packed* forms a column's sum: chunks = min(64, ceil(T / 32)),
 *     rpc = ceil(T / chunks), every chunk a serial f64 sum of its rpc rows (the last chunks may be short or empty), the chunk sums
 *     added serially in chunk order.  So the mean is bit for bit the mean ss_cmvn_packed* subtracts from that column.  Where
 *     energy_mean_scale == 0 the mean is not formed: thr = (double)energy_threshold, whatever the column holds elsewhere.
 *     Row u is raw-voiced iff (double)e[u] > thr (a NaN energy, or a NaN thr, compares false).
 *     num[t] = raw-voiced rows among t - L .. t + L that lie inside the clip; den[t] = the rows among them inside the clip.
 *     mask[t] = ((float)num[t] >= (float)den[t] * proportion_threshold) ? 1 : 0, the product ONE f32 multiply (Kaldi's int x float).
 *   THE ONE DEPARTURE FROM KALDI: thr is kept in f64, where Kaldi rounds energy_threshold + energy_mean_scale * mean to float
 *   before comparing.  A decision can differ from Kaldi's only for an energy within one float ulp of the threshold.
 * Packed clips, the decision (ss_vad_energy_packed*): vec is [total_rows x cols], clip b owns rows offsets[b] .. offsets[b+1] (a
 * device table of n_clips + 1 entries that only the kernel reads); d_mask [total_rows] gets one byte 0 / 1 per row, d_counts
 * [n_clips] (may be NULL) the voiced rows of every clip.  One launch (ss_vad_energy_packed_kernel) whatever the clip count; long
 * clips share workgroups and the bits do not depend on the split; no atomics.  Containment is that of ss_cmvn_packed_device: a
 * segment that is reversed, starts below 0 or ends past total_rows is skipped -- its mask bytes and its count word are left
 * unwritten -- and nothing outside [0, total_rows) is touched.  A valid clip without rows writes count 0.  n_clips == 0 is SS_OK
 * without a device.  SS_ERR_ARG, decided before the device is touched: null buffers (d_counts apart); cols == 0; energy_col >=
 * cols; L > 32; proportion_threshold outside (0, 1) or not finite; a non-finite threshold or mean scale; n_clips, total_rows or
 * cols >= 2^31.  The host form checks the table first and names the first bad clip (the rules of ss_cmvn_packed). */
int ss_vad_energy_packed_device(const float *d_vec, size_t n_clips, const int64_t *d_offsets, size_t total_rows, size_t cols,
                                size_t energy_col, float energy_threshold, float energy_mean_scale, size_t frames_context,
                                float proportion_threshold, uint8_t *d_mask, int64_t *d_counts, void *stream);
int ss_vad_energy_packed(const float *vec, size_t n_clips, const int64_t *offsets, size_t total_rows, size_t cols,
                         size_t energy_col, float energy_threshold, float energy_mean_scale, size_t frames_context,
                         float proportion_threshold, uint8_t *mask, int64_t *counts);
/* Packed clips, the selection (ss_select_rows_packed*): d_mask [total_rows] is ANY byte mask, a byte != 0 keeps its row.  The call
 * writes d_out_offsets [n_clips + 1]: oo[0] = 0, oo[b+1] = oo[b] + kept rows of clip b (a skipped segment contributes 0); clip b's
 * kept rows, in order, are rows oo[b] .. oo[b+1] of d_out [total_rows x cols] (the caller gives room for every row).  Every float is
 * a BIT COPY, as in ss_splice_*.  Rows at and past oo[n_clips] are left unwritten.  The device form is asynchronous with no
 * read-back: three launches (count, scan, move) whatever n_clips and total_rows, and one stream-ordered scratch block as
 * ss_cmvnw_packed_device uses; total_rows == 0 is one memset of the table.  d_out_offsets with total_rows as the bound is a valid
 * table for ss_cmvn_packed_device, ss_cmvnw_packed_device, ss_add_deltas_packed_device and ss_splice_packed_device, so the chain
 * goes on without the host ever learning the sizes.  Containment: a segment that is reversed, starts below 0 or ends past
 * total_rows keeps no row; a clip whose rows would end past total_rows (only a table whose clips overlap can ask for that) has no
 * row written; nothing outside the blocks is touched.  n_clips == 0 is SS_OK without a device (nothing is written).  SS_ERR_ARG,
 * decided before the device is touched: null buffers; cols == 0; n_clips, total_rows or cols >= 2^31; out overlapping vec or the
 * mask.  The host form checks the table first, names the first bad clip, and returns the table and the rows it covers. */
int ss_select_rows_packed_device(const float *d_vec, size_t n_clips, const int64_t *d_row_offsets, size_t total_rows, size_t cols,
                                 const uint8_t *d_mask, int64_t *d_out_offsets, float *d_out, void *stream);
int ss_select_rows_packed(const float *vec, size_t n_clips, const int64_t *row_offsets, size_t total_rows, size_t cols,
                          const uint8_t *mask, int64_t *out_offsets, float *out);
/* Pool of stream states, the decision only (ss_vad_energy_stream_*), on the row_offsets / slots of the feature pool call, with a
 * fixed latency of L = frames_context rows exactly as the add-deltas pool: an entry gets as many mask bytes as it brought rows,
 * the first L bytes of a fresh stream are 0 (warm-up), and the flush gives a stream's last L decisions.
 *   The causal threshold: the decision for stream row t uses thr_t = energy_threshold + energy_mean_scale * (S_n / n) in f64 (a
 *   division, a product and a sum, each rounded), n = min(t + L + 1, rows seen): every row that has arrived when t is decided, all
 *   rows in the flush.  S_n is ONE f64 accumulator advanced row by row in stream order -- that order is the definition.  Every
 *   member of the window t - L .. t + L is compared against thr_t; the window is clipped at the stream's first row and, in the
 *   flush, at its last.  With energy_mean_scale == 0 thr_t = energy_threshold (the accumulator is still advanced).
 *   Pool: a caller-owned block [pool_streams x len] of floats, len = ss_vad_energy_stream_state_len = 2 L + 4: the low and the high
 *   half of the f64 sum, bit-cast; the rows seen as a bit-cast uint32 (a stream of more than 2^32 - 1 rows is out of contract);
 *   the stream's last 2 L energies, oldest first, right-aligned, zeros in front; the count word min(rows seen, 2 L) as a float,
 *   last.  All zeros = fresh stream.  A count word that is not an integer in [0, 2 L], or rows seen below the count, reads as fresh.
 *   Entry i owns rows ro[i] .. ro[i+1] of vec, the same bytes of mask and pool row slots[i].  Byte k is the decision for stream row
 *   seen + k - L (0 where that is negative).  An entry without rows writes nothing and leaves its pool row bit for bit.
 *   Flush: entry i gets exactly L bytes, mask[i*L .. (i+1)*L): the decisions for rows seen - L .. seen - 1 (0 where negative);
 *   afterwards the pool row is all zeros.  L == 0: no bytes, d_mask may be NULL, and the pool rows are still zeroed.
 *   Invariants: with energy_mean_scale == 0, all of a stream's bytes plus the flush, the first L dropped, are ss_vad_energy_packed*
 *   on the whole clip byte for byte, however the stream was cut.  With a non-zero scale they are the causal definition's bytes,
 *   and the final pool rows do not depend on the cut.
 *   One launch each (ss_vad_energy_stream_kernel), one workgroup per entry, one kernel node whose grid depends on n_active only,
 *   asynchronous on `stream`, no allocation, no scratch.  Containment as ss_add_deltas_stream_*: an entry is served only if 0 <=
 *   ro[i] <= ro[i+1] <= total_rows and 0 <= slots[i] < pool_streams (flush: the slot rule); a skipped entry has no byte written and
 *   its pool row untouched.  Duplicate slots in a device-form call are a caller error that is NOT detected; the host forms reject
 *   them.
 * Arguments: n_active == 0 is SS_OK with nothing launched, also without a device.  SS_ERR_ARG, decided before the device is
 * touched, pool and mask untouched: null buffers; the scalar rules above; n_active, pool_streams, total_rows or cols >= 2^31;
 * pool_streams == 0; mask overlapping vec; the pool overlapping vec or mask.  The host forms also check the tables first -- ro[0] !=
 * 0, a decreasing pair, a slot outside the pool, a slot named twice; ss_last_error_string() names the first bad entry -- gather and
 * scatter the named pool rows, and write the caller's pool last. */
/* host only, no device: len = 2 * frames_context + 4 */
int ss_vad_energy_stream_state_len(size_t frames_context, size_t *state_len);
int ss_vad_energy_stream_packed_device(const float *d_vec, size_t n_active, const int64_t *d_row_offsets, size_t total_rows,
                                       const int32_t *d_slots, size_t pool_streams, size_t cols, size_t energy_col,
                                       float energy_threshold, float energy_mean_scale, size_t frames_context,
                                       float proportion_threshold, float *d_pool, uint8_t *d_mask, void *stream);
int ss_vad_energy_stream_packed(const float *vec, size_t n_active, const int64_t *row_offsets, const int32_t *slots,
                                size_t pool_streams, size_t cols, size_t energy_col, float energy_threshold,
                                float energy_mean_scale, size_t frames_context, float proportion_threshold, float *pool,
                                uint8_t *mask);
int ss_vad_energy_stream_flush_device(size_t n_active, const int32_t *d_slots, size_t pool_streams, float energy_threshold,
                                      float energy_mean_scale, size_t frames_context, float proportion_threshold, float *d_pool,
                                      uint8_t *d_mask, void *stream);
int ss_vad_energy_stream_flush(size_t n_active, const int32_t *slots, size_t pool_streams, float energy_threshold,
                               float energy_mean_scale, size_t frames_context, float proportion_threshold, float *pool,
                               uint8_t *mask);

/* ---- padded-batch collation of packed rows ----
 * The last stage of the packed chain: every model the rows are meant for takes a rectangular batch [B x T_max x C] (time-major
 * rows) or [B x C x T_max] (channels first: conv front ends, Whisper-style encoders) plus a lengths vector, almost always in f16 or
 * bf16.  One launch takes packed float rows and a device offset table and writes that batch: the dtype conversion, the optional
 * transpose, the pad filling and the per-clip lengths.  The reference crate has none: this comment is the specification.
 *   Clip b owns rows ro[b] .. ro[b+1] of vec [total_rows x cols]; T_b = ro[b+1] - ro[b]; kept_b = min(T_b, max_rows): a clip longer
 *   than max_rows is truncated to its first max_rows rows, which is legal (max_rows is the static shape a captured graph needs).
 *   out[b][t][c] (SS_PAD_BTC: [n_clips x max_rows x cols]) or out[b][c][t] (SS_PAD_BCT: [n_clips x cols x max_rows]) is
 *   conv(vec[ro[b] + t][c]) for t < kept_b and conv(pad_value) for kept_b <= t < max_rows; lengths[b] = kept_b.
 *   conv, by the element type of out:
 *     SS_PAD_F32   a bit copy: NaN payloads, -0.0 and denormals are unchanged, as in ss_splice_*.
 *     SS_PAD_F16   IEEE round-to-nearest-even, bit for bit numpy's astype(float16): |x| >= 65520 gives +-inf, results in the f16
 *                  denormal range are produced, not flushed.
 *     SS_PAD_BF16  round-to-nearest-even, (bits + 0x7FFF + ((bits >> 16) & 1)) >> 16 on the f32 bit pattern: f32 denormal inputs are
 *                  not flushed, +-inf stays.
 *     For both 16-bit types a NaN gives a NaN; its payload is not specified.
 *   Bad segments (device form): a segment that is reversed, starts below 0 or ends past total_rows is contained -- its whole block
 *   of out is conv(pad_value) and lengths[b] = -1, distinguishable from a valid clip without rows (0).  Nothing of vec outside
 *   [0, total_rows) x cols is read, whatever the table holds.  There is no error word: the stage has no handle.
 *   Every element of out and of lengths is written by every call (the caller needs no memset and the result never depends on what
 *   the buffers held), nothing is written outside them, and a clip's block depends on its own rows, max_rows and the scalars only
 *   -- not on its place in the block, its row offset or the workgroup split.
 *   One launch (ss_pad_packed_kernel<btc|bct,f32|f16|bf16>) whatever n_clips and the table hold, with a grid that depends on
 *   n_clips, max_rows and cols only; asynchronous on `stream`, no allocation, no read-back: graph-capturable and replayable over
 *   changed table contents.  The d_out_offsets of ss_select_rows_packed_device and the out_offsets of ss_splice_packed_offsets are
 *   valid tables as they stand, with total_rows as the bound; so are the row_offsets of a stream-pool call, whose entries then act
 *   as clips: max_rows = the largest chunk gives the [n_active x R_max x cols] tick batch of a streaming model.
 * Arguments: n_clips == 0 is SS_OK and writes nothing, also without a device.  pad_value may be any float, NaN and inf included.
 * SS_ERR_ARG, decided before the device is touched: null buffers; cols == 0; max_rows == 0; a layout or dtype outside its enum;
 * n_clips, total_rows, cols or max_rows >= 2^31; an output byte count that overflows size_t; out not aligned to its element size;
 * (device form) out or lengths overlapping vec.  The host form stages through device buffers; it checks the table first as the
 * other host forms do and names the first bad clip.  ss_pad_packed_out_bytes (host only, no device) returns n_clips * max_rows *
 * cols * (4 or 2) and SS_ERR_ARG where that overflows size_t. */
enum { SS_PAD_F32 = 0, SS_PAD_F16 = 1, SS_PAD_BF16 = 2 }; /* element type of out */
enum { SS_PAD_BTC = 0, SS_PAD_BCT = 1 };                   /* [n_clips x max_rows x cols] / [n_clips x cols x max_rows] */
int ss_pad_packed_out_bytes(size_t n_clips, size_t max_rows, size_t cols, int dtype, size_t *bytes);
int ss_pad_packed_device(const float *d_vec, size_t n_clips, const int64_t *d_row_offsets, size_t total_rows, size_t cols,
                         size_t max_rows, int layout, int dtype, float pad_value, void *d_out, int32_t *d_lengths, void *stream);
int ss_pad_packed(const float *vec, size_t n_clips, const int64_t *row_offsets, size_t total_rows, size_t cols, size_t max_rows,
                  int layout, int dtype, float pad_value, void *out, int32_t *lengths);

/* ---- SpecAugment: time / frequency masking of packed rows, seeded on the device ----
 * The augmentation every training recipe applies between CMVN and collation (WeNet spec_aug, ESPnet SpecAug, torchaudio
 * TimeMasking / FrequencyMasking): n_time spans of rows and n_freq spans of columns of every clip are overwritten with mask_value.
 * The spans are drawn on the device from a counter-based generator, so the stage reads nothing back, needs no host lengths and
 * draws fresh masks on every replay of a captured graph.  The reference crate has none: this comment is the specification.
 *   Clip b owns rows ro[b] .. ro[b+1] of vec [total_rows x cols]; T_b = ro[b+1] - ro[b].
 *   Scalars: n_time, n_freq (0 .. 16 each); max_time_width, max_freq_width; time_ratio (a float in [0, 1]; 1 = no cap by the clip's
 *   length); mask_value (any float, NaN and -0.0 included: it is written as its bit pattern); clip_base (the id of clip 0).
 *   rng: two uint64 words {seed, epoch}.
 *   Generator: Philox4x32-10 (Salmon et al., Random123; csrc/ss_philox.h), philox(counter[4], key[2]) -> four 32-bit words.
 *   Bounds: W_b = min(max_time_width, (uint32)floor((double)time_ratio * (double)T_b)) -- one f64 product, truncated;
 *           F = min(max_freq_width, cols).
 *   Draw of mask index k (k = time mask k for k < n_time; k = 0x10000 + j for frequency mask j):
 *     (u0, u1, -, -) = philox((low32(clip_base + b), k, low32(epoch), high32(epoch)), (low32(seed), high32(seed)))
 *     width = (u0 * (bound + 1)) >> 32 in 64-bit integers, so width is in [0, bound]             (bound = W_b or F)
 *     start = (u1 * (extent - width + 1)) >> 32, so start is in [0, extent - width]                (extent = T_b or cols)
 *     words 2 and 3 are reserved.
 *   Spans table: int32 [n_clips x (n_time + n_freq) x 2], (start, width) pairs, time masks first.  A segment that is reversed,
 *   starts below 0 or ends past total_rows has (-1, 0) in every one of its spans.
 *   out[r][c] = mask_value where row r - ro[b] lies in any time span of its clip or c lies in any frequency span of its clip, and
 *   a bit copy of vec[r][c] otherwise (NaN payloads, -0.0 and denormals unchanged); overlapping spans are a union.
 *   A clip's spans depend on (seed, epoch, clip_base + b, T_b, cols, the scalars) only -- not on its offset or its neighbours: the
 *   clips [B, C] at clip_base 1 get the spans they have as clips 1 and 2 of [A, B, C] at clip_base 0.
 *   Worked pin: seed 2026, epoch 0, clip_base 0, T_b = 200, max_time_width = 40, time_ratio 1, n_time = 2: clips 0, 1, 2 have
 *   (start, width) = (96, 17) (1, 29) | (56, 40) (105, 31) | (124, 28) (130, 13).
 * Calls:
 *   ss_specaug_spans               host only, no device: the spans table the plan launch writes, from the same code.
 *   ss_specaug_plan_packed_device  the plan launch alone (ss_specaug_plan_kernel, one lane per clip and mask); epoch is not touched.
 *   ss_mask_spans_packed[_device]  the apply launch alone (ss_specaug_apply_kernel<copy|inplace>) on any spans table -- the caller's
 *                                  own, or one plan applied to two blocks.  A span that is out of range (start < 0, width < 0 or start
 *                                  + width > its extent) is skipped whole.
 *   ss_specaug_packed[_device]     plan + apply, two launches, and the epoch bump: lane 0 of the apply launch stores epoch + 1, so
 *                                  the next call -- or the next replay of a captured graph -- draws other masks with no host
 *                                  involvement.  d_spans is caller-owned and always written; the host form updates rng[1].
 *   d_out == d_vec is the in-place call: nothing of vec is loaded and only the masked elements are stored.  Otherwise out must not
 *   overlap vec.  Rows of a bad segment and rows in no clip are left untouched (out of place: left unwritten); nothing outside [0,
 *   total_rows) x cols is read or written, whatever the table or the spans hold.  The grids depend on n_clips, n_time and n_freq
 *   only; the device forms are asynchronous on `stream`, allocate nothing and read nothing back.
 *   One rng block serves one stream of calls: concurrent calls that share a block race on epoch (give every stream its own block,
 *   with its own seed or a disjoint clip_base range).
 * Arguments: n_clips == 0 is SS_OK, also without a device.  SS_ERR_ARG, decided before the device is touched: null buffers (spans
 * may be null when n_time + n_freq == 0); cols == 0; n_time or n_freq > 16; time_ratio outside [0, 1] or NaN; n_clips, total_rows,
 * cols, max_time_width or max_freq_width >= 2^31; clip_base + n_clips > 2^32; vec, out or spans not 4-byte, rng not 8-byte aligned;
 * out partly overlapping vec (equal is in place); spans or rng overlapping vec, out or each other.  The host forms check the table
 * first as the other host forms do and name the first bad clip in ss_last_error_string(); they write rows 0 .. ro[n_clips) of out. */
int ss_specaug_spans(const uint64_t *rng, size_t clip_base, size_t n_clips, const int64_t *row_offsets, size_t total_rows, size_t cols,
                     size_t n_time, size_t max_time_width, float time_ratio, size_t n_freq, size_t max_freq_width, int32_t *spans);
int ss_specaug_plan_packed_device(const uint64_t *d_rng, size_t clip_base, size_t n_clips, const int64_t *d_row_offsets,
                                  size_t total_rows, size_t cols, size_t n_time, size_t max_time_width, float time_ratio,
                                  size_t n_freq, size_t max_freq_width, int32_t *d_spans, void *stream);
int ss_mask_spans_packed_device(const float *d_vec, size_t n_clips, const int64_t *d_row_offsets, size_t total_rows, size_t cols,
                                const int32_t *d_spans, size_t n_time, size_t n_freq, float mask_value, float *d_out, void *stream);
int ss_mask_spans_packed(const float *vec, size_t n_clips, const int64_t *row_offsets, size_t total_rows, size_t cols,
                         const int32_t *spans, size_t n_time, size_t n_freq, float mask_value, float *out);
int ss_specaug_packed_device(const float *d_vec, size_t n_clips, const int64_t *d_row_offsets, size_t total_rows, size_t cols,
                             uint64_t *d_rng, size_t clip_base, size_t n_time, size_t max_time_width, float time_ratio, size_t n_freq,
                             size_t max_freq_width, float mask_value, float *d_out, int32_t *d_spans, void *stream);
int ss_specaug_packed(const float *vec, size_t n_clips, const int64_t *row_offsets, size_t total_rows, size_t cols, uint64_t *rng,
                      size_t clip_base, size_t n_time, size_t max_time_width, float time_ratio, size_t n_freq, size_t max_freq_width,
                      float mask_value, float *out, int32_t *spans);

/* ---- additive noise at a drawn SNR and gain perturbation of packed clips, seeded on the device ----
 * The waveform augmentation of the training recipes (Kaldi wav-reverberate --additive-signals --snrs and sox vol, ESPnet
 * noise_apply_prob / noise_db_range, NeMo NoisePerturbation / GainPerturbation, lhotse mix, torchaudio.functional.add_noise), ahead of
 * the front end: with probability prob a clip gets a segment of a drawn noise clip added at a drawn SNR, and every clip a drawn gain.
 * The stage reads nothing back and draws fresh noise on every replay of a captured graph.  The reference crate has none: this comment
 * is the specification.
 *   Speech: x, packed samples; clip b owns samples so[b] .. so[b+1] (the sample_offsets of ss_mfcc_packed*, the out_offsets of
 *   ss_resample_packed*); L_b = so[b+1] - so[b] < 2^31.  Noise bank: nz, packed samples; noise clip c owns no[c] .. no[c+1] of its
 *   total_noise samples, N_c = no[c+1] - no[c] < 2^31; the bank is never written.  rng: two uint64 words {seed, epoch}, the block of
 *   ss_specaug_packed* with the same rules.  clip_base: the id of clip 0.  Scalars: prob in [0, 1]; snr_lo_db <= snr_hi_db and
 *   gain_lo_db <= gain_hi_db, finite (0, 0: no gain perturbation).
 *   Plan: one ss_noise_plan_row per clip (40 bytes, 8-byte aligned), caller-owned and always written.
 *   Draws (integers and f64 only: host and device agree exactly), with id = low32(clip_base + b), key = (low32(seed), high32(seed)):
 *     (u0, u1, u2, u3) = philox((id, 0x20000, low32(epoch), high32(epoch)), key);  (v0, -, -, -) = philox((id, 0x20001, ..), key)
 *     -- counter words apart from SpecAugment's mask indices, so that one seed may serve both stages.
 *     mixed = (uint64)u0 < (uint64)((double)prob * 4294967296.0) and n_noise > 0;  c = (u1 * n_noise) >> 32;
 *     a drawn noise clip that is empty, reversed or not inside [0, total_noise]: mixed = false;  start = (u2 * N_c) >> 32;
 *     snr_db = (float)((double)snr_lo_db + ((double)snr_hi_db - (double)snr_lo_db) * (u3 * 2^-32)) -- the product and the sum each
 *     rounded once in f64, the result once to f32; gain_db likewise from v0 and the gain range.
 *     Not mixed: noise_clip = -1, start = 0.  A speech segment that is reversed, starts below 0 or ends past total_samples:
 *     noise_clip = -2, start = 0, both gains and both energies 0, and its samples are untouched (out of place: left unwritten).
 *   Energies (f64): speech_energy = sum (double)x_i^2 over the clip; noise_energy = sum (double)n_i^2 over the segment the clip gets,
 *     n_i = nz[no[c] + (start + i) mod N_c], i = 0 .. L_b - 1 (the noise clip repeats); 0, and the bank unread, when not mixed.
 *     Each square is exact.  The order of the additions is a function of L_b alone: chunks of 2048 clip-relative samples; within a
 *     chunk 256 partials, partial l = ((0 + s_l) + s_{l+256}) + .. in ascending order over the samples the clip has; the tree
 *     p[l] += p[l + h] for h = 128, 64, .. 1; the energy = ((0 + chunk_0) + chunk_1) + ..  No atomics.
 *   Gains, formed in f64 and rounded once: G = 10^(gain_db / 20), exactly 1 when gain_db == 0;  speech_gain = (float)G;
 *     noise_gain = (float)((G * sqrt(speech_energy / noise_energy)) * 10^(-snr_db / 20)) when the clip is mixed and both energies
 *     are > 0, else 0.  The device's pow is not correctly rounded: these two words are specified to the f32 nearest the f64 value or
 *     its neighbour; every other word and every output bit is exact.
 *   Mix, bit for bit a function of the plan row: out[i] = fmaf(noise_gain, n_i, speech_gain * x_i), the product rounded on its own.
 *     A row with noise_gain == 0, or whose noise_clip or start is out of range for the bank (a caller's plan), is not mixed: out[i] =
 *     speech_gain * x_i and the bank is not read.  A row with noise_clip == -2 leaves its samples untouched.
 *   A clip's row and output depend on (seed, epoch, clip_base + b), its own samples, the bank and the scalars only -- not on its
 *   offset or its neighbours: the clips [B, C] at clip_base 1 get what they get as clips 1 and 2 of [A, B, C] at clip_base 0.
 *   Worked pin: seed 2026, epoch 0, clip_base 0, prob 0.5, SNR 10 .. 30 dB, gain -6 .. 6 dB, three speech clips of 16000 samples, a
 *   bank of noise clips of 8000, 1, 0, 50001 and 32000 samples: (noise_clip, start, snr_db, gain_db) of clips 0, 1, 2 =
 *   (3, 24801, 28.130686, -3.0997949) | (0, 4033, 14.968082, -1.3559483) | (-1, 0, 11.51598, 4.993896) -- the shortest decimals
 *   that round to the f32 words.
 * Calls:
 *   ss_noise_draws                   host only, no device: the four draw fields of every row from the same code; gains and energies 0.
 *   ss_noise_mix_work_bytes          the size of the caller-owned scratch of the device plan and mix forms (f64 partial sums: two words
 *                                    per chunk, total_samples / 2048 + n_clips chunk slots), 8-byte aligned.
 *   ss_noise_plan_packed[_i16]_device    draws, energies and gains into the plan: ss_noise_energy_kernel (workgroups (clip, share): a block
 *                                    of few long clips still fills the device) and ss_noise_fold_kernel.  epoch is not touched.
 *   ss_noise_apply_packed[_i16][_device] the mix alone (ss_noise_apply_kernel, a flat walk over the block) on any plan table: the
 *                                    caller's own for fixed gains, or one plan applied twice.
 *   ss_noise_mix_packed[_i16][_device]   plan + apply, three launches, and the epoch bump: lane 0 of the apply launch stores epoch + 1.
 *                                    The host forms update rng[1] and allocate their own scratch.
 *   The _i16 forms take x and the bank as 16-bit PCM with x_scale and noise_scale (powers of two, as in ss_mfcc_packed_i16): sample k
 *   is (float)pcm[k] * scale, out is float, and every plan word and output bit is that of the float call on the converted arrays;
 *   2-byte alignment is enough.  There is no mixed float / PCM form.
 *   d_out == d_x is the in-place call of the float form; any other overlap of out and x is an error, and the bank, the plan, rng and
 *   the scratch may overlap neither.  Samples in no clip are left untouched; nothing outside the blocks is read or written, whatever
 *   the tables or the plan hold.  The device forms expect speech segments that do not overlap one another (a sample in two segments
 *   is mixed as part of one of them, and the two clips' energies are unspecified).  The grids depend on n_clips and total_samples
 *   only; the device forms are asynchronous on `stream`, allocate nothing and read nothing back.  One rng block serves one stream of
 *   calls.
 * Arguments: n_clips == 0 is SS_OK, also without a device.  SS_ERR_ARG, decided before the device is touched: null buffers (the bank
 * and noise_offsets may be null when n_noise == 0); prob outside [0, 1] or NaN; a reversed or non-finite dB range; n_clips,
 * total_samples, n_noise or total_noise >= 2^31; clip_base + n_clips > 2^32; a scale that is not a power of two; samples, bank or
 * out not aligned to their element, tables, plan, rng or work not 8-byte aligned; work_bytes below ss_noise_mix_work_bytes; the
 * overlaps above.  The host forms check both tables first as the other host forms do (the speech table names the first bad clip)
 * and write samples 0 .. so[n_clips) of out. */
typedef struct ss_noise_plan_row {
    int32_t noise_clip; /* the bank's clip; -1: not mixed; -2: a bad speech segment */
    int32_t start;      /* first noise sample, 0 .. N_c - 1 */
    float snr_db;
    float gain_db;
    float speech_gain;
    float noise_gain;
    double speech_energy;
    double noise_energy;
} ss_noise_plan_row;
int ss_noise_draws(const uint64_t *rng, size_t clip_base, size_t n_clips, const int64_t *sample_offsets, size_t total_samples,
                   size_t n_noise, const int64_t *noise_offsets, size_t total_noise, float prob, float snr_lo_db, float snr_hi_db,
                   float gain_lo_db, float gain_hi_db, ss_noise_plan_row *plan);
int ss_noise_mix_work_bytes(size_t n_clips, size_t total_samples, size_t *bytes);
int ss_noise_plan_packed_device(const float *d_x, size_t n_clips, const int64_t *d_sample_offsets, size_t total_samples,
                                const float *d_bank, size_t n_noise, const int64_t *d_noise_offsets, size_t total_noise,
                                const uint64_t *d_rng, size_t clip_base, float prob, float snr_lo_db, float snr_hi_db, float gain_lo_db,
                                float gain_hi_db, ss_noise_plan_row *d_plan, void *d_work, size_t work_bytes, void *stream);
int ss_noise_plan_packed_i16_device(const int16_t *d_x, float x_scale, size_t n_clips, const int64_t *d_sample_offsets,
                                    size_t total_samples, const int16_t *d_bank, float noise_scale, size_t n_noise,
                                    const int64_t *d_noise_offsets, size_t total_noise, const uint64_t *d_rng, size_t clip_base,
                                    float prob, float snr_lo_db, float snr_hi_db, float gain_lo_db, float gain_hi_db,
                                    ss_noise_plan_row *d_plan, void *d_work, size_t work_bytes, void *stream);
int ss_noise_apply_packed_device(const float *d_x, size_t n_clips, const int64_t *d_sample_offsets, size_t total_samples,
                                 const float *d_bank, size_t n_noise, const int64_t *d_noise_offsets, size_t total_noise,
                                 const ss_noise_plan_row *d_plan, float *d_out, void *stream);
int ss_noise_apply_packed(const float *x, size_t n_clips, const int64_t *sample_offsets, size_t total_samples, const float *bank,
                          size_t n_noise, const int64_t *noise_offsets, size_t total_noise, const ss_noise_plan_row *plan, float *out);
int ss_noise_apply_packed_i16_device(const int16_t *d_x, float x_scale, size_t n_clips, const int64_t *d_sample_offsets,
                                     size_t total_samples, const int16_t *d_bank, float noise_scale, size_t n_noise,
                                     const int64_t *d_noise_offsets, size_t total_noise, const ss_noise_plan_row *d_plan, float *d_out,
                                     void *stream);
int ss_noise_apply_packed_i16(const int16_t *x, float x_scale, size_t n_clips, const int64_t *sample_offsets, size_t total_samples,
                              const int16_t *bank, float noise_scale, size_t n_noise, const int64_t *noise_offsets, size_t total_noise,
                              const ss_noise_plan_row *plan, float *out);
int ss_noise_mix_packed_device(const float *d_x, size_t n_clips, const int64_t *d_sample_offsets, size_t total_samples,
                               const float *d_bank, size_t n_noise, const int64_t *d_noise_offsets, size_t total_noise, uint64_t *d_rng,
                               size_t clip_base, float prob, float snr_lo_db, float snr_hi_db, float gain_lo_db, float gain_hi_db,
                               float *d_out, ss_noise_plan_row *d_plan, void *d_work, size_t work_bytes, void *stream);
int ss_noise_mix_packed(const float *x, size_t n_clips, const int64_t *sample_offsets, size_t total_samples, const float *bank,
                        size_t n_noise, const int64_t *noise_offsets, size_t total_noise, uint64_t *rng, size_t clip_base, float prob,
                        float snr_lo_db, float snr_hi_db, float gain_lo_db, float gain_hi_db, float *out, ss_noise_plan_row *plan);
int ss_noise_mix_packed_i16_device(const int16_t *d_x, float x_scale, size_t n_clips, const int64_t *d_sample_offsets,
                                   size_t total_samples, const int16_t *d_bank, float noise_scale, size_t n_noise,
                                   const int64_t *d_noise_offsets, size_t total_noise, uint64_t *d_rng, size_t clip_base, float prob,
                                   float snr_lo_db, float snr_hi_db, float gain_lo_db, float gain_hi_db, float *d_out,
                                   ss_noise_plan_row *d_plan, void *d_work, size_t work_bytes, void *stream);
int ss_noise_mix_packed_i16(const int16_t *x, float x_scale, size_t n_clips, const int64_t *sample_offsets, size_t total_samples,
                            const int16_t *bank, float noise_scale, size_t n_noise, const int64_t *noise_offsets, size_t total_noise,
                            uint64_t *rng, size_t clip_base, float prob, float snr_lo_db, float snr_hi_db, float gain_lo_db,
                            float gain_hi_db, float *out, ss_noise_plan_row *plan);

/* ---- reverberation of packed clips from a bank of room impulse responses, seeded on the device ----
 * The convolution step of the multi-condition recipes (Kaldi wav-reverberate --impulse-response, NeMo ImpulsePerturbation, lhotse
 * reverb_rir, ESPnet rir_scp / rir_apply_prob, torchaudio fftconvolve(x, rir)), ahead of ss_noise_mix_packed*: with probability prob a
 * clip is convolved with a drawn response of the bank.  The stage reads nothing back and draws afresh on every replay of a captured
 * graph.  The reference crate has none: this comment is the specification.
 *   Bank handle (ss_reverb_bank): ss_reverb_bank_create takes the responses packed on the host, response c = rir[ro[c] .. ro[c+1]) of
 *   total_rir floats, K_c = ro[c+1] - ro[c] in 1 .. 16384 finite taps; ro[0] == 0.  normalize: 0 = as given; 1 = unit energy,
 *   h / sqrt(sum h^2); 2 = peak magnitude 1, h / max |h| -- the squares, their sum in ascending order, the root and the quotient in
 *   f64, the quotient rounded once to f32; a response of zeros stays as it is.  peak_c = the first index of max |h|.  The handle's
 *   shift of response c is peak_c with align_peak = 1 (Kaldi's --shift-output=true: the direct path stays where it was) and 0 with
 *   align_peak = 0 (fftconvolve(x, h)[:L]).  At creation the host forms the partition spectra: partition p = taps [pB, pB + B) of the
 *   normalised response, B = 512, zero-padded to N = 1024 points, transformed in f64 (exp(-2 pi i nk / N)) and rounded once to f32.
 *   The handle works without a device; the first device call uploads the spectra to the device that is current then (a first call
 *   inside a graph capture therefore fails: make one call of the handle before capturing).
 *     ss_reverb_bank_info      n_rir, the block B, the longest K_c and the number of partition spectra.
 *     ss_reverb_bank_rir       n_taps = K_c and peak = peak_c of response c, and with taps != NULL (cap >= K_c floats) the normalised
 *                              f32 taps exactly as the spectra were made from them: references are built from these.
 *     ss_reverb_bank_spectrum  partition p of response c as N interleaved (re, im) pairs, bin 0 first.
 *   Speech: x, packed samples; clip b owns samples so[b] .. so[b+1] (the sample_offsets of ss_noise_mix_packed*); L_b < 2^31.  rng and
 *   clip_base: as in ss_noise_mix_packed*.
 *   Plan: one ss_reverb_plan_row {rir, shift} per clip (8 bytes, 8-byte aligned table), caller-owned and always written.
 *   Draws (integers and f64 only: host and device agree exactly), with id = low32(clip_base + b), key = (low32(seed), high32(seed)):
 *     (u0, u1, -, -) = philox((id, 0x30000, low32(epoch), high32(epoch)), key) -- a counter word apart from SpecAugment's mask indices
 *     (below 0x20000) and the noise stage's 0x20000 / 0x20001, so that one {seed, epoch} block may serve all three stages.
 *     reverberated = (uint64)u0 < (uint64)((double)prob * 4294967296.0) and n_rir > 0;  rir = (u1 * n_rir) >> 32, shift = the handle's
 *     shift of that response.  Not reverberated: rir = -1, shift = 0.  A speech segment that is reversed, starts below 0 or ends past
 *     total_samples: rir = -2, shift = 0.
 *   Output, a pure function of the clip's samples and its row: out[i] = sum_k h[k] * x[i + shift - k], i = 0 .. L_b - 1, k = 0 ..
 *     K - 1, samples outside the clip's own segment taken as +0.0: the same length as the clip, and a clip never reads its neighbour.
 *     Computed by partitioned overlap-save in f32 (ss_reverb_apply_kernel): per block pair of 2B clip-relative outputs one forward
 *     transform per partition whose window meets the clip, products with the partition spectra accumulated in ascending p, one
 *     inverse transform.  Specified to max |out - ref| <= 1e-4 * max |ref| per clip against the f64 direct sum over the taps
 *     ss_reverb_bank_rir returns; not bit-exact against it, also not for a delta response (h = [1], or a lone 1 at the peak with
 *     align_peak: x comes back within the same bound, a transform pair in between).  Bit-exact are: a clip against the same clip at
 *     any other place of any other block (the blocks are clip-relative), the PCM forms against the float forms, the host forms
 *     against the device forms, and one plan applied twice.
 *     A row with rir == -1, or whose rir is not in [0, n_rir) or whose shift is not in [0, K_rir) (a caller's plan), is not
 *     reverberated: its samples are copied bit for bit (NaN payloads, -0.0 and denormals kept).  A row with rir == -2 leaves its
 *     samples unwritten, and so are samples in no clip.
 *   A clip's row and output depend on (seed, epoch, clip_base + b), its own samples and the bank only: the clips [B, C] at clip_base 1
 *   get what they get as clips 1 and 2 of [A, B, C] at clip_base 0.
 *   Worked pin: seed 2026, epoch 0, clip_base 0, prob 0.5, a bank of five responses whose peaks lie at 0, 7, 100, 3 and 11 with
 *   align_peak = 1, three speech clips of 16000 samples: (rir, shift) of clips 0, 1, 2 =
 *   (2, 100) | (-1, 0) | (0, 0).
 * Calls:
 *   ss_reverb_draws                        host only, no device: every plan row from the same code.
 *   ss_reverb_plan_packed_device           the rows on the device (ss_reverb_plan_kernel).  epoch is not touched.
 *   ss_reverb_apply_packed[_i16][_device]  the convolution alone on any plan table: the caller's own, or one plan applied twice.
 *   ss_reverb_packed[_i16][_device]        plan + apply, two launches, and the epoch bump: lane 0 of the apply launch stores epoch + 1.
 *                                          The host forms update rng[1].
 *   The _i16 forms take x as 16-bit PCM with x_scale (a power of two, as in ss_mfcc_packed_i16): sample k is (float)pcm[k] * x_scale,
 *   out is float, and every output bit is that of the float call on the converted array; 2-byte alignment is enough.
 *   out may not overlap x (an in-place convolution is an error), and the plan and rng may overlap neither.  Nothing outside the
 *   blocks is read or written, whatever the table or the plan hold.  The device forms expect speech segments that do not overlap one
 *   another.  The grids depend on n_clips and total_samples only; the device forms are asynchronous on `stream`, allocate nothing
 *   (the handle's first device call apart) and read nothing back.  One rng block serves one stream of calls.
 *   Not served: Kaldi's --normalize-output power matching (a following ss_noise_mix_packed* measures the reverberated speech's energy
 *   itself and applies the gain), multi-channel responses, responses over 16384 taps, stream pools.
 * Arguments: n_clips == 0 is SS_OK, also without a device.  SS_ERR_ARG, decided before the device is touched: null buffers; prob
 * outside [0, 1] or NaN; n_clips or total_samples >= 2^31; clip_base + n_clips > 2^32; a scale that is not a power of two; samples or
 * out not aligned to their element, the table, plan or rng not 8-byte aligned; the overlaps above; at creation a response that is
 * empty, reversed, longer than 16384 taps, past total_rir or not finite (the message names it), normalize outside 0 .. 2, align_peak
 * outside 0 .. 1, n_rir >= 2^26.  The host forms check the table first as the other host forms do (the first bad clip is named),
 * write samples 0 .. so[n_clips) of out, and hand the caller's out to the device first, so that rows a caller's plan leaves
 * unwritten keep what they held. */
typedef struct ss_reverb_bank ss_reverb_bank; /* opaque: taps, partition spectra and, after the first device call, their device copy */
typedef struct ss_reverb_plan_row {
    int32_t rir;   /* the bank's response; -1: not reverberated; -2: a bad speech segment */
    int32_t shift; /* first tap index that lands on the output sample itself, 0 .. K - 1 */
} ss_reverb_plan_row;
int ss_reverb_bank_create(const float *rir, size_t n_rir, const int64_t *rir_offsets, size_t total_rir, int normalize, int align_peak,
                          ss_reverb_bank **bank);
void ss_reverb_bank_destroy(ss_reverb_bank *bank);
int ss_reverb_bank_info(const ss_reverb_bank *bank, size_t *n_rir, size_t *block, size_t *max_taps, size_t *n_partitions);
int ss_reverb_bank_rir(const ss_reverb_bank *bank, size_t c, float *taps, size_t cap, size_t *n_taps, size_t *peak);
int ss_reverb_bank_spectrum(const ss_reverb_bank *bank, size_t c, size_t p, float *out);
int ss_reverb_draws(const uint64_t *rng, size_t clip_base, size_t n_clips, const int64_t *sample_offsets, size_t total_samples,
                    const ss_reverb_bank *bank, float prob, ss_reverb_plan_row *plan);
int ss_reverb_plan_packed_device(size_t n_clips, const int64_t *d_sample_offsets, size_t total_samples, const ss_reverb_bank *bank,
                                 const uint64_t *d_rng, size_t clip_base, float prob, ss_reverb_plan_row *d_plan, void *stream);
int ss_reverb_apply_packed_device(const float *d_x, size_t n_clips, const int64_t *d_sample_offsets, size_t total_samples,
                                  const ss_reverb_bank *bank, const ss_reverb_plan_row *d_plan, float *d_out, void *stream);
int ss_reverb_apply_packed(const float *x, size_t n_clips, const int64_t *sample_offsets, size_t total_samples,
                           const ss_reverb_bank *bank, const ss_reverb_plan_row *plan, float *out);
int ss_reverb_apply_packed_i16_device(const int16_t *d_x, float x_scale, size_t n_clips, const int64_t *d_sample_offsets,
                                      size_t total_samples, const ss_reverb_bank *bank, const ss_reverb_plan_row *d_plan, float *d_out,
                                      void *stream);
int ss_reverb_apply_packed_i16(const int16_t *x, float x_scale, size_t n_clips, const int64_t *sample_offsets, size_t total_samples,
                               const ss_reverb_bank *bank, const ss_reverb_plan_row *plan, float *out);
int ss_reverb_packed_device(const float *d_x, size_t n_clips, const int64_t *d_sample_offsets, size_t total_samples,
                            const ss_reverb_bank *bank, uint64_t *d_rng, size_t clip_base, float prob, float *d_out,
                            ss_reverb_plan_row *d_plan, void *stream);
int ss_reverb_packed(const float *x, size_t n_clips, const int64_t *sample_offsets, size_t total_samples, const ss_reverb_bank *bank,
                     uint64_t *rng, size_t clip_base, float prob, float *out, ss_reverb_plan_row *plan);
int ss_reverb_packed_i16_device(const int16_t *d_x, float x_scale, size_t n_clips, const int64_t *d_sample_offsets, size_t total_samples,
                                const ss_reverb_bank *bank, uint64_t *d_rng, size_t clip_base, float prob, float *d_out,
                                ss_reverb_plan_row *d_plan, void *stream);
int ss_reverb_packed_i16(const int16_t *x, float x_scale, size_t n_clips, const int64_t *sample_offsets, size_t total_samples,
                         const ss_reverb_bank *bank, uint64_t *rng, size_t clip_base, float prob, float *out, ss_reverb_plan_row *plan);

/* ---- polyphase windowed-sinc resampling ahead of the feature calls ----
 * Every call above takes audio at the rate its ss_params was built for; these calls bring telephony (8 kHz), capture (48 kHz) and
 * corpus (44.1 kHz) audio to it on the device, on the packed layout and the stream pools of the feature calls, from floats or 16-bit
 * PCM.  The reference crate has no resampler: this comment is the specification.  The filter is torchaudio.functional.resample's
 * default, resampling_method = "sinc_interp_hann" (lowpass_filter_width = 6, rolloff = 0.99).
 *   g = gcd(orig_rate, new_rate), o = orig_rate / g, n = new_rate / g, lpw = lowpass_filter_width;
 *   base = min(o, n) * rolloff;  width = ceil(lpw * o / base);  for phase i in 0 .. n-1 and tap k in 0 .. 2*width+o-1, all in f64:
 *     t = (-i / n + (k - width) / o) * base
 *     h[i][k] = 0                                                                      where |t| >= lpw (an exact zero)
 *             = (t == 0 ? 1 : sin(pi t) / (pi t)) * cos(pi t / (2 lpw))^2 * (base / o)  otherwise, rounded once to f32
 *     out[j*n + i] = sum_k h[i][k] * x[j*o + k - width]   (x outside the clip = +0.0);   out_len(L) = ceil(n * L / o)
 *   rolloff crosses the ABI as a float and is read as the decimal the caller wrote: the double nearest to the float's
 *   seven-significant-digit decimal (0.99f means 0.99, torchaudio's double).
 *   Per phase the taps with |t| < lpw are one run first[i] .. first[i] + count[i] - 1; taps = max count.  The table is compact:
 *   [n x taps] floats, row i holding the run of phase i, zero-padded on the right.
 *   lookback = max_i(width - first[i]), lookahead = max_i(first[i] + count[i] - 1 - width): how far left and right of sample j*o the
 *   outputs of period j reach.  A period is o samples in and n outputs out.
 *   Arithmetic of one output (normative): acc = +0.0f; for the taps of the phase's run in ascending k (the padding excluded):
 *   acc = fmaf(h, x, acc); a sample outside the clip is +0.0f and its fma is executed.  Dense, packed, pool and flush outputs are
 *   therefore the same bits: a stream's zero history is the clip's zero padding.
 * Arguments of every call that takes the four filter parameters, decided before any device is touched: SS_ERR_ARG for a rate of 0,
 * equal rates, lpw outside 1 .. 64, rolloff outside (0, 1], o or n above 1024; SS_ERR_UNSUPPORTED for taps > 256 or a compact table
 * above 40960 bytes (n * taps * 4). */
typedef struct ss_resample_info {
    uint32_t o, n, width, taps, lookback, lookahead;
    uint32_t latency_periods; /* D of the pool calls below */
    uint32_t tile_outputs;    /* outputs per workgroup tile of the kernels (a whole number of periods); results do not depend on it */
} ss_resample_info;
typedef struct ss_resampler ss_resampler; /* opaque: the filter and, after the first device call, its device copy */

/* host only, no device */
int ss_resample_sizes(uint32_t orig_rate, uint32_t new_rate, uint32_t lowpass_filter_width, float rolloff, ss_resample_info *info);
/* h: [n x taps]; first, count (may be NULL): [n] */
int ss_resample_taps(uint32_t orig_rate, uint32_t new_rate, uint32_t lowpass_filter_width, float rolloff, float *h, int32_t *first,
                     int32_t *count);
/* out_len = ceil(n * n_samples / o) */
int ss_resample_len(uint32_t orig_rate, uint32_t new_rate, size_t n_samples, size_t *out_len);
/* sample offsets [n_clips + 1] (offsets[0] == 0, not decreasing, clips shorter than 2^31) -> out offsets [n_clips + 1]: what
 * ss_resample_packed* take as out_offsets, and the sample_offsets of a feature call on the resampled block */
int ss_resample_packed_offsets(uint32_t orig_rate, uint32_t new_rate, size_t n_clips, const int64_t *sample_offsets, int64_t *out_offsets);

/* The handle owns the table; creation needs no device.  The first device call uploads the table, once, to the device that is current
 * then (a later call under another current device is SS_ERR_ARG); after that warm call nothing is allocated or copied inside a
 * launch, so the *_device forms are graph-capturable.  A handle may be used from several threads / streams concurrently. */
int ss_resampler_create(uint32_t orig_rate, uint32_t new_rate, uint32_t lowpass_filter_width, float rolloff, ss_resampler **out);
void ss_resampler_destroy(ss_resampler *rs);
int ss_resampler_info(const ss_resampler *rs, ss_resample_info *info);

/* Dense batch: x [batch x ld] (n_samples <= ld used per row) -> out [batch x ld_out], row b = the resampled row b, out_len(n_samples)
 * <= ld_out samples; the rest of an out row is left unwritten.  One launch (ss_resample_kernel<dense,f32>).  batch == 0 is SS_OK
 * without a device.  SS_ERR_ARG: null buffers, batch or n_samples or out_len >= 2^31, ld < n_samples, ld_out < out_len, out
 * overlapping x.  The last row ends with its samples, not a whole stride behind its start: x is (batch - 1) * ld + n_samples
 * floats, out (batch - 1) * ld_out + out_len, and those two ranges are what must not overlap.  The _i16 forms take int16 samples and a scale behind the sample-layout arguments: sample = (float)pcm * scale,
 * converted on load (no conversion launch; 2-byte alignment is enough, an odd address is SS_ERR_ARG), scale a power of two in
 * [2^-64, 2^64] else SS_ERR_ARG; every output is bit for bit that of the float call on x_f[k] = (float)pcm[k] * scale. */
int ss_resample_device(const ss_resampler *rs, const float *d_x, size_t batch, size_t n_samples, size_t ld, float *d_out, size_t ld_out,
                       void *stream);
int ss_resample(const ss_resampler *rs, const float *x, size_t batch, size_t n_samples, size_t ld, float *out, size_t ld_out);
int ss_resample_i16_device(const ss_resampler *rs, const int16_t *d_x, size_t batch, size_t n_samples, size_t ld, float scale, float *d_out,
                           size_t ld_out, void *stream);
int ss_resample_i16(const ss_resampler *rs, const int16_t *x, size_t batch, size_t n_samples, size_t ld, float scale, float *out,
                    size_t ld_out);

/* Packed clips: clip b owns x[so[b] .. so[b+1]) of x [total_in] and out[oo[b] .. oo[b+1]) of out [total_out].  Contract and containment
 * are those of ss_add_deltas_packed*: the tables are device arrays that only the kernel reads; one launch (ss_resample_kernel<packed,
 * f32>) whatever the clip count; a clip is skipped unless 0 <= so[b] <= so[b+1] <= total_in, 0 <= oo[b], oo[b+1] <= total_out and
 * oo[b+1] - oo[b] == out_len(so[b+1] - so[b]) (and the clip is shorter than 2^31 samples in and out); nothing outside the two blocks is
 * touched; outputs in no valid clip are left unwritten; a clip's bits depend on its own samples and the handle only -- not on its
 * place, not on its neighbours' contents: taps past a clip's end read zeros, never the next clip.  Empty clips are legal.  n_clips
 * == 0 is SS_OK without a device.  SS_ERR_ARG: null buffers, n_clips >= 2^31, out overlapping x, the PCM scale rule.  The host forms
 * (total_in = so[n_clips], total_out = oo[n_clips]) check the tables first -- offsets[0] != 0, a decreasing pair, an output span that
 * is not out_len long -- and name the first bad clip in ss_last_error_string().
 * out_offsets (ss_resample_packed_offsets) is by construction the sample_offsets of a following ss_mfcc_packed_device call on out:
 * INTEGRATION.md shows the chain. */
int ss_resample_packed_device(const ss_resampler *rs, const float *d_x, size_t n_clips, const int64_t *d_sample_offsets,
                              const int64_t *d_out_offsets, size_t total_in, size_t total_out, float *d_out, void *stream);
int ss_resample_packed(const ss_resampler *rs, const float *x, size_t n_clips, const int64_t *sample_offsets, const int64_t *out_offsets,
                       float *out);
int ss_resample_packed_i16_device(const ss_resampler *rs, const int16_t *d_x, size_t n_clips, const int64_t *d_sample_offsets, float scale,
                                  const int64_t *d_out_offsets, size_t total_in, size_t total_out, float *d_out, void *stream);
int ss_resample_packed_i16(const ss_resampler *rs, const int16_t *x, size_t n_clips, const int64_t *sample_offsets, float scale,
                           const int64_t *out_offsets, float *out);

/* Pool of stream states, fixed latency of D = ceil((lookahead + 1) / o) periods (ss_resample_stream_*): a stream is fed whole periods,
 * as the feature pools take whole hops (441 samples = 10 ms at 44.1 kHz -> 16 kHz, 3 samples at 48 kHz -> 16 kHz), and gets its
 * outputs D * n outputs late.  Pool: a caller-owned block [pool_streams x len] of floats, len = ss_resample_stream_state_len = D * o +
 * lookback + 1: the stream's last D * o + lookback samples as floats, oldest first, right-aligned, zeros in front, then the count word
 * min(periods seen, D) as a float.  All zeros = fresh stream.  A count word that is not an integer in [0, D] (NaN included) is read
 * as 0.
 *   Entry i owns x[so[i] .. so[i+1]) of x [total_in], P_i = (so[i+1] - so[i]) / o >= 0 periods, pool row slots[i], and exactly P_i * n
 *   outputs: out[so[i] / o * n .. so[i+1] / o * n) of out [total_in / o * n].  Output k of the entry is stream output time tau = seen_out
 *   + k - D * n (seen_out: outputs of the stream before this call).  tau < 0: +0.0, a forced warm-up output (not the filter's
 *   pre-ringing).  tau >= 0: the output defined above with zeros to the left of the stream's first sample.  P_i == 0 writes nothing
 *   and leaves the pool row bit for bit.
 *   Flush (ss_resample_stream_flush*): entry i gets exactly D * n outputs, out[i * D * n .. (i + 1) * D * n): the stream's last outputs,
 *   with zeros to the right of its last sample (forced +0.0 where tau < 0).  Afterwards the pool row is all zeros.
 *   Invariant: however a stream is cut into calls (empty entries included, float and PCM calls mixed), the outputs of all its calls
 *   plus the flush, the first D * n dropped, are bit for bit ss_resample_packed* on the whole clip of P * o samples (out_len(P * o)
 *   = P * n).
 *   One launch each (ss_resample_stream_kernel), one workgroup per entry, asynchronous on `stream`, no scratch, graph-capturable as a
 *   single kernel node whose grid depends on n_active only.  Containment as ss_add_deltas_stream_packed*: an entry is skipped -- no
 *   output written, its pool row untouched -- unless 0 <= so[i] <= so[i+1] <= total_in, so[i] and so[i+1] are multiples of o, the
 *   entry brings fewer than 2^20 periods and 0 <= slots[i] < pool_streams (flush: the slot rule); whatever the tables and count words
 *   hold, nothing outside the blocks is read or written.  Duplicate slots in a device-form call are a caller error that is NOT
 *   detected (results of those entries unspecified, everything stays inside the pool); the host forms reject them.
 *   The float output of this pool is the x of ss_mfcc_stream_packed_device; the caller still buffers it to whole hops, since a period
 *   of n outputs and a hop are different granularities.
 * Arguments: n_active == 0 is SS_OK with nothing launched, also without a device.  SS_ERR_ARG, decided before the device is touched,
 * pool and out untouched: null buffers; n_active or pool_streams >= 2^31, total_in >= 2^40; pool_streams == 0; out overlapping x; the
 * pool overlapping x or out; the PCM scale rule.  The host forms (total_in = so[n_active]) also check the tables first -- so[0] != 0,
 * a decreasing pair, an entry that is not whole periods, a slot outside the pool, a slot named twice; ss_last_error_string() names
 * the first bad entry -- and move only what the call touches; the caller's pool is written only after everything before it
 * succeeded. */
int ss_resample_stream_state_len(const ss_resampler *rs, size_t *state_len);
int ss_resample_stream_packed_device(const ss_resampler *rs, const float *d_x, size_t n_active, const int64_t *d_sample_offsets,
                                     size_t total_in, const int32_t *d_slots, size_t pool_streams, float *d_pool, float *d_out,
                                     void *stream);
int ss_resample_stream_packed(const ss_resampler *rs, const float *x, size_t n_active, const int64_t *sample_offsets, const int32_t *slots,
                              size_t pool_streams, float *pool, float *out);
int ss_resample_stream_packed_i16_device(const ss_resampler *rs, const int16_t *d_x, size_t n_active, const int64_t *d_sample_offsets,
                                         size_t total_in, const int32_t *d_slots, size_t pool_streams, float scale, float *d_pool,
                                         float *d_out, void *stream);
int ss_resample_stream_packed_i16(const ss_resampler *rs, const int16_t *x, size_t n_active, const int64_t *sample_offsets,
                                  const int32_t *slots, size_t pool_streams, float scale, float *pool, float *out);
int ss_resample_stream_flush_device(const ss_resampler *rs, size_t n_active, const int32_t *d_slots, size_t pool_streams, float *d_pool,
                                    float *d_out, void *stream);
int ss_resample_stream_flush(const ss_resampler *rs, size_t n_active, const int32_t *slots, size_t pool_streams, float *pool, float *out);

/* ---- Kaldi-compatible fbank / MFCC front end (compute-fbank-feats / compute-mfcc-feats as torchaudio.compliance.kaldi.fbank / .mfcc
 * restate them) for frames that pad to 512 points ----
 * The stage that ss_resample*, ss_cmvn_stream_packed* and ss_add_deltas* wrap in a Kaldi-shaped pipeline.  The reference crate has no
 * such path and no combination of ss_params switches gives it, so it has its own parameter structure, its own handle and this comment
 * as its specification.  Arithmetic is f32 on the device unless stated; tables are formed in f64 on the host and rounded once.
 *   Sizes: flen = (int)(sample_rate * 0.001 * frame_length_ms), shift = (int)(sample_rate * 0.001 * frame_shift_ms), in double;
 *   N = the smallest power of two >= flen.  This version serves N == 512 only (256 < flen <= 512: 16 kHz at 20 / 25 / 32 ms, 11.025 kHz
 *   at 25 ms); every other N is SS_ERR_UNSUPPORTED and is the next step.  shift >= 1, of either parity, may exceed flen.
 *   Frames (snip_edges = true): T = 0 if L < flen, else 1 + (L - flen) / shift; frame t is x[t * shift : t * shift + flen].
 *   Per frame, in this order:
 *    1. s[i] = x[i] * input_scale (skipped when input_scale == 1).
 *    2. remove_dc_offset: m = (sum s[i]) / flen -- a true division -- and s[i] -= m.
 *    3. raw energy Er = sum s[i]^2 (used when raw_energy).
 *    4. pre-emphasis with c = preemph_coef, when c != 0: y[i] = s[i] - c * s[i-1] for i >= 1, y[0] = s[0] - c * s[0]: the predecessor
 *       is the frame's own sample, never the clip's.
 *    5. window: y[i] *= w[i]; with a = 2 pi i / (flen - 1): povey (0.5 - 0.5 cos a)^0.85, hanning 0.5 - 0.5 cos a, hamming
 *       0.54 - 0.46 cos a, rectangular 1, blackman b - 0.5 cos a + (0.5 - b) cos 2a with b = blackman_coeff.  Without raw_energy the
 *       energy is sum y[i]^2 taken here.
 *    6. zero-pad to N, real FFT, P[k] = |X[k]|^2 (use_power) or |X[k]| for k = 0 .. N/2 - 1: no 1/N, the Nyquist bin is not used.
 *    7. mel bank: mel(f) = 1127 ln(1 + f / 700); high_freq <= 0 means sample_rate / 2 + high_freq; delta = (mel(high) - mel(low)) /
 *       (num_mel_bins + 1); filter b has left, centre, right at mel(low) + b delta, + (b+1) delta, + (b+2) delta; bin k at mu =
 *       mel(k sample_rate / N) has a weight only if left < mu < right (strict): (mu - left) / (centre - left) if mu <= centre, else
 *       (right - mu) / (right - centre).  No normalisation, no VTLN.  e[b] = sum_k weight[b][k] P[k].
 *    8. fbank[b] = ln(max(e[b], eps)), eps = 1.1920929e-7: a floor (not the reference's == 0 patch); an empty filter gives ln eps.
 *    9. log energy = ln(max(E, eps)), and the maximum of that and ln(energy_floor) if energy_floor > 0.
 *   10. MFCC: c[k] = lift[k] sum_b D[k][b] fbank[b], k < num_ceps; D[0][b] = sqrt(1/M), D[k][b] = sqrt(2/M) cos(pi/M (b + 0.5) k);
 *       lift[k] = 1 + 0.5 Q sin(pi k / Q), Q = cepstral_lifter (Q == 0: no lifter), folded into the host table; use_energy: c[0] = the
 *       log energy.
 * Stream pools, fed floats or 16-bit PCM: the ss_kstream_* section below.  The one-shot calls fed 16-bit PCM: ss_kpcm_* below.
 * Not in this version: snip_edges = false, non-zero dither, VTLN, htk_compat, subtract_mean (ss_cmvn_packed does that), N != 512. */
enum {
    SS_KALDI_WINDOW_POVEY = 0,
    SS_KALDI_WINDOW_HANNING = 1,
    SS_KALDI_WINDOW_HAMMING = 2,
    SS_KALDI_WINDOW_RECTANGULAR = 3,
    SS_KALDI_WINDOW_BLACKMAN = 4
};
/* every field is 4 bytes wide, no padding.  ss_kaldi_params_default fills TORCHAUDIO's defaults (in the comments below); they differ
 * from the Kaldi binaries' in dither = 0 (Kaldi: 1), energy_floor = 1 (Kaldi: 0) and use_energy = 0 (compute-mfcc-feats: true). */
typedef struct ss_kaldi_params {
    uint32_t struct_size;     /* sizeof(ss_kaldi_params) */
    uint32_t sample_rate;
    float frame_length_ms;    /* 25 */
    float frame_shift_ms;     /* 10 */
    uint32_t num_mel_bins;    /* 23 */
    uint32_t num_ceps;        /* 13; the mfcc calls only, <= num_mel_bins */
    float low_freq;           /* 20 */
    float high_freq;          /* 0: <= 0 is an offset from sample_rate / 2 */
    float preemph_coef;       /* 0.97 */
    float cepstral_lifter;    /* 22 */
    int32_t window_type;      /* SS_KALDI_WINDOW_POVEY */
    float blackman_coeff;     /* 0.42 */
    int32_t remove_dc_offset; /* 1 */
    int32_t use_power;        /* 1 */
    int32_t use_energy;       /* 0; the mfcc calls: c[0] = the log energy */
    int32_t raw_energy;       /* 1 */
    float energy_floor;       /* 1.0 */
    float input_scale;        /* 1.0 */
    float dither;             /* 0.0: the only value served */
} ss_kaldi_params;
typedef struct ss_kaldi_config ss_kaldi_config; /* opaque: the parameters, the device tables and a device error word */

/* host only, no device.  Validation: SS_ERR_BAD_CONFIG for num_mel_bins < 3, low_freq < 0, a resolved high_freq <= low_freq or above
 * sample_rate / 2, flen < 2, shift < 1, num_ceps > num_mel_bins, input_scale not finite or <= 0, energy_floor < 0, a window_type outside
 * the enum; SS_ERR_UNSUPPORTED for a padded size other than 512, num_mel_bins > 80, num_ceps > 32, dither != 0. */
int ss_kaldi_params_default(ss_kaldi_params *p, uint32_t sample_rate);
int ss_kaldi_params_validate(const ss_kaldi_params *p);
int ss_kaldi_sizes(const ss_kaldi_params *p, size_t *frame_len, size_t *frame_shift, size_t *padded);
/* T == 0 is SS_ERR_SHORT_SIGNAL, as for ss_num_frames */
int ss_kaldi_num_frames(const ss_kaldi_params *p, size_t n_samples, size_t *n_frames);
/* the rules of ss_packed_frame_offsets */
int ss_kaldi_packed_frame_offsets(const ss_kaldi_params *p, size_t n_clips, const int64_t *sample_offsets, int64_t *frame_offsets);
/* w: [frame_len];  bank: [num_mel_bins x 256] dense (bins 0 .. 255);  dct: [num_ceps x num_mel_bins], the lifter folded in */
int ss_kaldi_window(const ss_kaldi_params *p, float *w);
int ss_kaldi_mel_bank(const ss_kaldi_params *p, float *bank);
int ss_kaldi_dct(const ss_kaldi_params *p, float *dct);

/* The handle: validated parameters, the kernel's tables uploaded at creation (to the current device: SS_ERR_HIP without one, after the
 * parameter rules) and a pinned device error word, as ss_config owns one.  Immutable afterwards: usable from several streams and
 * threads at once.  ss_kaldi_config_device_status has ss_config_device_status's contract: SS_ERR_DEVICE once if a launch on the handle
 * reported a bad packed clip since the last look, then SS_OK. */
int ss_kaldi_config_create(const ss_kaldi_params *p, ss_kaldi_config **out);
void ss_kaldi_config_destroy(ss_kaldi_config *cfg);
int ss_kaldi_config_params(const ss_kaldi_config *cfg, ss_kaldi_params *out);
int ss_kaldi_config_device_status(const ss_kaldi_config *cfg);

/* Equal-length clips: x [batch x ld] (n_samples <= ld used per row) -> out [batch x T x num_mel_bins] (fbank) or [batch x T x num_ceps]
 * (mfcc; num_ceps >= 1), T = ss_kaldi_num_frames(n_samples).  log_energy ([batch x T], may be NULL) is written whenever the pointer
 * is non-null, whatever use_energy says.  One launch of ss_kaldi_c256<NE,...> (ss_last_kernel_name(): NE = 10 / 13 / 16 live input
 * pairs for flen <= 320 / 416 / 512, then "pow2" with use_power, "mfcc" or "fbank").  The _device forms are asynchronous on `stream`
 * and graph-capturable; the host forms stage through device buffers and return when the results are in place.  Any ld, any base
 * alignment of 4 bytes and either parity of shift are served.  batch == 0 is SS_OK; SS_ERR_SHORT_SIGNAL for n_samples < flen;
 * SS_ERR_ARG for null buffers, ld < n_samples, n_samples >= 2^31, batch * T >= 2^32 - 8. */
int ss_kaldi_fbank_device(const ss_kaldi_config *cfg, const float *d_x, size_t batch, size_t n_samples, size_t ld, float *d_out,
                          float *d_log_energy, void *stream);
int ss_kaldi_fbank(const ss_kaldi_config *cfg, const float *x, size_t batch, size_t n_samples, size_t ld, float *out, float *log_energy);
int ss_kaldi_mfcc_device(const ss_kaldi_config *cfg, const float *d_x, size_t batch, size_t n_samples, size_t ld, float *d_out,
                         void *stream);
int ss_kaldi_mfcc(const ss_kaldi_config *cfg, const float *x, size_t batch, size_t n_samples, size_t ld, float *out);

/* Packed clips: the contract of ss_mfcc_packed*.  Clip b is x[so[b] : so[b+1]], its T_b frames are rows fo[b] .. fo[b+1] of the output
 * (fo from ss_kaldi_packed_frame_offsets, or computed by the caller on the device); one launch (ss_kaldi_c256<...,v>) whatever the
 * clip count; n_clips == 0 is SS_OK.  The _device forms' tables are DEVICE arrays of n_clips + 1 entries that only the kernel reads:
 * it recomputes every T_b from so, and a clip whose rows are not those T_b frames, or end past total_frames, is skipped -- its rows are
 * left untouched, nothing is written outside d_out / d_log_energy -- and the handle's error word is raised (SS_ERR_DEVICE through
 * ss_kaldi_config_device_status or the next call on the handle).  A clip's rows are bit for bit those of the equal-length call on that
 * clip alone, whatever the parity of its offset.  The out_offsets of ss_resample_packed_offsets are valid sample_offsets as they
 * stand: INTEGRATION.md shows the chain.  The host forms take sample_offsets alone, check them (ss_kaldi_packed_frame_offsets) and
 * write out [so-implied rows x cols]. */
int ss_kaldi_fbank_packed_device(const ss_kaldi_config *cfg, const float *d_x, size_t n_clips, const int64_t *d_sample_offsets,
                                 const int64_t *d_frame_offsets, size_t total_frames, float *d_out, float *d_log_energy, void *stream);
int ss_kaldi_fbank_packed(const ss_kaldi_config *cfg, const float *x, size_t n_clips, const int64_t *sample_offsets, float *out,
                          float *log_energy);
int ss_kaldi_mfcc_packed_device(const ss_kaldi_config *cfg, const float *d_x, size_t n_clips, const int64_t *d_sample_offsets,
                                const int64_t *d_frame_offsets, size_t total_frames, float *d_out, void *stream);
int ss_kaldi_mfcc_packed(const ss_kaldi_config *cfg, const float *x, size_t n_clips, const int64_t *sample_offsets, float *out);

/* ---- ss_kpcm_*: the eight one-shot calls above, fed signed 16-bit PCM ------------------------------------------------------
 * (The prefix is ss_kpcm_, not ss_kaldi_: the set of ss_kaldi_* names is closed, as it was for ss_kstream_*.)  Sample k of the call is
 * (float)x[k] * scale, scale a power of two in [2^-64, 2^64] (else SS_ERR_ARG, checked first among the data checks); the product is
 * exact.  scale = 1.0 is Kaldi's own sample convention (integer-valued floats), scale = 2^-15 torchaudio's; input_scale still applies
 * afterwards.  `scale` stands behind ld (equal-length clips) or behind the sample offsets (packed clips), as in ss_mfcc_batch_i16* /
 * ss_mfcc_packed_i16*.  Every output bit -- the rows, the log energy, the handle's error status -- is that of the float call on the
 * converted samples with the same handle; every other argument rule and return code is the float call's.  ld, n_samples and the
 * offsets stay in samples; x needs 2-byte alignment only, device and host form alike (any ld, any clip offset, either parity of
 * shift).  One launch of the kernel's PCM build: ss_kaldi_c256<NE,...,i> (equal-length clips) or <NE,...,vi> (packed), which fetches
 * a sample pair as one dword and converts it in registers -- no float copy of the samples exists anywhere; the host forms cross the
 * link as int16.  Graph-capturable and contained exactly as the float calls. */
int ss_kpcm_fbank_device(const ss_kaldi_config *cfg, const int16_t *d_x, size_t batch, size_t n_samples, size_t ld, float scale,
                         float *d_out, float *d_log_energy, void *stream);
int ss_kpcm_fbank(const ss_kaldi_config *cfg, const int16_t *x, size_t batch, size_t n_samples, size_t ld, float scale, float *out,
                  float *log_energy);
int ss_kpcm_mfcc_device(const ss_kaldi_config *cfg, const int16_t *d_x, size_t batch, size_t n_samples, size_t ld, float scale,
                        float *d_out, void *stream);
int ss_kpcm_mfcc(const ss_kaldi_config *cfg, const int16_t *x, size_t batch, size_t n_samples, size_t ld, float scale, float *out);
int ss_kpcm_fbank_packed_device(const ss_kaldi_config *cfg, const int16_t *d_x, size_t n_clips, const int64_t *d_sample_offsets, float scale,
                                const int64_t *d_frame_offsets, size_t total_frames, float *d_out, float *d_log_energy, void *stream);
int ss_kpcm_fbank_packed(const ss_kaldi_config *cfg, const int16_t *x, size_t n_clips, const int64_t *sample_offsets, float scale,
                         float *out, float *log_energy);
int ss_kpcm_mfcc_packed_device(const ss_kaldi_config *cfg, const int16_t *d_x, size_t n_clips, const int64_t *d_sample_offsets, float scale,
                               const int64_t *d_frame_offsets, size_t total_frames, float *d_out, void *stream);
int ss_kpcm_mfcc_packed(const ss_kaldi_config *cfg, const int16_t *x, size_t n_clips, const int64_t *sample_offsets, float scale,
                        float *out);

/* ---- ss_kstream_*: the Kaldi front end over a pool of stream states (live audio) -----------------------------------
 * The online form of ss_kaldi_fbank / ss_kaldi_mfcc, on the tables of the other stream pools (ss_resample_stream_packed*,
 * ss_cmvn_stream_packed*, ss_add_deltas_stream_packed*): one set of sample_offsets / row_offsets / slots serves the whole chain
 * (INTEGRATION.md).  The handle is an ss_kaldi_config; the arithmetic is the ss_kaldi_* specification above, on the same kernel body.
 * Sizes: flen and shift from ss_kaldi_sizes; D = ceil(flen / shift) - 1 is the delay in rows (0 where shift >= flen) and S = D * shift
 *   the carried samples per stream (ss_kstream_state_len; 16 kHz, 25 / 10 ms: D = 2, S = 320).  S is a whole number of hops, not
 *   flen - shift: only then do a stream's rows land on Kaldi's own frame grid.
 * Pool: a caller-owned [pool_streams x S] block of floats.  An all-zero row is a fresh stream; zeroing a row resets it.  S == 0 allows
 *   a NULL pool.
 * Entries (the rules of ss_mfcc_stream_packed*): a call serves n_active entries.  Entry i's chunk is x[so[i] : so[i+1]], R_i = n_i /
 *   shift whole hops (R_i = 0 is legal); its state is pool row slots[i]; its rows are rows ro[i] .. ro[i+1] of the packed output
 *   (ss_kstream_row_offsets); total_rows >= ro[n_active], rows past ro[n_active] are left alone.  Row t of an entry is the Kaldi frame
 *   of length flen that starts at chunk sample t * shift - S, a sample at position p < 0 being pool[slot * S + S + p].  Afterwards the
 *   pool row is the last S samples of (old row ++ chunk).
 * Equivalence: all of a stream's rows over all calls, however the stream was cut into calls, are bit for bit the rows (and the log
 *   energy) of ss_kaldi_fbank_device / ss_kaldi_mfcc_device on zeros(S) ++ stream, whatever else shares the call and whatever the
 *   entry's place or slot.  Every per-frame stage of the specification (DC removal, pre-emphasis from the frame's own first sample,
 *   window) is frame-local, and a clip of K hops has exactly K - D offline frames: with the first D rows after a reset dropped, the
 *   rows are ss_kaldi_fbank / ss_kaldi_mfcc of the stream itself.  THE FIRST D ROWS AFTER A RESET ARE WARM-UP ROWS over the zero
 *   prefix.  A caller who chains CMVN behind the call primes a new stream: its first D hops go through a call of their own whose
 *   rows are discarded, and in the chained call that stream is an R_i = 0 entry.
 * Containment: the skip rules are the frame pool's.  A bad entry (not whole hops, ro inconsistent, ro[i+1] > total_rows, slot outside
 *   the pool) is skipped by both launches -- its rows and its pool row stay untouched -- and raises the handle's error word:
 *   SS_ERR_DEVICE once, through ss_kaldi_config_device_status or the next call on the handle.  Nothing is read outside the entries'
 *   chunk ranges and the named pool rows; nothing is written outside rows [0, total_rows) and the named pool rows.
 * Arguments: n_active == 0 is SS_OK with no launch.  SS_ERR_ARG, with nothing touched, for null buffers, sizes >= 2^31, a pool range
 *   that overlaps an output, and a handle with num_ceps == 0 on the MFCC calls.  The host forms check the tables first and name the
 *   first bad entry (ss_kstream_row_offsets' rules: so[0] == 0, no decreasing pair, whole hops), reject duplicate slots, and write
 *   the caller's pool only after everything else succeeded.
 * shift of either parity is served: S, so[i] and a row's first sample may be odd.
 * _i16 forms: sample = (float)pcm * scale, scale a power of two in [2^-64, 2^64] (else SS_ERR_ARG); input_scale still applies
 *   afterwards.  The results are bit for bit the float call on the converted samples; the pool stays float, so a stream may alternate
 *   between PCM and float chunks.  The device forms need 2-byte alignment of d_x only.
 * The device forms are a linear chain of two launches on `stream` (one where S == 0) -- ss_kaldi_c256<NE,[pow2,]fbank|mfcc,sp> (,spi>
 *   for PCM) and the frame pool's state advance -- whose grids depend on n_active and total_rows only: capturable, and replayable over
 *   changed table contents.  d_log_energy ([total_rows], may be NULL) as in ss_kaldi_fbank_device.
 * Not served: snip_edges = false, dither, VTLN, padded sizes other than 512 (N != 512), and a dense
 *   (non-ragged) Kaldi stream call. */
int ss_kstream_state_len(const ss_kaldi_params *p, size_t *state_len, size_t *delay_rows); /* host only */
int ss_kstream_row_offsets(const ss_kaldi_params *p, size_t n_active, const int64_t *sample_offsets, int64_t *row_offsets); /* host only */
int ss_kstream_fbank_packed_device(const ss_kaldi_config *cfg, const float *d_x, size_t n_active, const int64_t *d_sample_offsets,
                                   const int64_t *d_row_offsets, size_t total_rows, const int32_t *d_slots, size_t pool_streams, float *d_pool,
                                   float *d_out, float *d_log_energy, void *stream);
int ss_kstream_mfcc_packed_device(const ss_kaldi_config *cfg, const float *d_x, size_t n_active, const int64_t *d_sample_offsets,
                                  const int64_t *d_row_offsets, size_t total_rows, const int32_t *d_slots, size_t pool_streams, float *d_pool,
                                  float *d_out, void *stream);
int ss_kstream_fbank_packed_i16_device(const ss_kaldi_config *cfg, const int16_t *d_x, size_t n_active, const int64_t *d_sample_offsets,
                                       const int64_t *d_row_offsets, size_t total_rows, const int32_t *d_slots, size_t pool_streams, float scale,
                                       float *d_pool, float *d_out, float *d_log_energy, void *stream);
int ss_kstream_mfcc_packed_i16_device(const ss_kaldi_config *cfg, const int16_t *d_x, size_t n_active, const int64_t *d_sample_offsets,
                                      const int64_t *d_row_offsets, size_t total_rows, const int32_t *d_slots, size_t pool_streams, float scale,
                                      float *d_pool, float *d_out, void *stream);
int ss_kstream_fbank_packed(const ss_kaldi_config *cfg, const float *x, size_t n_active, const int64_t *sample_offsets, const int32_t *slots,
                            size_t pool_streams, float *pool, float *out, float *log_energy);
int ss_kstream_mfcc_packed(const ss_kaldi_config *cfg, const float *x, size_t n_active, const int64_t *sample_offsets, const int32_t *slots,
                           size_t pool_streams, float *pool, float *out);
int ss_kstream_fbank_packed_i16(const ss_kaldi_config *cfg, const int16_t *x, size_t n_active, const int64_t *sample_offsets,
                                const int32_t *slots, size_t pool_streams, float scale, float *pool, float *out, float *log_energy);
int ss_kstream_mfcc_packed_i16(const ss_kaldi_config *cfg, const int16_t *x, size_t n_active, const int64_t *sample_offsets,
                               const int32_t *slots, size_t pool_streams, float scale, float *pool, float *out);

/* ---- Whisper log-mel front end (whisper.audio.log_mel_spectrogram / transformers.WhisperFeatureExtractor) ------------------
 * The model input of Whisper and of the speech encoders built on it.  The reference crate has no such stage; this comment is the
 * definition and tests/whisper_model.py restates it in numpy f64.  For one clip x of len samples and a frame count n_frames >= 2:
 *     N   = n_frames * 160
 *     a   = x[:N] followed by zeros up to N                              (pad_or_trim)
 *     p   = np.pad(a, 200, mode="reflect")
 *     w   = 0.5 - 0.5 cos(2 pi n / 400), n = 0 .. 399                    (periodic Hann, formed in f64, rounded once)
 *     P[t, k] = |rfft(p[160 t : 160 t + 400] * w)[k]|^2, t = 0 .. n_frames - 1, k = 0 .. 200   (the frame at t = n_frames is never formed)
 *     mel = B @ P^T,  B = librosa.filters.mel(sr=16000, n_fft=400, n_mels=M, htk=False, norm="slaney"), [M x 201], f64 rounded once
 *     l   = log10(max(mel, 1e-10));  l = max(l, max(l over the whole [M x n_frames] block) - 8);  out = (l + 4) / 4
 *   out is [M x n_frames] per clip, mels outermost.  An empty or all-zero clip gives -1.5 everywhere.
 *   Arithmetic (f32): one 200-point complex transform of z[n] = p[2n] w[2n] + i p[2n+1] w[2n+1] per frame and the real-FFT untangle;
 *   mel[m] is the sum over the filter's non-zero taps in ascending k, each step one fmaf; a sum <= 1e-10 gives l = -10 exactly; the
 *   last step is out = conv(fmaf(max(l, mx - 8), 0.25f, 1.0f)) -- ONE fmaf -- with conv of ss_pad_packed (SS_PAD_F32 / _F16 / _BF16,
 *   bit for bit its rounding rules).  The dense and the packed call run the same kernel code: they cannot round differently.
 *   A SILENT frame is one whose every sample index, after reflection, lies at or beyond min(len, N): t >= 2 with 160 t - 200 >=
 *   min(len, N), or any t of an empty clip.  Its l is the constant -10; no sample of it is loaded and no transform is run.
 * Served: sample_rate 16000, n_fft 400, hop_length 160 exactly, 1 <= n_mels <= 128.  Any other valid combination (n_fft even,
 *   1 <= hop_length <= n_fft, sample_rate >= 1, n_mels >= 1) is SS_ERR_UNSUPPORTED; anything else SS_ERR_BAD_CONFIG; a struct_size
 *   other than sizeof(ss_whisper_params) SS_ERR_ARG.
 * The handle is opaque and immutable: the tables go to the device it was created on at creation, with a pinned device error word
 *   of its own (ss_whisper_config_device_status has ss_config_device_status's contract) and a block of per-clip maximum keys for
 *   SS_WHISPER_MAX_CLIPS clips.  Calls on ONE handle must be ordered on one stream (they share the keys block); use one handle per
 *   stream otherwise.
 * Dense call: every row of d_x ([batch] rows of n_samples, row stride ld >= n_samples) is a clip, padded or trimmed to n_frames * 160.
 * Packed call: clip b is d_x[so[b] .. so[b + 1]) (int64 table of n_clips + 1 entries on the device); every clip is padded or trimmed
 *   to the same n_frames, so out is the rectangular [n_clips x M x n_frames] model input.  d_lengths (int32 [n_clips], may be NULL)
 *   gets min(len / 160, n_frames), or -1 for a bad table entry (so[b] < 0 or so[b + 1] < so[b]): that clip's block is all -1.5, the
 *   handle's error word is raised and reported once (SS_ERR_DEVICE, by ss_whisper_config_device_status or the next call on the
 *   handle).  The grids depend on n_clips, n_frames and M only and nothing is read back: the call replays as a captured graph over
 *   changed device tables.  Every element of out and of d_lengths is written by every call.
 * Three launches on `stream`: ss_whisper_keys_kernel (keys, lengths, table check), ss_whisper_c200 (ss_last_kernel_name(); the
 *   log10 block in f32) and ss_whisper_floor_kernel<f32|f16|bf16> (floor, scale, conversion, 16-byte stores).  For SS_PAD_F32 the
 *   log10 block lives in d_out itself and d_work is NULL (it is not read); for the 16-bit types the caller passes
 *   ss_whisper_work_bytes of f32 scratch, 16-byte aligned.  Nothing is allocated inside a call.
 * Errors: n_frames < 2, n_frames * 160 >= 2^31, more than SS_WHISPER_MAX_CLIPS clips, null buffers, d_x not 4-byte or d_out /
 *   d_work not 16-byte aligned, ld < n_samples: SS_ERR_ARG.  batch or n_clips of zero: SS_OK, nothing launched.
 * _i16 forms (16-bit PCM): sample k is (float)x[k] * scale, scale a power of two in [2^-64, 2^64] (else SS_ERR_ARG, checked first
 *   among the data checks; 2^-15 is Whisper's own convention); `scale` stands behind ld (dense) or behind the sample offsets (packed).
 *   out in all three dtypes, d_lengths and the error status are bit for bit the float call's on the converted samples; every other
 *   rule is the float call's, except that d_x needs 2-byte alignment only.  The middle launch is the kernel's PCM build,
 *   ss_whisper_c200i: a sample pair is one dword at either parity of the clip's first sample.  No float copy of the samples exists;
 *   the host forms cross the link as int16.
 * Not served: streaming and pool forms (a stream has no clip maximum), dither, other sizes. */
#define SS_WHISPER_MAX_CLIPS 1048576
typedef struct ss_whisper_params {
    uint32_t struct_size; /* sizeof(ss_whisper_params) */
    uint32_t sample_rate; /* 16000 */
    uint32_t n_fft;       /* 400 */
    uint32_t hop_length;  /* 160 */
    uint32_t n_mels;      /* 80 (Whisper up to large-v2) or 128 (large-v3) */
} ss_whisper_params;
typedef struct ss_whisper_config ss_whisper_config; /* opaque */

/* host only, no device */
int ss_whisper_params_default(ss_whisper_params *p, uint32_t n_mels);
int ss_whisper_params_validate(const ss_whisper_params *p);
int ss_whisper_num_frames(size_t n_samples, size_t *n_frames);                     /* n_samples / 160 */
int ss_whisper_first_silent_frame(size_t len, size_t n_frames, size_t *t_silent);  /* n_frames if no frame is silent */
int ss_whisper_window(const ss_whisper_params *p, float *w);                       /* [400] */
int ss_whisper_mel_bank(const ss_whisper_params *p, float *bank);                  /* [n_mels x 201] */
int ss_whisper_work_bytes(const ss_whisper_params *p, size_t batch, size_t n_frames, int dtype, size_t *bytes); /* 0 for SS_PAD_F32 */

int ss_whisper_config_create(const ss_whisper_params *p, ss_whisper_config **out);
void ss_whisper_config_destroy(ss_whisper_config *cfg);
int ss_whisper_config_params(const ss_whisper_config *cfg, ss_whisper_params *out);
int ss_whisper_config_device_status(const ss_whisper_config *cfg);

int ss_whisper_log_mel_device(const ss_whisper_config *cfg, const float *d_x, size_t batch, size_t n_samples, size_t ld, size_t n_frames,
                              int dtype, void *d_work, void *d_out, void *stream);
int ss_whisper_log_mel(const ss_whisper_config *cfg, const float *x, size_t batch, size_t n_samples, size_t ld, size_t n_frames, int dtype,
                       void *out);
int ss_whisper_log_mel_packed_device(const ss_whisper_config *cfg, const float *d_x, size_t n_clips, const int64_t *d_sample_offsets,
                                     size_t n_frames, int dtype, void *d_work, void *d_out, int32_t *d_lengths, void *stream);
int ss_whisper_log_mel_packed(const ss_whisper_config *cfg, const float *x, size_t n_clips, const int64_t *sample_offsets, size_t n_frames,
                              int dtype, void *out, int32_t *lengths);
int ss_whisper_log_mel_i16_device(const ss_whisper_config *cfg, const int16_t *d_x, size_t batch, size_t n_samples, size_t ld, float scale,
                                  size_t n_frames, int dtype, void *d_work, void *d_out, void *stream);
int ss_whisper_log_mel_i16(const ss_whisper_config *cfg, const int16_t *x, size_t batch, size_t n_samples, size_t ld, float scale,
                           size_t n_frames, int dtype, void *out);
int ss_whisper_log_mel_packed_i16_device(const ss_whisper_config *cfg, const int16_t *d_x, size_t n_clips, const int64_t *d_sample_offsets,
                                         float scale, size_t n_frames, int dtype, void *d_work, void *d_out, int32_t *d_lengths, void *stream);
int ss_whisper_log_mel_packed_i16(const ss_whisper_config *cfg, const int16_t *x, size_t n_clips, const int64_t *sample_offsets, float scale,
                                  size_t n_frames, int dtype, void *out, int32_t *lengths);

/* ---- NeMo / Parakeet log-mel front end (NeMo's AudioToMelSpectrogramPreprocessor / FilterbankFeatures;
 *      transformers.ParakeetFeatureExtractor) ----------------------------------------------------------------------------------
 * The model input of the NeMo family of encoders: Parakeet, Canary, FastConformer and the models built on them.  The reference
 * crate has no such stage; this comment is the definition and tests/nemo_model.py restates it in numpy f64.  Sizes: sample_rate
 * 16000, n_fft N = 512, hop_length H = 160, win_length W even in [258, 512] (default 400), lo = (N - W) / 2.  For one clip x of len
 * samples:
 *   1. T = len / H rounded down (the extractor's features_lengths: torch.stft yields one frame more, which is dropped).  T = 0 is
 *      allowed: the clip has no rows.
 *   2. y[i] = fmaf(-c, x[i - 1], x[i]) for 0 <= i < len with x[-1] = 0, c = preemph (0: the samples as they are); y[i] = 0 for every
 *      other i -- the zero beyond len is applied AFTER the pre-emphasis, as the extractor's masked_fill does.
 *   3. frame t, n = 0 .. W - 1: s[n] = y[t H - N / 2 + lo + n] * w[n], w[n] = 0.5 - 0.5 cos(2 pi n / (W - 1)) (the symmetric Hann
 *      window, formed in f64, rounded once).  The frames are centred with ZERO padding: the first ones begin before the clip, the
 *      last ones end behind it.
 *   4. P[k] = |sum_n s[n] exp(-2 pi i k n / N)|^2, k = 0 .. 256: the live samples sit at positions 0 .. W - 1 of the transform (the
 *      shift by lo that torch.stft applies changes the phase only).
 *   5. mel[m] = sum_k B[m, k] P[k], B = librosa.filters.mel(sr=16000, n_fft=512, n_mels, fmin=0, fmax=8000, norm="slaney"),
 *      [n_mels x 257], formed in f64 and rounded to f32; the Nyquist bin has weight 0 in it.
 *   6. l = ln(mel + log_guard), log_guard = 2^-24.
 *   7. normalize = SS_NEMO_NORM_NONE: row t = l.
 *   8. SS_NEMO_NORM_PER_FEATURE: per band over the clip's own T rows, mean = sum l / T, var = sum (l - mean)^2 / (T - 1) (ddof = 1),
 *      out = (l - mean) / (sqrt(var) + norm_eps), norm_eps = 1e-5 (the f32 value, widened).  Both sums are formed in f64 in row
 *      order and the result is rounded to f32 once.  With T = 1 the deviation is taken as 0 and the row is all zeros: NeMo's own
 *      rule for a single frame; the extractor's text divides by T - 1 = 0 there and gives NaN, which is not reproduced.
 *   Output: packed float32 rows [total_frames x n_mels], the layout ss_specaug_packed / ss_pad_packed / ss_splice_packed take.
 *   Arithmetic (f32): steps 2 and 3 round every product and sum on their own (step 2 is one fmaf); one 256-point complex transform
 *   of the sample pairs and the real-FFT untangle; mel[m] over the filter's taps in ascending k, one fmaf a step; step 6 is
 *   v_log_f32 of fmaf(0.25, sum |2X|^2 B, log_guard) times ln 2.  The dense and the packed call run the same kernel code.
 * Served: sample_rate / n_fft / hop_length = 16000 / 512 / 160 and n_mels <= 128; anything else that is a valid combination is
 *   SS_ERR_UNSUPPORTED.  SS_ERR_BAD_CONFIG: n_mels < 1, a win_length that is odd or outside [258, 512], a preemph, log_guard or
 *   norm_eps that is negative or not finite, log_guard = 0, an unknown normalize, sample_rate / hop_length = 0, an odd n_fft.  A
 *   struct_size other than sizeof(ss_nemo_params) is SS_ERR_ARG.
 * The handle is opaque and immutable: the tables go to the device it was created on, with a pinned device error word of its own
 *   (ss_nemo_config_device_status has ss_kaldi_config_device_status's contract).
 * Dense call: every row of d_x ([batch] rows of n_samples, row stride ld >= n_samples) is a clip; out is [batch x T x n_mels].
 * Packed call: clip b is d_x[so[b] .. so[b + 1]) and owns rows fo[b] .. fo[b + 1]; both tables are int64 [n_clips + 1] on the device
 *   (ss_nemo_packed_frame_offsets computes fo on the host; the offsets ss_resample_packed_offsets wrote are valid sample offsets as
 *   they stand).  A clip whose entries are inconsistent -- negative length, longer than 2^31 - 1 samples, rows that are not the
 *   T its samples give, rows past total_frames -- is skipped by every launch: nothing of it is loaded and nothing stored, the
 *   handle's error word is raised and reported once (SS_ERR_DEVICE, by ss_nemo_config_device_status or the next call on the
 *   handle).  No sample outside [so[b], so[b + 1]) is fetched for clip b: what lies there belongs to the neighbour.
 * One launch of ss_nemo_c256<NE[,v]> (ss_last_kernel_name(); NE = 10 / 13 / 16 live sample pairs per lane for W <= 320 / 416 / 512,
 *   v: packed), then with SS_NEMO_NORM_PER_FEATURE ss_nemo_norm_kernel in place on the rows.  Both queue on `stream` only; the grids
 *   depend on the row count, n_clips and n_mels; nothing is allocated or read back inside a call, so the calls replay as a captured
 *   graph over changed device tables.
 * The host forms stage through the device; the packed one refuses a bad sample table (SS_ERR_ARG) before any launch.
 * Stream pools, fed floats or 16-bit PCM: the ss_nstream_* section below.
 * Not served: 16-bit PCM twins of these one-shot calls, dither, other n_fft / hop_length / sample rates, normalize = "all_features",
 *   narrow-band fmin / fmax, NaN for T = 1. */
#define SS_NEMO_NORM_NONE 0
#define SS_NEMO_NORM_PER_FEATURE 1
typedef struct ss_nemo_params {
    uint32_t struct_size; /* sizeof(ss_nemo_params) */
    uint32_t sample_rate; /* 16000 */
    uint32_t n_fft;       /* 512 */
    uint32_t win_length;  /* even, 258 .. 512; 400 */
    uint32_t hop_length;  /* 160 */
    uint32_t n_mels;      /* 80 or 128 (1 .. 128) */
    int32_t normalize;    /* SS_NEMO_NORM_* */
    float preemph;        /* 0.97; 0: none */
    float log_guard;      /* 2^-24 */
    float norm_eps;       /* 1e-5 */
} ss_nemo_params;
typedef struct ss_nemo_config ss_nemo_config; /* opaque */

/* host only, no device */
int ss_nemo_params_default(ss_nemo_params *p, uint32_t n_mels);
int ss_nemo_params_validate(const ss_nemo_params *p);
int ss_nemo_num_frames(const ss_nemo_params *p, size_t n_samples, size_t *n_frames); /* n_samples / 160; 0 is a result */
int ss_nemo_packed_frame_offsets(const ss_nemo_params *p, size_t n_clips, const int64_t *sample_offsets, int64_t *frame_offsets);
int ss_nemo_window(const ss_nemo_params *p, float *w);      /* [win_length] */
int ss_nemo_mel_bank(const ss_nemo_params *p, float *bank); /* [n_mels x 257] */

int ss_nemo_config_create(const ss_nemo_params *p, ss_nemo_config **out);
void ss_nemo_config_destroy(ss_nemo_config *cfg);
int ss_nemo_config_params(const ss_nemo_config *cfg, ss_nemo_params *out);
int ss_nemo_config_device_status(const ss_nemo_config *cfg);

int ss_nemo_log_mel_device(const ss_nemo_config *cfg, const float *d_x, size_t batch, size_t n_samples, size_t ld, float *d_out, void *stream);
int ss_nemo_log_mel(const ss_nemo_config *cfg, const float *x, size_t batch, size_t n_samples, size_t ld, float *out);
int ss_nemo_log_mel_packed_device(const ss_nemo_config *cfg, const float *d_x, size_t n_clips, const int64_t *d_sample_offsets,
                                  const int64_t *d_frame_offsets, size_t total_frames, float *d_out, void *stream);
int ss_nemo_log_mel_packed(const ss_nemo_config *cfg, const float *x, size_t n_clips, const int64_t *sample_offsets, float *out);

/* ---- ss_nstream_*: the NeMo / Parakeet front end over a pool of stream states (live audio) -------------------------
 * The online form of ss_nemo_log_mel with normalize = SS_NEMO_NORM_NONE -- the input of cache-aware FastConformer and the real-time
 * Parakeet models -- on the tables of the other stream pools (ss_resample_stream_packed*, ss_kstream_*, ss_cmvn_stream_packed*,
 * ss_splice_stream_packed*): one set of sample_offsets / row_offsets / slots serves the whole chain.  The handle is
 * an ss_nemo_config; the arithmetic is steps 2 - 6 of the ss_nemo_* specification above, on the same kernel body.  (The prefix is
 * ss_nstream_, not ss_nemo_: the set of ss_nemo_* names is closed.)
 * Sizes, with W = win_length and H = 160: L = ceil(W / 320) - 1 is the delay in rows (0 for W <= 320, else 1) -- a centred frame
 *   reaches W / 2 samples past its hop -- and S = L * 160 + W / 2 + 1 the carried samples per stream: the frame's reach plus the one
 *   pre-emphasis predecessor (ss_nstream_state_len, which reads the sizes only; W = 400: L = 1, S = 361; W = 320: L = 0, S = 161;
 *   W = 512: L = 1, S = 417).
 * Pool: a caller-owned [pool_streams x S] block of floats.  An all-zero row is a fresh stream; zeroing a row resets it.
 * Entries (the rules of ss_kstream_*): a call serves n_active entries.  Entry i's chunk is x[so[i] : so[i+1]], R_i = n_i / 160 whole
 *   hops (R_i = 0 is legal); its state is pool row slots[i]; its rows are rows ro[i] .. ro[i+1] of the packed [total_rows x n_mels]
 *   float32 output (ss_nstream_row_offsets); total_rows >= ro[n_active], rows past ro[n_active] are left alone.  Row t of an entry is
 *   steps 2 - 6 on ONE frame: its first live sample is chunk position p0 = 160 (t - L) - W / 2, a position p < 0 being
 *   pool[slot * S + S + p]; the pre-emphasis predecessor of the first sample is position p0 - 1.  Every position a row reads lies in
 *   [-S, 160 (t + 1)); nothing is masked.  Afterwards the pool row is the last S samples of (old row ++ chunk).
 * Flush (ss_nstream_flush*): takes no samples.  Entry i gets exactly L rows, out[i * L .. (i + 1) * L) of [n_active * L x n_mels]: row
 *   u is the frame that starts at position 160 (u - L) - W / 2 relative to the stream's end, every position at or beyond the end being
 *   zero AFTER the pre-emphasis (step 2's masked fill).  Afterwards the named pool rows are all zeros (as ss_resample_stream_flush*
 *   leaves them): the slot is a fresh stream.  With L = 0 nothing is written (d_out may be NULL) and the rows are zeroed all the same.
 * Equivalence: however a stream of K whole hops was cut into calls -- empty entries included, float and PCM calls mixed, whatever
 *   else shares the call and whatever the entry's place or slot -- its K pool rows are bit for bit rows 0 .. K - 1 of
 *   ss_nemo_log_mel_device (a SS_NEMO_NORM_NONE handle) on zeros(L * 160) ++ stream, and the pool rows with the first L dropped,
 *   followed by the flush rows, are bit for bit ss_nemo_log_mel_device on the stream itself (K rows).  THE FIRST L ROWS AFTER A RESET
 *   ARE WARM-UP ROWS over the zero prefix.  A trailing partial hop is the caller's to drop (or to keep for the next call): neither
 *   call takes one.
 * A handle with SS_NEMO_NORM_PER_FEATURE is SS_ERR_UNSUPPORTED on every call that takes a handle: a stream has no clip statistics.
 *   ss_cmvn_stream_packed* or ss_cmvn_apply_packed* chains behind the pool instead.
 * Containment: the skip rules are the frame pool's.  A bad entry (not whole hops, ro inconsistent, ro[i+1] > total_rows, slot outside
 *   the pool; for the flush: slot outside the pool) is skipped by every launch -- its rows and its pool row stay untouched -- and
 *   raises the handle's error word: SS_ERR_DEVICE once, through ss_nemo_config_device_status or the next call on the handle.
 *   Nothing is read outside the entries' chunk ranges and the named pool rows; nothing is written outside rows [0, total_rows) and
 *   the named pool rows.
 * Arguments: n_active == 0 is SS_OK with no launch.  SS_ERR_ARG, with nothing touched, for null buffers, sizes >= 2^31 and a pool
 *   range that overlaps an output.  The host forms check the tables first and name the first bad entry (ss_nstream_row_offsets'
 *   rules: so[0] == 0, no decreasing pair, whole hops), reject duplicate slots, and write the caller's pool only after everything
 *   else succeeded.
 * _i16 forms: sample = (float)pcm * scale, scale a power of two in [2^-64, 2^64] (else SS_ERR_ARG).  The results are bit for bit
 *   the float call on the converted samples; the pool stays float, so a stream may alternate between PCM and float chunks.  The
 *   device forms need 2-byte alignment of d_x only (W / 2 may be odd: a frame starts at either parity).
 * The pool call is a linear chain of two launches on `stream` -- ss_nemo_c256<NE,sp> (,spi> for PCM; ss_last_kernel_name()) and the
 *   frame pool's state advance; the flush is ss_nemo_c256<NE,fl> (no launch where L = 0) and the zeroing of the named rows.  The grids
 *   depend on n_active and total_rows only; nothing is allocated or read back: capturable, and replayable over changed table contents.
 * Not served: a partial-hop tail in the flush, per-feature normalisation inside the pool, dither, 16-bit PCM twins of the one-shot
 *   ss_nemo_* calls. */
int ss_nstream_state_len(const ss_nemo_params *p, size_t *state_len, size_t *delay_rows); /* host only */
int ss_nstream_row_offsets(const ss_nemo_params *p, size_t n_active, const int64_t *sample_offsets, int64_t *row_offsets); /* host only */
int ss_nstream_log_mel_packed_device(const ss_nemo_config *cfg, const float *d_x, size_t n_active, const int64_t *d_sample_offsets,
                                     const int64_t *d_row_offsets, size_t total_rows, const int32_t *d_slots, size_t pool_streams, float *d_pool,
                                     float *d_out, void *stream);
int ss_nstream_log_mel_packed(const ss_nemo_config *cfg, const float *x, size_t n_active, const int64_t *sample_offsets, const int32_t *slots,
                              size_t pool_streams, float *pool, float *out);
int ss_nstream_log_mel_packed_i16_device(const ss_nemo_config *cfg, const int16_t *d_x, size_t n_active, const int64_t *d_sample_offsets,
                                         const int64_t *d_row_offsets, size_t total_rows, const int32_t *d_slots, size_t pool_streams, float scale,
                                         float *d_pool, float *d_out, void *stream);
int ss_nstream_log_mel_packed_i16(const ss_nemo_config *cfg, const int16_t *x, size_t n_active, const int64_t *sample_offsets,
                                  const int32_t *slots, size_t pool_streams, float scale, float *pool, float *out);
int ss_nstream_flush_device(const ss_nemo_config *cfg, size_t n_active, const int32_t *d_slots, size_t pool_streams, float *d_pool, float *d_out,
                            void *stream);
int ss_nstream_flush(const ss_nemo_config *cfg, size_t n_active, const int32_t *slots, size_t pool_streams, float *pool, float *out);

/* ---- multi-GPU callers below Python (one process or thread per GPU) -------------------------------------
 * Clips are independent, so a batch shards by contiguous blocks with no exchange inside the path: rank r of `world`
 * computes clips [lo, hi) of ss_shard_bounds on its own device with the *_device entry points.  The north-star's "RCCL
 * gather over xGMI of the final [n_frames x n_mfcc] blocks" is ss_gather_features: every rank passes its block of
 * elems_per_rank floats (pad uneven shards to the largest); rank `root` receives [world x elems_per_rank] in rank order
 * (one ncclRecv per peer and one device copy of its own block inside an ncclGroup: every peer has a direct xGMI link to
 * the root, so the blocks arrive concurrently), the other ranks only send (d_out may be NULL there).
 * ss_all_gather_features is the all-to-all form for consumers that need the whole corpus on every GPU (one
 * ncclAllGather; every rank then writes (world - 1) blocks into its HBM).
 * `nccl_comm` is the caller's ncclComm_t and MUST come from the RCCL library this one resolves: the copy already mapped
 * into the process (e.g. torch's bundled librccl.so) is preferred, then librccl.so.1 / librccl.so by name;
 * ss_rccl_library(path) names the library explicitly (before the first collective) -- passing a communicator created by a
 * different RCCL copy is undefined behaviour.  Nothing is linked at build time.  The automatic search runs ONCE per process: if
 * the first collective finds no RCCL (it ran before torch / librccl was mapped), every later collective fails with SS_ERR_HIP
 * as well until ss_rccl_library(path) is called -- load RCCL first, or name it. */
int ss_shard_bounds(size_t n_items, int world, int rank, size_t *lo, size_t *hi);
int ss_rccl_library(const char *path);
int ss_gather_features(void *nccl_comm, const float *d_block, size_t elems_per_rank, float *d_out, int root, int rank,
                       int world, void *stream);
int ss_all_gather_features(void *nccl_comm, const float *d_block, size_t elems_per_rank, float *d_out, void *stream);

/* ---- device / diagnostics ------------------------------------------------------------------- */

int ss_device_count(int *count);
int ss_set_device(int device);
/* name of the kernel the last *_device call on this thread launched (for rocprof cross-checks) */
const char *ss_last_kernel_name(void);
/* Times `iters` back-to-back launches of the MFCC batch kernel with HIP events recorded on `stream`
 * (the stream the kernel runs on) and returns the average launch duration in milliseconds. */
int ss_time_mfcc_batch_device(const ss_config *cfg, const float *d_x, size_t batch, size_t n_samples, size_t ld,
                              float *d_out, void *stream, int iters, float *avg_ms);
int ss_time_mel_spectrogram_device(const ss_config *cfg, const float *d_x, size_t channels, size_t n_samples,
                                   size_t ld, float *d_out, void *stream, int iters, float *avg_ms);

/* Shader clock (GHz) the part held during `launches` launches of the MFCC batch kernel on `stream`: every wave of the kernel
 * writes its lifetime once, in shader cycles and on the constant 100 MHz clock, into a buffer that THIS CALL owns; the result
 * is the mean ratio over the waves of the last launch.  A per-call diagnostic (bench.py's roofline.clock_ghz_measured): no
 * process-wide state, other threads' launches are unaffected.  The stamps exist in the fft_points = 512 kernel:
 * SS_ERR_UNSUPPORTED for configurations served by another kernel. */
int ss_mfcc_shader_clock(const ss_config *cfg, const float *d_x, size_t batch, size_t n_samples, size_t ld, float *d_out,
                         void *stream, int launches, float *ghz);

/* A timed region whose duration and shader clock come from the SAME launches (bench.py's secondary.cfg2 / cfg5): `launches`
 * launches of the MFCC batch kernel on `stream`, launch i reading d_x[i % n_x] and writing d_out[i % n_out] (host arrays of device pointers: a
 * ring of inputs larger than the 256 MiB Infinity Cache keeps the samples coming from HBM), HIP events recorded on `stream` around
 * all of them, and the per-wave stamps of the LAST min(stamped, launches, 4096) launches kept, each launch in a slot of its own of
 * a buffer this call owns.  *avg_ms = region / launches; *ghz = (sum of the waves' shader cycles) / (sum of their lifetimes on
 * the 100 MHz clock) over every stamped launch; stamped = 0 times only.  *wall_ms (may be NULL) = host time from the first launch
 * call to the completion of the last launch (the region starts on a synchronised stream; reading the stamps back is not part of
 * it).  SS_ERR_UNSUPPORTED (after timing) where the launches ran on a kernel without stamps.  Blocks until the region has run. */
int ss_mfcc_timed_region(const ss_config *cfg, const float *const *d_x, size_t n_x, size_t batch, size_t n_samples, size_t ld,
                         float *const *d_out, size_t n_out, void *stream, int launches, int stamped, float *avg_ms, float *ghz,
                         float *wall_ms);

/* The same for the mel-spectrogram path.  The wave stamps exist in the 512-point MFCC kernel and in the twelve-wave builds of the
 * 4096-point MFCC kernel (default shape) and of the 2048-point mel kernel (the builds of BASELINE configurations 2 / 4, 5 and 3):
 * with stamped > 0 on any other kernel both functions time the region and then return SS_ERR_UNSUPPORTED. */
int ss_mel_spectrogram_timed_region(const ss_config *cfg, const float *const *d_x, size_t n_x, size_t channels, size_t n_samples,
                                    size_t ld, float *const *d_out, size_t n_out, void *stream, int launches, int stamped,
                                    float *avg_ms, float *ghz, float *wall_ms);

/* Shader clock (GHz) of the device while WHATEVER ELSE runs on it: one wave on `stream` sleeps through a lead-in (a tenth of
 * `micros`, at most 200 us), reads the shader-cycle counter and the constant 100 MHz counter, sleeps (no memory traffic, no LDS,
 * a handful of registers) for about `micros` microseconds and reads both again; *ghz = cycles / time.  Call it on a side stream
 * FIRST (from a thread of its own: the call blocks) and launch the kernels of interest on their stream right behind it: the
 * probe wave is resident before they start, fits beside the persistent workgroups (they leave wave slots free) and sees the
 * clock the part holds under that load (the power cap).  Enqueued BEHIND a backlog of launches it may only start
 * when the backlog has drained and read the idle clock; the call may also return only once the other stream is idle.  Works
 * for every kernel of the library (bench.py's clock_ghz_measured where a kernel has no stamps of its own; checked against the
 * 512-point kernel's own stamps in profiles/r05/clock_probe_check.txt).  10 <= micros <= 1 000 000. */
int ss_shader_clock_probe(void *stream, uint32_t micros, float *ghz);
/* The same probe without the wait: queues the one-wave kernel on `stream` and returns; when the stream has run it,
 * d_words[0] = shader cycles and d_words[1] = ticks of the 100 MHz counter over the counted interval (GHz = d_words[0] /
 * (10 * d_words[1])).  `d_words`: two 64-bit words of device memory.  This is the form to queue AHEAD of the launches to watch. */
int ss_shader_clock_probe_async(void *stream, uint32_t micros, unsigned long long *d_words);

/* Process-wide test aids (LDS poisoning, kernel-selection overrides, fault injection, a stamp buffer) are NOT part of this
 * library: include/speechsauce_amd_debug.h, exported by the lab build libspeechsauce_amd_lab.so only. */

const char *ss_status_string(int status);
const char *ss_last_error_string(void); /* thread-local detail of the last failure */
int ss_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* SPEECHSAUCE_AMD_H */
