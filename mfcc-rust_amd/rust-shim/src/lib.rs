//! `speechsauce-amd`: the hot-path API of the `speechsauce` crate on an MI355X.
//!
//! Drop-in by module path: the crate has the reference's public modules (`speechsauce/src/lib.rs:2-6`) -- `config`, `feature`,
//! `functions`, `processing`, `util` -- so with `speechsauce = { package = "speechsauce-amd", path = ".." }` in Cargo.toml an
//! existing `use speechsauce::feature::mfcc;` keeps compiling with no source edit.  Every item also stays at the crate root.
//! Signatures follow the reference one for one:
//!   speechsauce::feature::mfcc(ArrayView1<f32>, &SpeechConfig) -> Array2<f32>          (feature.rs:99)
//!   speechsauce::feature::mfe(ArrayView1<f32>, &SpeechConfig) -> (Array2, Array1)       (feature.rs:200)
//!   speechsauce::feature::mel_spectrogram1 / mel_spectrogram2                           (feature.rs:151,163)
//!   speechsauce::processing::preemphasis(Array1<f32>, isize, f32) -> Array1<f32>        (processing.rs:31)
//!   speechsauce::processing::stack_frames(signal, sample_rate, frame_length, frame_stride, filter, zero_padding)
//!   speechsauce::processing::power_spectrum(frames, fft_points)                         (processing.rs:65,179)
//!   speechsauce::functions::stft1 / stft2 -> Array2 / Array3<Complex32>                 (functions.rs:199,86)
//!   speechsauce::config::{SpeechConfig, SpeechConfigBuilder}                            (config.rs:10-190)
//! The host side here owns what the north-star assigns to Rust: ndarray I/O (contiguity, shapes,
//! allocation of the outputs) and the framing parameters; every numeric step runs in the HIP kernels
//! behind the `extern "C"` layer of include/speechsauce_amd.h.  Where the reference panics these
//! functions panic too, with the library's error text (`expect`-style), so behaviour under bad input is
//! unchanged for existing callers; `try_*` variants return `Result`.
//!
//! `SpeechConfig` is `Clone` like the reference's (config.rs:98): clones share one immutable device handle (`Arc`), which is
//! released when the last clone drops.  Its public fields are the reference's plain-data fields (config.rs:100-126), including
//! `window_size_half`, `frame_size`, `wnorm` and `window`; the reference's five fields that hold third-party plan objects or
//! streaming state (`analysis_mem`, `dct_handler`, `fft_handler`, `fft_forward`, `analysis_scratch`) have no counterpart: the
//! plans live on the device and the STFT starts from zero state per call.
//!
//! This file is shipped uncompiled (the build image has no Rust toolchain): NEVER COMPILED, checked textually by
//! tests/test_binding_mirrors.py.

use ndarray::{Array, Array1, Array2, Array3, ArrayView1, ArrayView2, Dimension};
use num_complex::Complex32;
use std::ffi::CStr;
use std::os::raw::{c_char, c_int, c_long, c_void};
use std::sync::Arc;

#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct SsParams {
    pub struct_size: u32,
    pub sample_rate: u32,
    pub fft_points: u32,
    pub frame_length: f32,
    pub frame_stride: f32,
    pub num_cepstral: u32,
    pub num_filters: u32,
    pub low_frequency: f32,
    pub high_frequency: f32,
    pub dc_elimination: i32,
    pub framing: i32,
    pub spectrum_exponent: i32,
    pub dct_norm: i32,
    pub dct2_gain: f32,
    pub mfcc_window: i32,
    pub preemph_coef: f32,
    pub preemph_shift: i32,
    /// librosa-compatible variants (0 = reference mode): SS_MEL_*, SS_MEL_NORM_*, SS_PAD_*
    pub mel_scale: i32,
    pub mel_norm: i32,
    pub pad_mode: i32,
}

#[repr(C)]
pub struct SsConfig {
    _private: [u8; 0],
}

extern "C" {
    fn ss_params_default(p: *mut SsParams, sample_rate: u32) -> c_int;
    fn ss_config_create(p: *const SsParams, out: *mut *mut SsConfig) -> c_int;
    fn ss_config_destroy(cfg: *mut SsConfig);
    fn ss_num_frames(p: *const SsParams, n_samples: usize, n_frames: *mut usize) -> c_int;
    fn ss_stft_rows(p: *const SsParams, n_samples: usize, rows: *mut usize, real_rows: *mut usize) -> c_int;
    fn ss_stft_sizes(p: *const SsParams, hop: *mut usize, n_pad: *mut usize, wnorm: *mut f32) -> c_int;  // (stft_sizes below)
    fn ss_vorbis_window(n: usize, w: *mut f32) -> c_int;
    fn ss_mfcc(cfg: *const SsConfig, x: *const f32, n: usize, out: *mut f32) -> c_int;
    fn ss_mfe(cfg: *const SsConfig, x: *const f32, n: usize, feat: *mut f32, energy: *mut f32) -> c_int;
    fn ss_lmfe(cfg: *const SsConfig, x: *const f32, n: usize, feat: *mut f32) -> c_int;
    fn ss_mel_spectrogram(cfg: *const SsConfig, x: *const f32, channels: usize, n: usize, out: *mut f32) -> c_int;
    fn ss_mfcc_batch(cfg: *const SsConfig, x: *const f32, batch: usize, n: usize, ld: usize, out: *mut f32) -> c_int;
    fn ss_mfcc_batch_device(cfg: *const SsConfig, d_x: *const f32, batch: usize, n: usize, ld: usize, d_out: *mut f32,
                            stream: *mut c_void) -> c_int;
    fn ss_mfcc_batches_device(cfg: *const SsConfig, n_batches: usize, d_x: *const *const f32, batch: *const usize, n: usize, ld: usize,
                              d_out: *const *mut f32, stream: *mut c_void) -> c_int;
    fn ss_mfcc_stream_packed_i16_device(cfg: *const SsConfig, d_x: *const i16, n_active: usize, d_sample_offsets: *const i64,
                                        d_row_offsets: *const i64, total_rows: usize, d_slots: *const i32, pool_streams: usize,
                                        scale: f32, norm_frames: u32, d_pool: *mut f32, d_out: *mut f32, stream: *mut c_void) -> c_int;
    fn ss_mfe_stream_packed_i16_device(cfg: *const SsConfig, d_x: *const i16, n_active: usize, d_sample_offsets: *const i64,
                                       d_row_offsets: *const i64, total_rows: usize, d_slots: *const i32, pool_streams: usize,
                                       scale: f32, d_pool: *mut f32, d_feat: *mut f32, d_energy: *mut f32, stream: *mut c_void) -> c_int;
    fn ss_mfcc_stream_packed_i16(cfg: *const SsConfig, x: *const i16, n_active: usize, sample_offsets: *const i64, slots: *const i32,
                                 pool_streams: usize, scale: f32, norm_frames: u32, pool: *mut f32, out: *mut f32) -> c_int;
    fn ss_mfe_stream_packed_i16(cfg: *const SsConfig, x: *const i16, n_active: usize, sample_offsets: *const i64, slots: *const i32,
                                pool_streams: usize, scale: f32, pool: *mut f32, feat: *mut f32, energy: *mut f32) -> c_int;
    fn ss_mfcc_batch_i16_device(cfg: *const SsConfig, d_x: *const i16, batch: usize, n: usize, ld: usize, scale: f32, d_out: *mut f32,
                                stream: *mut c_void) -> c_int;
    fn ss_mfe_batch_i16_device(cfg: *const SsConfig, d_x: *const i16, batch: usize, n: usize, ld: usize, scale: f32, d_feat: *mut f32,
                               d_energy: *mut f32, stream: *mut c_void) -> c_int;
    fn ss_mfcc_packed_i16_device(cfg: *const SsConfig, d_x: *const i16, n_clips: usize, d_sample_offsets: *const i64, scale: f32,
                                 d_frame_offsets: *const i64, total_frames: usize, d_out: *mut f32, stream: *mut c_void) -> c_int;
    fn ss_mfe_packed_i16_device(cfg: *const SsConfig, d_x: *const i16, n_clips: usize, d_sample_offsets: *const i64, scale: f32,
                                d_frame_offsets: *const i64, total_frames: usize, d_feat: *mut f32, d_energy: *mut f32,
                                stream: *mut c_void) -> c_int;
    fn ss_mfcc_batch_i16(cfg: *const SsConfig, x: *const i16, batch: usize, n: usize, ld: usize, scale: f32, out: *mut f32) -> c_int;
    fn ss_mfe_batch_i16(cfg: *const SsConfig, x: *const i16, batch: usize, n: usize, ld: usize, scale: f32, feat: *mut f32,
                        energy: *mut f32) -> c_int;
    fn ss_mfcc_packed_i16(cfg: *const SsConfig, x: *const i16, n_clips: usize, sample_offsets: *const i64, scale: f32,
                          out: *mut f32) -> c_int;
    fn ss_mfe_packed_i16(cfg: *const SsConfig, x: *const i16, n_clips: usize, sample_offsets: *const i64, scale: f32, feat: *mut f32,
                         energy: *mut f32) -> c_int;
    fn ss_mel_spectrogram_i16_device(cfg: *const SsConfig, d_x: *const i16, channels: usize, n: usize, ld: usize, scale: f32,
                                     d_out: *mut f32, stream: *mut c_void) -> c_int;
    fn ss_stft_i16_device(cfg: *const SsConfig, d_x: *const i16, channels: usize, n: usize, ld: usize, scale: f32, d_out: *mut f32,
                          stream: *mut c_void) -> c_int;
    fn ss_mel_spectrogram_i16(cfg: *const SsConfig, x: *const i16, channels: usize, n: usize, scale: f32, out: *mut f32) -> c_int;
    fn ss_stft_i16(cfg: *const SsConfig, x: *const i16, channels: usize, n: usize, scale: f32, out: *mut f32) -> c_int;
    fn ss_mel_spectrogram_packed_i16_device(cfg: *const SsConfig, d_x: *const i16, n_clips: usize, d_sample_offsets: *const i64,
                                            scale: f32, d_row_offsets: *const i64, total_rows: usize, d_out: *mut f32,
                                            stream: *mut c_void) -> c_int;
    fn ss_stft_packed_i16_device(cfg: *const SsConfig, d_x: *const i16, n_clips: usize, d_sample_offsets: *const i64, scale: f32,
                                 d_row_offsets: *const i64, total_rows: usize, d_out: *mut f32, stream: *mut c_void) -> c_int;
    fn ss_mel_spectrogram_packed_i16(cfg: *const SsConfig, x: *const i16, n_clips: usize, sample_offsets: *const i64, scale: f32,
                                     out: *mut f32) -> c_int;
    fn ss_stft_packed_i16(cfg: *const SsConfig, x: *const i16, n_clips: usize, sample_offsets: *const i64, scale: f32,
                          out: *mut f32) -> c_int;
    fn ss_log_mel_spectrogram(cfg: *const SsConfig, x: *const f32, channels: usize, n: usize, ref_: f32, amin: f32, top_db: f32,
                              out: *mut f32) -> c_int;
    fn ss_log_mel_spectrogram_device(cfg: *const SsConfig, d_x: *const f32, channels: usize, n: usize, ld: usize, ref_: f32, amin: f32,
                                     top_db: f32, d_out: *mut f32, stream: *mut c_void) -> c_int;
    fn ss_log_mel_spectrogram_i16(cfg: *const SsConfig, x: *const i16, channels: usize, n: usize, scale: f32, ref_: f32, amin: f32,
                                  top_db: f32, out: *mut f32) -> c_int;
    fn ss_log_mel_spectrogram_i16_device(cfg: *const SsConfig, d_x: *const i16, channels: usize, n: usize, ld: usize, scale: f32,
                                         ref_: f32, amin: f32, top_db: f32, d_out: *mut f32, stream: *mut c_void) -> c_int;
    fn ss_log_mel_spectrogram_packed(cfg: *const SsConfig, x: *const f32, n_clips: usize, sample_offsets: *const i64, ref_: f32,
                                     amin: f32, top_db: f32, out: *mut f32) -> c_int;
    fn ss_log_mel_spectrogram_packed_device(cfg: *const SsConfig, d_x: *const f32, n_clips: usize, d_sample_offsets: *const i64,
                                            d_row_offsets: *const i64, total_rows: usize, ref_: f32, amin: f32, top_db: f32,
                                            d_out: *mut f32, stream: *mut c_void) -> c_int;
    fn ss_log_mel_spectrogram_packed_i16(cfg: *const SsConfig, x: *const i16, n_clips: usize, sample_offsets: *const i64, scale: f32,
                                         ref_: f32, amin: f32, top_db: f32, out: *mut f32) -> c_int;
    fn ss_log_mel_spectrogram_packed_i16_device(cfg: *const SsConfig, d_x: *const i16, n_clips: usize, d_sample_offsets: *const i64,
                                                scale: f32, d_row_offsets: *const i64, total_rows: usize, ref_: f32, amin: f32,
                                                top_db: f32, d_out: *mut f32, stream: *mut c_void) -> c_int;
    fn ss_mel_spectrogram_stream_packed_i16_device(cfg: *const SsConfig, d_x: *const i16, n_active: usize, d_sample_offsets: *const i64,
                                                   d_row_offsets: *const i64, total_rows: usize, d_slots: *const i32, pool_streams: usize,
                                                   scale: f32, d_pool: *mut f32, d_out: *mut f32, stream: *mut c_void) -> c_int;
    fn ss_stft_stream_packed_i16_device(cfg: *const SsConfig, d_x: *const i16, n_active: usize, d_sample_offsets: *const i64,
                                        d_row_offsets: *const i64, total_rows: usize, d_slots: *const i32, pool_streams: usize,
                                        scale: f32, d_pool: *mut f32, d_out: *mut f32, stream: *mut c_void) -> c_int;
    fn ss_mel_spectrogram_stream_packed_i16(cfg: *const SsConfig, x: *const i16, n_active: usize, sample_offsets: *const i64,
                                            slots: *const i32, pool_streams: usize, scale: f32, pool: *mut f32, out: *mut f32) -> c_int;
    fn ss_stft_stream_packed_i16(cfg: *const SsConfig, x: *const i16, n_active: usize, sample_offsets: *const i64, slots: *const i32,
                                 pool_streams: usize, scale: f32, pool: *mut f32, out: *mut f32) -> c_int;
    fn ss_preemphasis(x: *const f32, n: usize, shift: c_long, cof: f32, y: *mut f32) -> c_int;
    fn ss_frame_sizes(p: *const SsParams, frame_len: *mut usize, frame_step: *mut usize) -> c_int;
    fn ss_stft(cfg: *const SsConfig, x: *const f32, channels: usize, n: usize, out: *mut f32) -> c_int;
    fn ss_stack_frames(cfg: *const SsConfig, x: *const f32, n: usize, frames: *mut f32) -> c_int;
    fn ss_stack_frames_shape(n_samples: usize, sample_rate: u32, frame_length: f32, frame_stride: f32, zero_padding: c_int,
                             num_frames: *mut usize, frame_len: *mut usize) -> c_int;
    fn ss_stack_frames_signal(x: *const f32, n_samples: usize, sample_rate: u32, frame_length: f32, frame_stride: f32,
                              window: *const f32, zero_padding: c_int, frames: *mut f32) -> c_int;
    fn ss_power_spectrum_frames(cfg: *const SsConfig, frames: *const f32, rows: usize, cols: usize, p_out: *mut f32) -> c_int;
    fn ss_power_spectrum(cfg: *const SsConfig, x: *const f32, n: usize, p_out: *mut f32) -> c_int;
    fn ss_config_device_status(cfg: *const SsConfig) -> c_int;
    fn ss_cmvn(vec: *const f32, rows: usize, cols: usize, variance_normalization: c_int, out: *mut f32) -> c_int;
    fn ss_cmvnw(vec: *const f32, rows: usize, cols: usize, win_size: usize, variance_normalization: c_int, out: *mut f32) -> c_int;
    fn ss_cmvn_packed(vec: *const f32, n_clips: usize, offsets: *const i64, total_rows: usize, cols: usize,
                      variance_normalization: c_int, out: *mut f32) -> c_int;
    fn ss_cmvnw_packed(vec: *const f32, n_clips: usize, offsets: *const i64, total_rows: usize, cols: usize, win_size: usize,
                       variance_normalization: c_int, out: *mut f32) -> c_int;
    fn ss_power_to_db_packed(s: *const f32, n_clips: usize, offsets: *const i64, total_rows: usize, cols: usize, ref_value: f32,
                             amin: f32, top_db: f32, out: *mut f32) -> c_int;
    fn ss_cmvn_stream_state_len(cols: usize, win_size: usize, state_len: *mut usize) -> c_int;
    fn ss_cmvn_stream_packed(vec: *const f32, n_active: usize, row_offsets: *const i64, slots: *const i32, pool_streams: usize,
                             cols: usize, win_size: usize, variance_normalization: c_int, pool: *mut f32, out: *mut f32) -> c_int;
    fn ss_cmvn_stats_len(cols: usize, len: *mut usize) -> c_int;
    fn ss_cmvn_stats_to_kaldi(stats: *const f64, cols: usize, kaldi: *mut f64) -> c_int;
    fn ss_cmvn_stats_from_kaldi(kaldi: *const f64, cols: usize, stats: *mut f64) -> c_int;
    fn ss_cmvn_stats_packed(vec: *const f32, n_clips: usize, offsets: *const i64, total_rows: usize, cols: usize,
                            clip_group: *const i32, n_groups: usize, stats: *mut f64) -> c_int;
    fn ss_cmvn_apply_packed(vec: *const f32, n_clips: usize, offsets: *const i64, total_rows: usize, cols: usize,
                            clip_group: *const i32, n_groups: usize, stats: *const f64, variance_normalization: c_int,
                            out: *mut f32) -> c_int;
    fn ss_cmvn_grouped_packed(vec: *const f32, n_clips: usize, offsets: *const i64, total_rows: usize, cols: usize,
                              clip_group: *const i32, n_groups: usize, variance_normalization: c_int, out: *mut f32) -> c_int;
    fn ss_add_deltas_packed(vec: *const f32, n_clips: usize, offsets: *const i64, total_rows: usize, cols: usize, order: usize,
                            window: usize, out: *mut f32) -> c_int;
    fn ss_add_deltas_stream_state_len(cols: usize, order: usize, window: usize, state_len: *mut usize) -> c_int;
    fn ss_add_deltas_stream_packed(vec: *const f32, n_active: usize, row_offsets: *const i64, slots: *const i32, pool_streams: usize,
                                   cols: usize, order: usize, window: usize, pool: *mut f32, out: *mut f32) -> c_int;
    fn ss_add_deltas_stream_flush(n_active: usize, slots: *const i32, pool_streams: usize, cols: usize, order: usize, window: usize,
                                  pool: *mut f32, out: *mut f32) -> c_int;
    fn ss_vad_energy_packed_device(d_vec: *const f32, n_clips: usize, d_offsets: *const i64, total_rows: usize, cols: usize,
                                   energy_col: usize, energy_threshold: f32, energy_mean_scale: f32, frames_context: usize,
                                   proportion_threshold: f32, d_mask: *mut u8, d_counts: *mut i64, stream: *mut c_void) -> c_int;
    fn ss_vad_energy_packed(vec: *const f32, n_clips: usize, offsets: *const i64, total_rows: usize, cols: usize, energy_col: usize,
                            energy_threshold: f32, energy_mean_scale: f32, frames_context: usize, proportion_threshold: f32,
                            mask: *mut u8, counts: *mut i64) -> c_int;
    fn ss_select_rows_packed_device(d_vec: *const f32, n_clips: usize, d_row_offsets: *const i64, total_rows: usize, cols: usize,
                                    d_mask: *const u8, d_out_offsets: *mut i64, d_out: *mut f32, stream: *mut c_void) -> c_int;
    fn ss_select_rows_packed(vec: *const f32, n_clips: usize, row_offsets: *const i64, total_rows: usize, cols: usize,
                             mask: *const u8, out_offsets: *mut i64, out: *mut f32) -> c_int;
    fn ss_vad_energy_stream_state_len(frames_context: usize, state_len: *mut usize) -> c_int;
    fn ss_vad_energy_stream_packed_device(d_vec: *const f32, n_active: usize, d_row_offsets: *const i64, total_rows: usize,
                                          d_slots: *const i32, pool_streams: usize, cols: usize, energy_col: usize,
                                          energy_threshold: f32, energy_mean_scale: f32, frames_context: usize,
                                          proportion_threshold: f32, d_pool: *mut f32, d_mask: *mut u8, stream: *mut c_void) -> c_int;
    fn ss_vad_energy_stream_packed(vec: *const f32, n_active: usize, row_offsets: *const i64, slots: *const i32, pool_streams: usize,
                                   cols: usize, energy_col: usize, energy_threshold: f32, energy_mean_scale: f32,
                                   frames_context: usize, proportion_threshold: f32, pool: *mut f32, mask: *mut u8) -> c_int;
    fn ss_vad_energy_stream_flush_device(n_active: usize, d_slots: *const i32, pool_streams: usize, energy_threshold: f32,
                                         energy_mean_scale: f32, frames_context: usize, proportion_threshold: f32, d_pool: *mut f32,
                                         d_mask: *mut u8, stream: *mut c_void) -> c_int;
    fn ss_vad_energy_stream_flush(n_active: usize, slots: *const i32, pool_streams: usize, energy_threshold: f32,
                                  energy_mean_scale: f32, frames_context: usize, proportion_threshold: f32, pool: *mut f32,
                                  mask: *mut u8) -> c_int;
    fn ss_pad_packed_out_bytes(n_clips: usize, max_rows: usize, cols: usize, dtype: c_int, bytes: *mut usize) -> c_int;
    fn ss_pad_packed_device(d_vec: *const f32, n_clips: usize, d_row_offsets: *const i64, total_rows: usize, cols: usize, max_rows: usize,
                            layout: c_int, dtype: c_int, pad_value: f32, d_out: *mut c_void, d_lengths: *mut i32,
                            stream: *mut c_void) -> c_int;
    fn ss_pad_packed(vec: *const f32, n_clips: usize, row_offsets: *const i64, total_rows: usize, cols: usize, max_rows: usize,
                     layout: c_int, dtype: c_int, pad_value: f32, out: *mut c_void, lengths: *mut i32) -> c_int;
    fn ss_specaug_spans(rng: *const u64, clip_base: usize, n_clips: usize, row_offsets: *const i64, total_rows: usize, cols: usize, n_time: usize,
                        max_time_width: usize, time_ratio: f32, n_freq: usize, max_freq_width: usize, spans: *mut i32) -> c_int;
    fn ss_specaug_plan_packed_device(d_rng: *const u64, clip_base: usize, n_clips: usize, d_row_offsets: *const i64, total_rows: usize, cols: usize,
                                     n_time: usize, max_time_width: usize, time_ratio: f32, n_freq: usize, max_freq_width: usize,
                                     d_spans: *mut i32, stream: *mut c_void) -> c_int;
    fn ss_mask_spans_packed_device(d_vec: *const f32, n_clips: usize, d_row_offsets: *const i64, total_rows: usize, cols: usize,
                                   d_spans: *const i32, n_time: usize, n_freq: usize, mask_value: f32, d_out: *mut f32,
                                   stream: *mut c_void) -> c_int;
    fn ss_mask_spans_packed(vec: *const f32, n_clips: usize, row_offsets: *const i64, total_rows: usize, cols: usize, spans: *const i32,
                            n_time: usize, n_freq: usize, mask_value: f32, out: *mut f32) -> c_int;
    fn ss_specaug_packed_device(d_vec: *const f32, n_clips: usize, d_row_offsets: *const i64, total_rows: usize, cols: usize, d_rng: *mut u64,
                                clip_base: usize, n_time: usize, max_time_width: usize, time_ratio: f32, n_freq: usize, max_freq_width: usize,
                                mask_value: f32, d_out: *mut f32, d_spans: *mut i32, stream: *mut c_void) -> c_int;
    fn ss_specaug_packed(vec: *const f32, n_clips: usize, row_offsets: *const i64, total_rows: usize, cols: usize, rng: *mut u64,
                         clip_base: usize, n_time: usize, max_time_width: usize, time_ratio: f32, n_freq: usize, max_freq_width: usize,
                         mask_value: f32, out: *mut f32, spans: *mut i32) -> c_int;
    fn ss_noise_draws(rng: *const u64, clip_base: usize, n_clips: usize, sample_offsets: *const i64, total_samples: usize, n_noise: usize,
                      noise_offsets: *const i64, total_noise: usize, prob: f32, snr_lo_db: f32, snr_hi_db: f32, gain_lo_db: f32, gain_hi_db: f32,
                      plan: *mut NoisePlanRow) -> c_int;
    fn ss_noise_mix_work_bytes(n_clips: usize, total_samples: usize, bytes: *mut usize) -> c_int;
    fn ss_noise_plan_packed_device(d_x: *const f32, n_clips: usize, d_sample_offsets: *const i64, total_samples: usize, d_bank: *const f32,
                                   n_noise: usize, d_noise_offsets: *const i64, total_noise: usize, d_rng: *const u64, clip_base: usize, prob: f32,
                                   snr_lo_db: f32, snr_hi_db: f32, gain_lo_db: f32, gain_hi_db: f32, d_plan: *mut NoisePlanRow, d_work: *mut c_void,
                                   work_bytes: usize, stream: *mut c_void) -> c_int;
    fn ss_noise_plan_packed_i16_device(d_x: *const i16, x_scale: f32, n_clips: usize, d_sample_offsets: *const i64, total_samples: usize,
                                       d_bank: *const i16, noise_scale: f32, n_noise: usize, d_noise_offsets: *const i64, total_noise: usize,
                                       d_rng: *const u64, clip_base: usize, prob: f32, snr_lo_db: f32, snr_hi_db: f32, gain_lo_db: f32,
                                       gain_hi_db: f32, d_plan: *mut NoisePlanRow, d_work: *mut c_void, work_bytes: usize,
                                       stream: *mut c_void) -> c_int;
    fn ss_noise_apply_packed_device(d_x: *const f32, n_clips: usize, d_sample_offsets: *const i64, total_samples: usize, d_bank: *const f32,
                                    n_noise: usize, d_noise_offsets: *const i64, total_noise: usize, d_plan: *const NoisePlanRow, d_out: *mut f32,
                                    stream: *mut c_void) -> c_int;
    fn ss_noise_apply_packed(x: *const f32, n_clips: usize, sample_offsets: *const i64, total_samples: usize, bank: *const f32, n_noise: usize,
                             noise_offsets: *const i64, total_noise: usize, plan: *const NoisePlanRow, out: *mut f32) -> c_int;
    fn ss_noise_apply_packed_i16_device(d_x: *const i16, x_scale: f32, n_clips: usize, d_sample_offsets: *const i64, total_samples: usize,
                                        d_bank: *const i16, noise_scale: f32, n_noise: usize, d_noise_offsets: *const i64, total_noise: usize,
                                        d_plan: *const NoisePlanRow, d_out: *mut f32, stream: *mut c_void) -> c_int;
    fn ss_noise_apply_packed_i16(x: *const i16, x_scale: f32, n_clips: usize, sample_offsets: *const i64, total_samples: usize, bank: *const i16,
                                 noise_scale: f32, n_noise: usize, noise_offsets: *const i64, total_noise: usize, plan: *const NoisePlanRow,
                                 out: *mut f32) -> c_int;
    fn ss_noise_mix_packed_device(d_x: *const f32, n_clips: usize, d_sample_offsets: *const i64, total_samples: usize, d_bank: *const f32,
                                  n_noise: usize, d_noise_offsets: *const i64, total_noise: usize, d_rng: *mut u64, clip_base: usize, prob: f32,
                                  snr_lo_db: f32, snr_hi_db: f32, gain_lo_db: f32, gain_hi_db: f32, d_out: *mut f32, d_plan: *mut NoisePlanRow,
                                  d_work: *mut c_void, work_bytes: usize, stream: *mut c_void) -> c_int;
    fn ss_noise_mix_packed(x: *const f32, n_clips: usize, sample_offsets: *const i64, total_samples: usize, bank: *const f32, n_noise: usize,
                           noise_offsets: *const i64, total_noise: usize, rng: *mut u64, clip_base: usize, prob: f32, snr_lo_db: f32,
                           snr_hi_db: f32, gain_lo_db: f32, gain_hi_db: f32, out: *mut f32, plan: *mut NoisePlanRow) -> c_int;
    fn ss_noise_mix_packed_i16_device(d_x: *const i16, x_scale: f32, n_clips: usize, d_sample_offsets: *const i64, total_samples: usize,
                                      d_bank: *const i16, noise_scale: f32, n_noise: usize, d_noise_offsets: *const i64, total_noise: usize,
                                      d_rng: *mut u64, clip_base: usize, prob: f32, snr_lo_db: f32, snr_hi_db: f32, gain_lo_db: f32,
                                      gain_hi_db: f32, d_out: *mut f32, d_plan: *mut NoisePlanRow, d_work: *mut c_void, work_bytes: usize,
                                      stream: *mut c_void) -> c_int;
    fn ss_noise_mix_packed_i16(x: *const i16, x_scale: f32, n_clips: usize, sample_offsets: *const i64, total_samples: usize, bank: *const i16,
                               noise_scale: f32, n_noise: usize, noise_offsets: *const i64, total_noise: usize, rng: *mut u64, clip_base: usize,
                               prob: f32, snr_lo_db: f32, snr_hi_db: f32, gain_lo_db: f32, gain_hi_db: f32, out: *mut f32,
                               plan: *mut NoisePlanRow) -> c_int;
    fn ss_reverb_bank_create(rir: *const f32, n_rir: usize, rir_offsets: *const i64, total_rir: usize, normalize: c_int, align_peak: c_int,
                             bank: *mut *mut c_void) -> c_int;
    fn ss_reverb_bank_destroy(bank: *mut c_void);
    fn ss_reverb_bank_info(bank: *const c_void, n_rir: *mut usize, block: *mut usize, max_taps: *mut usize, n_partitions: *mut usize) -> c_int;
    fn ss_reverb_bank_rir(bank: *const c_void, c: usize, taps: *mut f32, cap: usize, n_taps: *mut usize, peak: *mut usize) -> c_int;
    fn ss_reverb_bank_spectrum(bank: *const c_void, c: usize, p: usize, out: *mut f32) -> c_int;
    fn ss_reverb_draws(rng: *const u64, clip_base: usize, n_clips: usize, sample_offsets: *const i64, total_samples: usize, bank: *const c_void,
                       prob: f32, plan: *mut ReverbPlanRow) -> c_int;
    fn ss_reverb_plan_packed_device(n_clips: usize, d_sample_offsets: *const i64, total_samples: usize, bank: *const c_void, d_rng: *const u64,
                                    clip_base: usize, prob: f32, d_plan: *mut ReverbPlanRow, stream: *mut c_void) -> c_int;
    fn ss_reverb_apply_packed_device(d_x: *const f32, n_clips: usize, d_sample_offsets: *const i64, total_samples: usize, bank: *const c_void,
                                     d_plan: *const ReverbPlanRow, d_out: *mut f32, stream: *mut c_void) -> c_int;
    fn ss_reverb_apply_packed(x: *const f32, n_clips: usize, sample_offsets: *const i64, total_samples: usize, bank: *const c_void,
                              plan: *const ReverbPlanRow, out: *mut f32) -> c_int;
    fn ss_reverb_apply_packed_i16_device(d_x: *const i16, x_scale: f32, n_clips: usize, d_sample_offsets: *const i64, total_samples: usize,
                                         bank: *const c_void, d_plan: *const ReverbPlanRow, d_out: *mut f32, stream: *mut c_void) -> c_int;
    fn ss_reverb_apply_packed_i16(x: *const i16, x_scale: f32, n_clips: usize, sample_offsets: *const i64, total_samples: usize,
                                  bank: *const c_void, plan: *const ReverbPlanRow, out: *mut f32) -> c_int;
    fn ss_reverb_packed_device(d_x: *const f32, n_clips: usize, d_sample_offsets: *const i64, total_samples: usize, bank: *const c_void,
                               d_rng: *mut u64, clip_base: usize, prob: f32, d_out: *mut f32, d_plan: *mut ReverbPlanRow,
                               stream: *mut c_void) -> c_int;
    fn ss_reverb_packed(x: *const f32, n_clips: usize, sample_offsets: *const i64, total_samples: usize, bank: *const c_void, rng: *mut u64,
                        clip_base: usize, prob: f32, out: *mut f32, plan: *mut ReverbPlanRow) -> c_int;
    fn ss_reverb_packed_i16_device(d_x: *const i16, x_scale: f32, n_clips: usize, d_sample_offsets: *const i64, total_samples: usize,
                                   bank: *const c_void, d_rng: *mut u64, clip_base: usize, prob: f32, d_out: *mut f32,
                                   d_plan: *mut ReverbPlanRow, stream: *mut c_void) -> c_int;
    fn ss_reverb_packed_i16(x: *const i16, x_scale: f32, n_clips: usize, sample_offsets: *const i64, total_samples: usize, bank: *const c_void,
                            rng: *mut u64, clip_base: usize, prob: f32, out: *mut f32, plan: *mut ReverbPlanRow) -> c_int;
    fn ss_resample_packed_offsets(orig_rate: u32, new_rate: u32, n_clips: usize, sample_offsets: *const i64, out_offsets: *mut i64) -> c_int;
    fn ss_resampler_create(orig_rate: u32, new_rate: u32, lowpass_filter_width: u32, rolloff: f32, out: *mut *mut c_void) -> c_int;
    fn ss_resampler_destroy(rs: *mut c_void);
    fn ss_resampler_info(rs: *const c_void, info: *mut ResampleInfo) -> c_int;
    fn ss_resample(rs: *const c_void, x: *const f32, batch: usize, n_samples: usize, ld: usize, out: *mut f32, ld_out: usize) -> c_int;
    fn ss_resample_packed(rs: *const c_void, x: *const f32, n_clips: usize, sample_offsets: *const i64, out_offsets: *const i64,
                          out: *mut f32) -> c_int;
    fn ss_resample_packed_i16(rs: *const c_void, x: *const i16, n_clips: usize, sample_offsets: *const i64, scale: f32,
                              out_offsets: *const i64, out: *mut f32) -> c_int;
    fn ss_resample_stream_state_len(rs: *const c_void, state_len: *mut usize) -> c_int;
    fn ss_resample_stream_packed(rs: *const c_void, x: *const f32, n_active: usize, sample_offsets: *const i64, slots: *const i32,
                                 pool_streams: usize, pool: *mut f32, out: *mut f32) -> c_int;
    fn ss_resample_stream_flush(rs: *const c_void, n_active: usize, slots: *const i32, pool_streams: usize, pool: *mut f32,
                                out: *mut f32) -> c_int;
    fn ss_affine_create(matrix: *const f32, out_dim: usize, in_dim: usize, ld: usize, bias_or_null: *const f32, out: *mut *mut c_void) -> c_int;
    fn ss_affine_destroy(t: *mut c_void);
    fn ss_affine_dims(t: *const c_void, out_dim: *mut usize, in_dim: *mut usize) -> c_int;
    fn ss_affine_chain_len(in_dim: usize, k4: *mut usize) -> c_int;
    fn ss_affine_splice_packed_device(t: *const c_void, d_vec: *const f32, n_clips: usize, d_row_offsets: *const i64, total_rows: usize,
                                      d_out_offsets: *const i64, total_out_rows: usize, cols: usize, left: usize, right: usize, stride: usize,
                                      d_out: *mut f32, stream: *mut c_void) -> c_int;
    fn ss_affine_splice_packed(t: *const c_void, vec: *const f32, n_clips: usize, row_offsets: *const i64, total_rows: usize, cols: usize,
                               left: usize, right: usize, stride: usize, out: *mut f32) -> c_int;
    fn ss_kaldi_params_default(p: *mut KaldiParams, sample_rate: u32) -> c_int;
    fn ss_kaldi_num_frames(p: *const KaldiParams, n_samples: usize, n_frames: *mut usize) -> c_int;
    fn ss_kaldi_packed_frame_offsets(p: *const KaldiParams, n_clips: usize, sample_offsets: *const i64, frame_offsets: *mut i64) -> c_int;
    fn ss_kaldi_config_create(p: *const KaldiParams, out: *mut *mut c_void) -> c_int;
    fn ss_kaldi_config_destroy(cfg: *mut c_void);
    fn ss_kaldi_fbank(cfg: *const c_void, x: *const f32, batch: usize, n_samples: usize, ld: usize, out: *mut f32, log_energy: *mut f32) -> c_int;
    fn ss_kaldi_mfcc(cfg: *const c_void, x: *const f32, batch: usize, n_samples: usize, ld: usize, out: *mut f32) -> c_int;
    fn ss_kaldi_fbank_packed(cfg: *const c_void, x: *const f32, n_clips: usize, sample_offsets: *const i64, out: *mut f32,
                             log_energy: *mut f32) -> c_int;
    fn ss_kaldi_mfcc_packed(cfg: *const c_void, x: *const f32, n_clips: usize, sample_offsets: *const i64, out: *mut f32) -> c_int;
    fn ss_kstream_state_len(p: *const KaldiParams, state_len: *mut usize, delay_rows: *mut usize) -> c_int;
    fn ss_kstream_row_offsets(p: *const KaldiParams, n_active: usize, sample_offsets: *const i64, row_offsets: *mut i64) -> c_int;
    fn ss_kstream_fbank_packed(cfg: *const c_void, x: *const f32, n_active: usize, sample_offsets: *const i64, slots: *const i32,
                               pool_streams: usize, pool: *mut f32, out: *mut f32, log_energy: *mut f32) -> c_int;
    fn ss_kstream_mfcc_packed(cfg: *const c_void, x: *const f32, n_active: usize, sample_offsets: *const i64, slots: *const i32,
                              pool_streams: usize, pool: *mut f32, out: *mut f32) -> c_int;
    fn ss_kstream_fbank_packed_i16(cfg: *const c_void, x: *const i16, n_active: usize, sample_offsets: *const i64, slots: *const i32,
                                   pool_streams: usize, scale: f32, pool: *mut f32, out: *mut f32, log_energy: *mut f32) -> c_int;
    fn ss_kstream_mfcc_packed_i16(cfg: *const c_void, x: *const i16, n_active: usize, sample_offsets: *const i64, slots: *const i32,
                                  pool_streams: usize, scale: f32, pool: *mut f32, out: *mut f32) -> c_int;
    fn ss_whisper_params_default(p: *mut SsWhisperParams, n_mels: u32) -> c_int;
    fn ss_whisper_num_frames(n_samples: usize, n_frames: *mut usize) -> c_int;
    fn ss_whisper_work_bytes(p: *const SsWhisperParams, batch: usize, n_frames: usize, dtype: c_int, bytes: *mut usize) -> c_int;
    fn ss_whisper_config_create(p: *const SsWhisperParams, out: *mut *mut c_void) -> c_int;
    fn ss_whisper_config_destroy(cfg: *mut c_void);
    fn ss_whisper_config_device_status(cfg: *const c_void) -> c_int;
    fn ss_whisper_log_mel_device(cfg: *const c_void, d_x: *const f32, batch: usize, n_samples: usize, ld: usize, n_frames: usize, dtype: c_int,
                                 d_work: *mut c_void, d_out: *mut c_void, stream: *mut c_void) -> c_int;
    fn ss_whisper_log_mel(cfg: *const c_void, x: *const f32, batch: usize, n_samples: usize, ld: usize, n_frames: usize, dtype: c_int,
                          out: *mut c_void) -> c_int;
    fn ss_whisper_log_mel_packed_device(cfg: *const c_void, d_x: *const f32, n_clips: usize, d_sample_offsets: *const i64, n_frames: usize,
                                        dtype: c_int, d_work: *mut c_void, d_out: *mut c_void, d_lengths: *mut i32, stream: *mut c_void) -> c_int;
    fn ss_whisper_log_mel_packed(cfg: *const c_void, x: *const f32, n_clips: usize, sample_offsets: *const i64, n_frames: usize, dtype: c_int,
                                 out: *mut c_void, lengths: *mut i32) -> c_int;
    fn ss_nemo_params_default(p: *mut SsNemoParams, n_mels: u32) -> c_int;
    fn ss_nemo_num_frames(p: *const SsNemoParams, n_samples: usize, n_frames: *mut usize) -> c_int;
    fn ss_nemo_packed_frame_offsets(p: *const SsNemoParams, n_clips: usize, sample_offsets: *const i64, frame_offsets: *mut i64) -> c_int;
    fn ss_nemo_config_create(p: *const SsNemoParams, out: *mut *mut c_void) -> c_int;
    fn ss_nemo_config_destroy(cfg: *mut c_void);
    fn ss_nemo_config_device_status(cfg: *const c_void) -> c_int;
    fn ss_nemo_log_mel_device(cfg: *const c_void, d_x: *const f32, batch: usize, n_samples: usize, ld: usize, d_out: *mut f32,
                              stream: *mut c_void) -> c_int;
    fn ss_nemo_log_mel(cfg: *const c_void, x: *const f32, batch: usize, n_samples: usize, ld: usize, out: *mut f32) -> c_int;
    fn ss_nemo_log_mel_packed_device(cfg: *const c_void, d_x: *const f32, n_clips: usize, d_sample_offsets: *const i64,
                                     d_frame_offsets: *const i64, total_frames: usize, d_out: *mut f32, stream: *mut c_void) -> c_int;
    fn ss_nemo_log_mel_packed(cfg: *const c_void, x: *const f32, n_clips: usize, sample_offsets: *const i64, out: *mut f32) -> c_int;
    fn ss_nstream_state_len(p: *const SsNemoParams, state_len: *mut usize, delay_rows: *mut usize) -> c_int;
    fn ss_nstream_row_offsets(p: *const SsNemoParams, n_active: usize, sample_offsets: *const i64, row_offsets: *mut i64) -> c_int;
    fn ss_nstream_log_mel_packed(cfg: *const c_void, x: *const f32, n_active: usize, sample_offsets: *const i64, slots: *const i32,
                                 pool_streams: usize, pool: *mut f32, out: *mut f32) -> c_int;
    fn ss_nstream_log_mel_packed_i16(cfg: *const c_void, x: *const i16, n_active: usize, sample_offsets: *const i64, slots: *const i32,
                                     pool_streams: usize, scale: f32, pool: *mut f32, out: *mut f32) -> c_int;
    fn ss_nstream_flush(cfg: *const c_void, n_active: usize, slots: *const i32, pool_streams: usize, pool: *mut f32, out: *mut f32) -> c_int;
    fn ss_derivative_extraction(feat: *const f32, rows: usize, cols: usize, delta_windows: usize, out: *mut f32) -> c_int;
    fn ss_extract_derivative_feature(feat: *const f32, rows: usize, cols: usize, cube: *mut f32) -> c_int;
    fn ss_shard_bounds(n_items: usize, world: c_int, rank: c_int, lo: *mut usize, hi: *mut usize) -> c_int;
    fn ss_all_gather_features(nccl_comm: *mut c_void, d_block: *const f32, elems_per_rank: usize, d_out: *mut f32,
                              stream: *mut c_void) -> c_int;
    fn ss_gather_features(nccl_comm: *mut c_void, d_block: *const f32, elems_per_rank: usize, d_out: *mut f32, root: c_int,
                          rank: c_int, world: c_int, stream: *mut c_void) -> c_int;
    fn ss_last_error_string() -> *const c_char;
}

/// Contiguous clip shard of rank `rank` of `world` (one process or thread per GPU; clips are independent units).
pub fn shard_bounds(n_items: usize, world: usize, rank: usize) -> (usize, usize) {
    let (mut lo, mut hi) = (0usize, 0usize);
    check(unsafe { ss_shard_bounds(n_items, world as c_int, rank as c_int, &mut lo, &mut hi) }).expect("shard_bounds");
    (lo, hi)
}

/// RCCL all-gather of the ranks' feature blocks (device pointers, `comm` = the caller's ncclComm_t): the north-star's
/// "gather over xGMI of the final [n_frames x n_mfcc] blocks".
///
/// # Safety
/// `d_block` / `d_out` must be device buffers of `elems_per_rank` / `world * elems_per_rank` floats on the current device.
pub unsafe fn all_gather_features(comm: *mut c_void, d_block: *const f32, elems_per_rank: usize, d_out: *mut f32,
                                  stream: *mut c_void) -> Result<(), Error> {
    check(ss_all_gather_features(comm, d_block, elems_per_rank, d_out, stream))
}

/// RCCL gather to `root` (the north-star's collective): the root receives `[world x elems_per_rank]` in rank order, one
/// direct xGMI transfer per peer; the other ranks only send and may pass a null `d_out`.
///
/// # Safety
/// As `all_gather_features`; `comm` must come from the RCCL library this crate's C side resolves (see speechsauce_amd.h).
#[allow(clippy::too_many_arguments)]
pub unsafe fn gather_features(comm: *mut c_void, d_block: *const f32, elems_per_rank: usize, d_out: *mut f32, root: usize,
                              rank: usize, world: usize, stream: *mut c_void) -> Result<(), Error> {
    check(ss_gather_features(comm, d_block, elems_per_rank, d_out, root as c_int, rank as c_int, world as c_int, stream))
}

/// SS_ERR_ARG of include/speechsauce_amd.h
pub const SS_ERR_ARG: i32 = 3;

#[derive(Debug)]
pub struct Error {
    pub status: i32,
    pub detail: String,
}

fn check(status: c_int) -> Result<(), Error> {
    if status == 0 {
        return Ok(());
    }
    let detail = unsafe { CStr::from_ptr(ss_last_error_string()) }.to_string_lossy().into_owned();
    Err(Error { status, detail })
}

/// config.rs:10-97
#[derive(Clone)]
pub struct SpeechConfigBuilder {
    p: SsParams,
}
impl Default for SpeechConfigBuilder {
    /// config.rs:10 derives Default (every field zero); `SpeechConfig::builder()` hands that out (config.rs:187-189)
    fn default() -> Self {
        let mut b = SpeechConfigBuilder::new(16000);  // (the switches of ss_params keep their reference-mode defaults)
        b.p.sample_rate = 0;
        b.p.fft_points = 0;
        b.p.frame_length = 0.0;
        b.p.frame_stride = 0.0;
        b.p.num_cepstral = 0;
        b.p.num_filters = 0;
        b.p.high_frequency = 0.0;
        b.p.dc_elimination = 0;
        b
    }
}

impl SpeechConfigBuilder {
    pub fn new(sample_rate: usize) -> Self {
        let mut p = std::mem::MaybeUninit::<SsParams>::uninit();
        unsafe {
            check(ss_params_default(p.as_mut_ptr(), sample_rate as u32)).expect("ss_params_default");
            SpeechConfigBuilder { p: p.assume_init() }
        }
    }
    pub fn high_freq(mut self, v: f32) -> Self { self.p.high_frequency = v; self }
    pub fn low_freq(mut self, v: f32) -> Self { self.p.low_frequency = v; self }
    pub fn dc_elimination(mut self, v: bool) -> Self { self.p.dc_elimination = v as i32; self }
    pub fn num_cepstral(mut self, v: usize) -> Self { self.p.num_cepstral = v as u32; self }
    pub fn frame_stride(mut self, v: f32) -> Self { self.p.frame_stride = v; self }
    pub fn frame_length(mut self, v: f32) -> Self { self.p.frame_length = v; self }
    pub fn fft_points(mut self, v: usize) -> Self { self.p.fft_points = v as u32; self }
    pub fn build(self) -> SpeechConfig { SpeechConfig::from_params(self.p).expect("SpeechConfig::new") }
}

/// The device-side half of a config: the opaque handle of include/speechsauce_amd.h, destroyed with the last clone.
struct Handle(*mut SsConfig);
// the handle is immutable after creation and safe for concurrent calls (speechsauce_amd.h, "Threading")
unsafe impl Send for Handle {}
unsafe impl Sync for Handle {}
impl Drop for Handle {
    fn drop(&mut self) { unsafe { ss_config_destroy(self.0) } }
}

/// config.rs:98-131.  Immutable after creation (no STFT carry-over), hence Send + Sync; `Clone` shares the device handle.
#[derive(Clone)]
pub struct SpeechConfig {
    pub sample_rate: usize,
    pub window_size: usize,
    pub window_size_half: usize,
    pub frame_length: f32,
    pub frame_stride: f32,
    pub num_cepstral: usize,
    pub num_filters: usize,
    pub low_frequency: f32,
    pub high_frequency: f32,
    pub freq_size: usize,
    /// samples per STFT chunk = trunc(frame_length * sample_rate) (config.rs:154), as the library computes it
    pub frame_size: usize,
    pub dc_elimination: bool,
    /// 2 * frame_size / fft_points^2 (config.rs:178)
    pub wnorm: f32,
    /// the Vorbis power-complementary window of `window_size` points (config.rs:151-160)
    pub window: Vec<f32>,
    params: SsParams,
    handle: Arc<Handle>,
}

impl SpeechConfig {
    /// config.rs:140-150
    #[allow(clippy::too_many_arguments)]
    pub fn new(sample_rate: usize, fft_points: usize, frame_length: f32, frame_stride: f32, num_cepstral: usize,
               num_filters: usize, low_frequency: f32, high_frequency: f32, dc_elimination: bool) -> Self {
        let mut b = SpeechConfigBuilder::new(sample_rate).p;
        b.fft_points = fft_points as u32;
        b.frame_length = frame_length;
        b.frame_stride = frame_stride;
        b.num_cepstral = num_cepstral as u32;
        b.num_filters = num_filters as u32;
        b.low_frequency = low_frequency;
        b.high_frequency = high_frequency;
        b.dc_elimination = dc_elimination as i32;
        Self::from_params(b).expect("SpeechConfig::new")
    }
    pub fn from_params(p: SsParams) -> Result<Self, Error> {
        let mut h: *mut SsConfig = std::ptr::null_mut();
        check(unsafe { ss_config_create(&p, &mut h) })?;
        let handle = Arc::new(Handle(h));  // from here on an early return releases the handle
        // config.rs:154 / :178 in the reference's own f32 arithmetic (every config has these two, not only the STFT-capable
        // ones ss_stft_sizes answers for; for those the library's values are the same numbers)
        let frame_size = (p.frame_length * p.sample_rate as f32) as usize;
        let wnorm = 1.0 / ((p.fft_points as usize).pow(2) as f32 / (2 * frame_size) as f32);
        let mut window = vec![0f32; p.fft_points as usize];
        check(unsafe { ss_vorbis_window(window.len(), window.as_mut_ptr()) })?;
        Ok(SpeechConfig {
            sample_rate: p.sample_rate as usize,
            window_size: p.fft_points as usize,
            window_size_half: p.fft_points as usize / 2,
            frame_size,
            wnorm,
            window,
            frame_length: p.frame_length,
            frame_stride: p.frame_stride,
            num_cepstral: p.num_cepstral as usize,
            num_filters: p.num_filters as usize,
            low_frequency: p.low_frequency,
            high_frequency: p.high_frequency,
            freq_size: p.fft_points as usize / 2 + 1,
            dc_elimination: p.dc_elimination != 0,
            params: p,
            handle,
        })
    }
    /// config.rs:187-189: the all-zero builder (set every field before `build()`, as with the reference)
    pub fn builder() -> SpeechConfigBuilder { SpeechConfigBuilder::default() }
}
impl Default for SpeechConfig {
    fn default() -> Self { SpeechConfigBuilder::new(16000).build() }
}
impl SpeechConfig {
    /// the raw handle for the `extern "C"` calls below (valid while any clone lives)
    fn raw(&self) -> *const SsConfig { self.handle.0 }
}

/// The samples of a 1-D view as one contiguous run: borrowed when the view already is one, copied otherwise (the reference accepts
/// any stride, `as_array()`).  `ArrayView::to_slice(&self) -> Option<&'a [A]>` hands out the VIEW's lifetime; `ArrayBase::as_slice`
/// would borrow from the by-value parameter, a local (E0515).
fn contiguous<'a>(signal: ArrayView1<'a, f32>) -> std::borrow::Cow<'a, [f32]> {
    match signal.to_slice() {
        Some(s) => std::borrow::Cow::Borrowed(s),
        None => std::borrow::Cow::Owned(signal.to_vec()),
    }
}

/// feature.rs:99-148
pub fn try_mfcc(signal: ArrayView1<f32>, cfg: &SpeechConfig) -> Result<Array2<f32>, Error> {
    let x = contiguous(signal);
    let mut t = 0usize;
    check(unsafe { ss_num_frames(&cfg.params, x.len(), &mut t) })?;
    let mut out = Array2::<f32>::zeros((t, cfg.num_cepstral));
    check(unsafe { ss_mfcc(cfg.raw(), x.as_ptr(), x.len(), out.as_mut_ptr()) })?;
    Ok(out)
}
pub fn mfcc(signal: ArrayView1<f32>, cfg: &SpeechConfig) -> Array2<f32> { try_mfcc(signal, cfg).expect("mfcc") }

/// feature.rs:200-233
pub fn try_mfe(signal: ArrayView1<f32>, cfg: &SpeechConfig) -> Result<(Array2<f32>, Array1<f32>), Error> {
    let x = contiguous(signal);
    let mut t = 0usize;
    check(unsafe { ss_num_frames(&cfg.params, x.len(), &mut t) })?;
    let mut feat = Array2::<f32>::zeros((t, cfg.num_filters));
    let mut en = Array1::<f32>::zeros(t);
    check(unsafe { ss_mfe(cfg.raw(), x.as_ptr(), x.len(), feat.as_mut_ptr(), en.as_mut_ptr()) })?;
    Ok((feat, en))
}
pub fn mfe(signal: ArrayView1<f32>, cfg: &SpeechConfig) -> (Array2<f32>, Array1<f32>) { try_mfe(signal, cfg).expect("mfe") }

/// feature.rs:242-245 (private there; README.md:14 lists log mel-filterbank energies as a supported feature)
pub fn try_lmfe(signal: ArrayView1<f32>, cfg: &SpeechConfig) -> Result<Array2<f32>, Error> {
    let x = contiguous(signal);
    let mut t = 0usize;
    check(unsafe { ss_num_frames(&cfg.params, x.len(), &mut t) })?;
    let mut feat = Array2::<f32>::zeros((t, cfg.num_filters));
    check(unsafe { ss_lmfe(cfg.raw(), x.as_ptr(), x.len(), feat.as_mut_ptr()) })?;
    Ok(feat)
}
pub fn lmfe(signal: ArrayView1<f32>, cfg: &SpeechConfig) -> Array2<f32> { try_lmfe(signal, cfg).expect("lmfe") }

/// feature.rs:163-174: [channels, samples] -> [channels, n_mels, rows]; rows need contiguous storage like
/// the reference's `as_slice().expect(..)` (functions.rs:104)
pub fn try_mel_spectrogram2(signal: ArrayView2<f32>, cfg: &SpeechConfig) -> Result<Array3<f32>, Error> {
    let owned = signal.as_standard_layout();
    let (ch, n) = owned.dim();
    let (mut rows, mut _real) = (0usize, 0usize);
    check(unsafe { ss_stft_rows(&cfg.params, n, &mut rows, &mut _real) })?;
    let mut out = Array3::<f32>::zeros((ch, cfg.num_filters, rows));
    check(unsafe { ss_mel_spectrogram(cfg.raw(), owned.as_ptr(), ch, n, out.as_mut_ptr()) })?;
    Ok(out)
}
pub fn mel_spectrogram2(signal: ArrayView2<f32>, cfg: &SpeechConfig) -> Array3<f32> {
    try_mel_spectrogram2(signal, cfg).expect("mel_spectrogram2")
}
/// feature.rs:151-162 (one channel)
pub fn mel_spectrogram1(signal: ArrayView1<f32>, cfg: &SpeechConfig) -> Array2<f32> {
    let x = contiguous(signal);
    let v = ArrayView2::from_shape((1, x.len()), &x[..]).expect("shape");  // (&x[..]: a plain &[f32], no deref coercion of &Cow needed)
    let out = mel_spectrogram2(v, cfg);
    let (_, m, r) = out.dim();
    out.into_shape((m, r)).expect("shape")
}

/// Batch form with no counterpart in the reference: [batch, samples] -> [batch, frames, n_cepstral] in one launch.
pub fn try_mfcc_batch(signals: ArrayView2<f32>, cfg: &SpeechConfig) -> Result<Array3<f32>, Error> {
    let owned = signals.as_standard_layout();
    let (b, n) = owned.dim();
    let mut t = 0usize;
    check(unsafe { ss_num_frames(&cfg.params, n, &mut t) })?;
    let mut out = Array3::<f32>::zeros((b, t, cfg.num_cepstral));
    check(unsafe { ss_mfcc_batch(cfg.raw(), owned.as_ptr(), b, n, n, out.as_mut_ptr()) })?;
    Ok(out)
}

/// Device-resident batch: raw device pointers + a hipStream_t, asynchronous.
/// # Safety
/// `d_x` / `d_out` must be device allocations of the right size on the device the config was created on.
pub unsafe fn mfcc_batch_device(cfg: &SpeechConfig, d_x: *const f32, batch: usize, n: usize, ld: usize, d_out: *mut f32,
                                stream: *mut c_void) -> Result<(), Error> {
    check(ss_mfcc_batch_device(cfg.raw(), d_x, batch, n, ld, d_out, stream))
}

/// Several device-resident batches per call (ABI 7): batch `b` is `batch[b]` clips of `n` samples at `d_x[b]` (row stride `ld`), its
/// features go to `d_out[b]`.  One persistent launch for up to 8 batches where the configuration's kernel takes a batch table;
/// bit-identical to `batch.len()` calls of `mfcc_batch_device`.
/// # Safety
/// As `mfcc_batch_device`, for every batch.
pub unsafe fn mfcc_batches_device(cfg: &SpeechConfig, d_x: &[*const f32], batch: &[usize], n: usize, ld: usize, d_out: &[*mut f32],
                                  stream: *mut c_void) -> Result<(), Error> {
    if d_x.len() != batch.len() || d_out.len() != batch.len() {
        return Err(Error { status: SS_ERR_ARG, detail: "d_x, batch and d_out must have one entry per batch".to_string() });
    }
    check(ss_mfcc_batches_device(cfg.raw(), batch.len(), d_x.as_ptr(), batch.as_ptr(), n, ld, d_out.as_ptr(), stream))
}

/// Ragged streaming MFCC over a pool of stream states, fed signed 16-bit PCM (`ss_mfcc_stream_packed_i16_device`): entry `i` is
/// the chunk `d_x[so[i]..so[i + 1]]` (whole hops) of the stream whose state is row `d_slots[i]` of the `[pool_streams x S]` float
/// pool; stream sample = `pcm as f32 * scale`, `scale` a power of two in `[2^-64, 2^64]`.  Two asynchronous launches on `stream`.
/// # Safety
/// Every pointer is a device allocation of the size the header states, on the device the config was created on; `d_x` is 4-byte
/// aligned.
pub unsafe fn mfcc_stream_packed_i16_device(cfg: &SpeechConfig, d_x: *const i16, n_active: usize, d_sample_offsets: *const i64,
                                            d_row_offsets: *const i64, total_rows: usize, d_slots: *const i32, pool_streams: usize,
                                            scale: f32, norm_frames: u32, d_pool: *mut f32, d_out: *mut f32, stream: *mut c_void)
                                            -> Result<(), Error> {
    check(ss_mfcc_stream_packed_i16_device(cfg.raw(), d_x, n_active, d_sample_offsets, d_row_offsets, total_rows, d_slots, pool_streams,
                                           scale, norm_frames, d_pool, d_out, stream))
}

/// The mfe form of `mfcc_stream_packed_i16_device`: `d_feat` `[total_rows x num_filters]`, `d_energy` `[total_rows]`.
/// # Safety
/// As `mfcc_stream_packed_i16_device`.
pub unsafe fn mfe_stream_packed_i16_device(cfg: &SpeechConfig, d_x: *const i16, n_active: usize, d_sample_offsets: *const i64,
                                           d_row_offsets: *const i64, total_rows: usize, d_slots: *const i32, pool_streams: usize,
                                           scale: f32, d_pool: *mut f32, d_feat: *mut f32, d_energy: *mut f32, stream: *mut c_void)
                                           -> Result<(), Error> {
    check(ss_mfe_stream_packed_i16_device(cfg.raw(), d_x, n_active, d_sample_offsets, d_row_offsets, total_rows, d_slots, pool_streams,
                                          scale, d_pool, d_feat, d_energy, stream))
}

/// Host-pointer form of the PCM pool call: `x` the packed int16 chunks, `sample_offsets` `n_active + 1` offsets in samples, `slots`
/// the pool row of each entry, `pool` the `[pool_streams x S]` float states (updated in place), `out` `[rows x num_cepstral]` with
/// `rows = sample_offsets[n_active] / hop`.  Synchronous; the tables are checked before anything touches the device.
pub fn try_mfcc_stream_packed_i16(cfg: &SpeechConfig, x: &[i16], sample_offsets: &[i64], slots: &[i32], pool_streams: usize, scale: f32,
                                  norm_frames: u32, pool: &mut [f32], out: &mut [f32]) -> Result<(), Error> {
    if sample_offsets.len() != slots.len() + 1 {
        return Err(Error { status: SS_ERR_ARG, detail: "sample_offsets must have one entry more than slots".to_string() });
    }
    check(unsafe { ss_mfcc_stream_packed_i16(cfg.raw(), x.as_ptr(), slots.len(), sample_offsets.as_ptr(), slots.as_ptr(), pool_streams,
                                             scale, norm_frames, pool.as_mut_ptr(), out.as_mut_ptr()) })
}

/// The mfe form of `try_mfcc_stream_packed_i16`: `feat` `[rows x num_filters]`, `energy` `[rows]`.
pub fn try_mfe_stream_packed_i16(cfg: &SpeechConfig, x: &[i16], sample_offsets: &[i64], slots: &[i32], pool_streams: usize, scale: f32,
                                 pool: &mut [f32], feat: &mut [f32], energy: &mut [f32]) -> Result<(), Error> {
    if sample_offsets.len() != slots.len() + 1 {
        return Err(Error { status: SS_ERR_ARG, detail: "sample_offsets must have one entry more than slots".to_string() });
    }
    check(unsafe { ss_mfe_stream_packed_i16(cfg.raw(), x.as_ptr(), slots.len(), sample_offsets.as_ptr(), slots.as_ptr(), pool_streams,
                                            scale, pool.as_mut_ptr(), feat.as_mut_ptr(), energy.as_mut_ptr()) })
}

/// The one-shot MFCC of equal-length clips fed signed 16-bit PCM (`ss_mfcc_batch_i16_device`): `mfcc_batch_device` with the samples as
/// int16, sample = `pcm as f32 * scale`, `scale` a power of two in `[2^-64, 2^64]`; bit for bit the float call on the converted
/// buffer.  `ld` is in samples; `d_x` needs 2-byte alignment only.
/// # Safety
/// As `mfcc_batch_device`.
pub unsafe fn mfcc_batch_i16_device(cfg: &SpeechConfig, d_x: *const i16, batch: usize, n: usize, ld: usize, scale: f32, d_out: *mut f32,
                                    stream: *mut c_void) -> Result<(), Error> {
    check(ss_mfcc_batch_i16_device(cfg.raw(), d_x, batch, n, ld, scale, d_out, stream))
}

/// The mfe form of `mfcc_batch_i16_device`: `d_feat` `[batch x frames x num_filters]`, `d_energy` `[batch x frames]`.
/// # Safety
/// As `mfcc_batch_device`.
pub unsafe fn mfe_batch_i16_device(cfg: &SpeechConfig, d_x: *const i16, batch: usize, n: usize, ld: usize, scale: f32, d_feat: *mut f32,
                                   d_energy: *mut f32, stream: *mut c_void) -> Result<(), Error> {
    check(ss_mfe_batch_i16_device(cfg.raw(), d_x, batch, n, ld, scale, d_feat, d_energy, stream))
}

/// MFCC of packed variable-length clips fed signed 16-bit PCM (`ss_mfcc_packed_i16_device`): clip `b` is
/// `d_x[so[b]..so[b + 1]]`, its rows `fo[b]..fo[b + 1]` of `d_out`; the tables are device arrays, offsets in samples.
/// # Safety
/// Every pointer is a device allocation of the size the header states, on the device the config was created on.
pub unsafe fn mfcc_packed_i16_device(cfg: &SpeechConfig, d_x: *const i16, n_clips: usize, d_sample_offsets: *const i64, scale: f32,
                                     d_frame_offsets: *const i64, total_frames: usize, d_out: *mut f32, stream: *mut c_void)
                                     -> Result<(), Error> {
    check(ss_mfcc_packed_i16_device(cfg.raw(), d_x, n_clips, d_sample_offsets, scale, d_frame_offsets, total_frames, d_out, stream))
}

/// The mfe form of `mfcc_packed_i16_device`.
/// # Safety
/// As `mfcc_packed_i16_device`.
pub unsafe fn mfe_packed_i16_device(cfg: &SpeechConfig, d_x: *const i16, n_clips: usize, d_sample_offsets: *const i64, scale: f32,
                                    d_frame_offsets: *const i64, total_frames: usize, d_feat: *mut f32, d_energy: *mut f32,
                                    stream: *mut c_void) -> Result<(), Error> {
    check(ss_mfe_packed_i16_device(cfg.raw(), d_x, n_clips, d_sample_offsets, scale, d_frame_offsets, total_frames, d_feat, d_energy,
                                   stream))
}

/// Host-pointer forms: the samples cross the link as int16.  `x` holds `batch` rows of `n` samples at row stride `ld`; `out` is
/// `[batch x frames x num_cepstral]`.  Synchronous.
pub fn try_mfcc_batch_i16(cfg: &SpeechConfig, x: &[i16], batch: usize, n: usize, ld: usize, scale: f32, out: &mut [f32])
                          -> Result<(), Error> {
    if batch > 0 && (ld < n || x.len() < (batch - 1) * ld + n) {
        return Err(Error { status: SS_ERR_ARG, detail: "x is shorter than batch rows of n samples at stride ld".to_string() });
    }
    check(unsafe { ss_mfcc_batch_i16(cfg.raw(), x.as_ptr(), batch, n, ld, scale, out.as_mut_ptr()) })
}

/// The mfe form of `try_mfcc_batch_i16`: `feat` `[batch x frames x num_filters]`, `energy` `[batch x frames]`.
pub fn try_mfe_batch_i16(cfg: &SpeechConfig, x: &[i16], batch: usize, n: usize, ld: usize, scale: f32, feat: &mut [f32],
                         energy: &mut [f32]) -> Result<(), Error> {
    if batch > 0 && (ld < n || x.len() < (batch - 1) * ld + n) {
        return Err(Error { status: SS_ERR_ARG, detail: "x is shorter than batch rows of n samples at stride ld".to_string() });
    }
    check(unsafe { ss_mfe_batch_i16(cfg.raw(), x.as_ptr(), batch, n, ld, scale, feat.as_mut_ptr(), energy.as_mut_ptr()) })
}

/// Packed clips from an int16 host buffer: `sample_offsets` holds `n_clips + 1` offsets in samples, `out` the clips' rows end to end.
pub fn try_mfcc_packed_i16(cfg: &SpeechConfig, x: &[i16], sample_offsets: &[i64], scale: f32, out: &mut [f32]) -> Result<(), Error> {
    if sample_offsets.is_empty() {
        return Err(Error { status: SS_ERR_ARG, detail: "sample_offsets must have n_clips + 1 entries".to_string() });
    }
    check(unsafe { ss_mfcc_packed_i16(cfg.raw(), x.as_ptr(), sample_offsets.len() - 1, sample_offsets.as_ptr(), scale, out.as_mut_ptr()) })
}

/// The mfe form of `try_mfcc_packed_i16`.
pub fn try_mfe_packed_i16(cfg: &SpeechConfig, x: &[i16], sample_offsets: &[i64], scale: f32, feat: &mut [f32], energy: &mut [f32])
                          -> Result<(), Error> {
    if sample_offsets.is_empty() {
        return Err(Error { status: SS_ERR_ARG, detail: "sample_offsets must have n_clips + 1 entries".to_string() });
    }
    check(unsafe { ss_mfe_packed_i16(cfg.raw(), x.as_ptr(), sample_offsets.len() - 1, sample_offsets.as_ptr(), scale, feat.as_mut_ptr(),
                                     energy.as_mut_ptr()) })
}

/// The mel spectrogram / STFT calls fed signed 16-bit PCM (`ss_mel_spectrogram_i16_device`, `ss_stft_i16_device` and their packed and
/// pool forms): the float forms with the samples as int16, sample = `pcm as f32 * scale`, `scale` a power of two in `[2^-64, 2^64]`;
/// bit for bit the float call on the converted buffer.  `ld` and the offsets are in samples; `d_x` needs 2-byte alignment only
/// (4-byte for the pool forms).  `d_out`: `[channels x num_filters x rows]`.
/// # Safety
/// Every pointer is a device allocation of the size the header states, on the device the config was created on.
pub unsafe fn mel_spectrogram_i16_device(cfg: &SpeechConfig, d_x: *const i16, channels: usize, n: usize, ld: usize, scale: f32,
                                         d_out: *mut f32, stream: *mut c_void) -> Result<(), Error> {
    check(ss_mel_spectrogram_i16_device(cfg.raw(), d_x, channels, n, ld, scale, d_out, stream))
}

/// The stft form of `mel_spectrogram_i16_device`: `d_out` `[channels x rows x (fft_points / 2 + 1) x 2]`.
/// # Safety
/// As `mel_spectrogram_i16_device`.
pub unsafe fn stft_i16_device(cfg: &SpeechConfig, d_x: *const i16, channels: usize, n: usize, ld: usize, scale: f32, d_out: *mut f32,
                              stream: *mut c_void) -> Result<(), Error> {
    check(ss_stft_i16_device(cfg.raw(), d_x, channels, n, ld, scale, d_out, stream))
}

/// Packed variable-length clips (`ss_mel_spectrogram_packed_i16_device`): clip `b` is `d_x[so[b]..so[b + 1]]`, its `[num_filters x R_b]`
/// block starts at `d_out + num_filters * ro[b]`; the tables are device arrays.
/// # Safety
/// As `mel_spectrogram_i16_device`.
pub unsafe fn mel_spectrogram_packed_i16_device(cfg: &SpeechConfig, d_x: *const i16, n_clips: usize, d_sample_offsets: *const i64,
                                                scale: f32, d_row_offsets: *const i64, total_rows: usize, d_out: *mut f32,
                                                stream: *mut c_void) -> Result<(), Error> {
    check(ss_mel_spectrogram_packed_i16_device(cfg.raw(), d_x, n_clips, d_sample_offsets, scale, d_row_offsets, total_rows, d_out, stream))
}

/// The stft form of `mel_spectrogram_packed_i16_device`: clip `b` owns rows `ro[b]..ro[b + 1]` of `d_out`.
/// # Safety
/// As `mel_spectrogram_i16_device`.
pub unsafe fn stft_packed_i16_device(cfg: &SpeechConfig, d_x: *const i16, n_clips: usize, d_sample_offsets: *const i64, scale: f32,
                                     d_row_offsets: *const i64, total_rows: usize, d_out: *mut f32, stream: *mut c_void)
                                     -> Result<(), Error> {
    check(ss_stft_packed_i16_device(cfg.raw(), d_x, n_clips, d_sample_offsets, scale, d_row_offsets, total_rows, d_out, stream))
}

/// The ragged streaming pool (`ss_mel_spectrogram_stream_packed_i16_device`): entry `i` is the chunk `d_x[so[i]..so[i + 1]]` (whole
/// hops) of the stream whose state is row `d_slots[i]` of the `[pool_streams x S]` float pool.  Two asynchronous launches.
/// # Safety
/// As `mel_spectrogram_i16_device`; `d_x` is 4-byte aligned.
pub unsafe fn mel_spectrogram_stream_packed_i16_device(cfg: &SpeechConfig, d_x: *const i16, n_active: usize, d_sample_offsets: *const i64,
                                                       d_row_offsets: *const i64, total_rows: usize, d_slots: *const i32,
                                                       pool_streams: usize, scale: f32, d_pool: *mut f32, d_out: *mut f32,
                                                       stream: *mut c_void) -> Result<(), Error> {
    check(ss_mel_spectrogram_stream_packed_i16_device(cfg.raw(), d_x, n_active, d_sample_offsets, d_row_offsets, total_rows, d_slots,
                                                      pool_streams, scale, d_pool, d_out, stream))
}

/// The stft form of `mel_spectrogram_stream_packed_i16_device`.
/// # Safety
/// As `mel_spectrogram_stream_packed_i16_device`.
pub unsafe fn stft_stream_packed_i16_device(cfg: &SpeechConfig, d_x: *const i16, n_active: usize, d_sample_offsets: *const i64,
                                            d_row_offsets: *const i64, total_rows: usize, d_slots: *const i32, pool_streams: usize,
                                            scale: f32, d_pool: *mut f32, d_out: *mut f32, stream: *mut c_void) -> Result<(), Error> {
    check(ss_stft_stream_packed_i16_device(cfg.raw(), d_x, n_active, d_sample_offsets, d_row_offsets, total_rows, d_slots, pool_streams,
                                           scale, d_pool, d_out, stream))
}

/// Host-pointer forms: the samples cross the link as int16.  `x` holds `channels` rows of `n` samples; `out` is
/// `[channels x num_filters x rows]`.  Synchronous.
pub fn try_mel_spectrogram_i16(cfg: &SpeechConfig, x: &[i16], channels: usize, n: usize, scale: f32, out: &mut [f32]) -> Result<(), Error> {
    if x.len() < channels * n {
        return Err(Error { status: SS_ERR_ARG, detail: "x is shorter than channels rows of n samples".to_string() });
    }
    check(unsafe { ss_mel_spectrogram_i16(cfg.raw(), x.as_ptr(), channels, n, scale, out.as_mut_ptr()) })
}

/// The stft form of `try_mel_spectrogram_i16`: `out` `[channels x rows x (fft_points / 2 + 1) x 2]`.
pub fn try_stft_i16(cfg: &SpeechConfig, x: &[i16], channels: usize, n: usize, scale: f32, out: &mut [f32]) -> Result<(), Error> {
    if x.len() < channels * n {
        return Err(Error { status: SS_ERR_ARG, detail: "x is shorter than channels rows of n samples".to_string() });
    }
    check(unsafe { ss_stft_i16(cfg.raw(), x.as_ptr(), channels, n, scale, out.as_mut_ptr()) })
}

/// Packed clips from an int16 host buffer: `sample_offsets` holds `n_clips + 1` offsets in samples, `out` the clips' blocks end to end.
pub fn try_mel_spectrogram_packed_i16(cfg: &SpeechConfig, x: &[i16], sample_offsets: &[i64], scale: f32, out: &mut [f32])
                                      -> Result<(), Error> {
    if sample_offsets.is_empty() {
        return Err(Error { status: SS_ERR_ARG, detail: "sample_offsets must have n_clips + 1 entries".to_string() });
    }
    check(unsafe { ss_mel_spectrogram_packed_i16(cfg.raw(), x.as_ptr(), sample_offsets.len() - 1, sample_offsets.as_ptr(), scale,
                                                 out.as_mut_ptr()) })
}

/// What the log-mel calls add to their mel counterparts: librosa's `power_to_db` arguments.  `top_db < 0.0` switches the floor off.
#[derive(Clone, Copy, Debug)]
pub struct DbScale {
    pub ref_: f32,
    pub amin: f32,
    pub top_db: f32,
}

impl Default for DbScale {
    fn default() -> Self {
        DbScale { ref_: 1.0, amin: 1e-10, top_db: 80.0 }
    }
}

/// Log-mel spectrogram (`ss_log_mel_spectrogram_device`): `mel_spectrogram` in decibels, converted in the mel kernel's epilogue.  Per
/// clip (channel) bit for bit the mel call followed by `ss_power_to_db_packed_device` with every clip as its own segment: the `top_db`
/// floor is the clip's own maximum - `top_db` -- not the one maximum `ss_power_to_db_device` takes over a multi-channel block.
/// `d_out`: `[channels x num_filters x rows]`.
/// # Safety
/// Every pointer is a device allocation of the size the header states, on the device the config was created on.
pub unsafe fn log_mel_spectrogram_device(cfg: &SpeechConfig, d_x: *const f32, channels: usize, n: usize, ld: usize, db: DbScale,
                                         d_out: *mut f32, stream: *mut c_void) -> Result<(), Error> {
    check(ss_log_mel_spectrogram_device(cfg.raw(), d_x, channels, n, ld, db.ref_, db.amin, db.top_db, d_out, stream))
}

/// `log_mel_spectrogram_device` fed signed 16-bit PCM (`sample = pcm as f32 * scale`, `scale` a power of two).
/// # Safety
/// As `log_mel_spectrogram_device`.
pub unsafe fn log_mel_spectrogram_i16_device(cfg: &SpeechConfig, d_x: *const i16, channels: usize, n: usize, ld: usize, scale: f32,
                                             db: DbScale, d_out: *mut f32, stream: *mut c_void) -> Result<(), Error> {
    check(ss_log_mel_spectrogram_i16_device(cfg.raw(), d_x, channels, n, ld, scale, db.ref_, db.amin, db.top_db, d_out, stream))
}

/// Packed variable-length clips (`ss_log_mel_spectrogram_packed_device`): the layout of `ss_mel_spectrogram_packed_device`, every clip's
/// block in decibels and floored at its own maximum - `top_db`; the tables are device arrays.
/// # Safety
/// As `log_mel_spectrogram_device`.
pub unsafe fn log_mel_spectrogram_packed_device(cfg: &SpeechConfig, d_x: *const f32, n_clips: usize, d_sample_offsets: *const i64,
                                                d_row_offsets: *const i64, total_rows: usize, db: DbScale, d_out: *mut f32,
                                                stream: *mut c_void) -> Result<(), Error> {
    check(ss_log_mel_spectrogram_packed_device(cfg.raw(), d_x, n_clips, d_sample_offsets, d_row_offsets, total_rows, db.ref_, db.amin,
                                               db.top_db, d_out, stream))
}

/// `log_mel_spectrogram_packed_device` fed signed 16-bit PCM.
/// # Safety
/// As `log_mel_spectrogram_device`.
pub unsafe fn log_mel_spectrogram_packed_i16_device(cfg: &SpeechConfig, d_x: *const i16, n_clips: usize, d_sample_offsets: *const i64,
                                                    scale: f32, d_row_offsets: *const i64, total_rows: usize, db: DbScale,
                                                    d_out: *mut f32, stream: *mut c_void) -> Result<(), Error> {
    check(ss_log_mel_spectrogram_packed_i16_device(cfg.raw(), d_x, n_clips, d_sample_offsets, scale, d_row_offsets, total_rows, db.ref_,
                                                   db.amin, db.top_db, d_out, stream))
}

/// Host-pointer forms of the log-mel calls.  `x` holds `channels` rows of `n` samples; `out` is `[channels x num_filters x rows]`.
pub fn try_log_mel_spectrogram(cfg: &SpeechConfig, x: &[f32], channels: usize, n: usize, db: DbScale, out: &mut [f32]) -> Result<(), Error> {
    if x.len() < channels * n {
        return Err(Error { status: SS_ERR_ARG, detail: "x is shorter than channels rows of n samples".to_string() });
    }
    check(unsafe { ss_log_mel_spectrogram(cfg.raw(), x.as_ptr(), channels, n, db.ref_, db.amin, db.top_db, out.as_mut_ptr()) })
}

/// `try_log_mel_spectrogram` from an int16 host buffer.
pub fn try_log_mel_spectrogram_i16(cfg: &SpeechConfig, x: &[i16], channels: usize, n: usize, scale: f32, db: DbScale, out: &mut [f32])
                                   -> Result<(), Error> {
    if x.len() < channels * n {
        return Err(Error { status: SS_ERR_ARG, detail: "x is shorter than channels rows of n samples".to_string() });
    }
    check(unsafe { ss_log_mel_spectrogram_i16(cfg.raw(), x.as_ptr(), channels, n, scale, db.ref_, db.amin, db.top_db, out.as_mut_ptr()) })
}

/// Packed clips from a float host buffer: `sample_offsets` holds `n_clips + 1` offsets in samples, `out` the clips' blocks end to end.
pub fn try_log_mel_spectrogram_packed(cfg: &SpeechConfig, x: &[f32], sample_offsets: &[i64], db: DbScale, out: &mut [f32])
                                      -> Result<(), Error> {
    if sample_offsets.is_empty() {
        return Err(Error { status: SS_ERR_ARG, detail: "sample_offsets must have n_clips + 1 entries".to_string() });
    }
    check(unsafe { ss_log_mel_spectrogram_packed(cfg.raw(), x.as_ptr(), sample_offsets.len() - 1, sample_offsets.as_ptr(), db.ref_, db.amin,
                                                 db.top_db, out.as_mut_ptr()) })
}

/// `try_log_mel_spectrogram_packed` from an int16 host buffer.
pub fn try_log_mel_spectrogram_packed_i16(cfg: &SpeechConfig, x: &[i16], sample_offsets: &[i64], scale: f32, db: DbScale, out: &mut [f32])
                                          -> Result<(), Error> {
    if sample_offsets.is_empty() {
        return Err(Error { status: SS_ERR_ARG, detail: "sample_offsets must have n_clips + 1 entries".to_string() });
    }
    check(unsafe { ss_log_mel_spectrogram_packed_i16(cfg.raw(), x.as_ptr(), sample_offsets.len() - 1, sample_offsets.as_ptr(), scale,
                                                     db.ref_, db.amin, db.top_db, out.as_mut_ptr()) })
}

/// The stft form of `try_mel_spectrogram_packed_i16`.
pub fn try_stft_packed_i16(cfg: &SpeechConfig, x: &[i16], sample_offsets: &[i64], scale: f32, out: &mut [f32]) -> Result<(), Error> {
    if sample_offsets.is_empty() {
        return Err(Error { status: SS_ERR_ARG, detail: "sample_offsets must have n_clips + 1 entries".to_string() });
    }
    check(unsafe { ss_stft_packed_i16(cfg.raw(), x.as_ptr(), sample_offsets.len() - 1, sample_offsets.as_ptr(), scale, out.as_mut_ptr()) })
}

/// Host-pointer form of the PCM pool call: `x` the packed int16 chunks, `sample_offsets` `n_active + 1` offsets in samples, `slots`
/// the pool row of each entry, `pool` the `[pool_streams x S]` float states (updated in place).  Synchronous.
pub fn try_mel_spectrogram_stream_packed_i16(cfg: &SpeechConfig, x: &[i16], sample_offsets: &[i64], slots: &[i32], pool_streams: usize,
                                             scale: f32, pool: &mut [f32], out: &mut [f32]) -> Result<(), Error> {
    if sample_offsets.len() != slots.len() + 1 {
        return Err(Error { status: SS_ERR_ARG, detail: "sample_offsets must have one entry more than slots".to_string() });
    }
    check(unsafe { ss_mel_spectrogram_stream_packed_i16(cfg.raw(), x.as_ptr(), slots.len(), sample_offsets.as_ptr(), slots.as_ptr(),
                                                        pool_streams, scale, pool.as_mut_ptr(), out.as_mut_ptr()) })
}

/// The stft form of `try_mel_spectrogram_stream_packed_i16`.
pub fn try_stft_stream_packed_i16(cfg: &SpeechConfig, x: &[i16], sample_offsets: &[i64], slots: &[i32], pool_streams: usize, scale: f32,
                                  pool: &mut [f32], out: &mut [f32]) -> Result<(), Error> {
    if sample_offsets.len() != slots.len() + 1 {
        return Err(Error { status: SS_ERR_ARG, detail: "sample_offsets must have one entry more than slots".to_string() });
    }
    check(unsafe { ss_stft_stream_packed_i16(cfg.raw(), x.as_ptr(), slots.len(), sample_offsets.as_ptr(), slots.as_ptr(), pool_streams,
                                             scale, pool.as_mut_ptr(), out.as_mut_ptr()) })
}

/// functions.rs:86-123: `[channels, samples]` -> `Array3<Complex32>` `[channels, rows, freq_size]`
pub fn try_stft2(input: ArrayView2<f32>, cfg: &SpeechConfig) -> Result<Array3<Complex32>, Error> {
    let owned = input.as_standard_layout();
    let (ch, n) = owned.dim();
    let (mut rows, mut _real) = (0usize, 0usize);
    check(unsafe { ss_stft_rows(&cfg.params, n, &mut rows, &mut _real) })?;
    let mut out = Array3::<Complex32>::zeros((ch, rows, cfg.freq_size));
    // Complex32 is #[repr(C)] { re: f32, im: f32 }: the interleaved block the ABI writes
    check(unsafe { ss_stft(cfg.raw(), owned.as_ptr(), ch, n, out.as_mut_ptr() as *mut f32) })?;
    Ok(out)
}
pub fn stft2(input: ArrayView2<f32>, cfg: &SpeechConfig) -> Array3<Complex32> { try_stft2(input, cfg).expect("stft2") }

/// functions.rs:199-233 (one channel): `Array2<Complex32>` `[rows, freq_size]`
pub fn stft1(input: ArrayView1<f32>, cfg: &SpeechConfig) -> Array2<Complex32> {
    let x = contiguous(input);
    let v = ArrayView2::from_shape((1, x.len()), &x[..]).expect("shape");
    let out = stft2(v, cfg);
    let (_, r, f) = out.dim();
    out.into_shape((r, f)).expect("shape")
}

/// processing.rs:65-129 with the reference's own signature:
/// `stack_frames(signal, sample_rate, frame_length, frame_stride, filter, zero_padding) -> Array2<f32>` -- a caller of
/// `speechsauce::processing::stack_frames` switches the `use` line and nothing else.  `filter` is called with the frame
/// length and its row 0 multiplies every frame (what `repeat_axis(filt, Axis(0), numframes)` does with the reference's
/// `(1, frame_len)` array, processing.rs:122-126); the framing is the documented contract (frame t = samples
/// `t * step .. t * step + frame_len`), see SURVEY.md Q1 for what the reference's copy loop does instead.
pub fn try_stack_frames(signal: ArrayView1<f32>, sample_rate: usize, frame_length: f32, frame_stride: f32,
                        filter: Option<fn(usize) -> Array2<f32>>, zero_padding: bool) -> Result<Array2<f32>, Error> {
    let x = contiguous(signal);
    let (mut t, mut flen) = (0usize, 0usize);
    if sample_rate > u32::MAX as usize {
        return Err(Error { status: SS_ERR_ARG, detail: "sample_rate does not fit 32 bits".to_string() });
    }
    check(unsafe { ss_stack_frames_shape(x.len(), sample_rate as u32, frame_length, frame_stride, zero_padding as c_int, &mut t, &mut flen) })?;
    let window: Option<Vec<f32>> = match filter {
        None => None,
        Some(f) => {
            let w = f(flen);
            // row 0 of the (1, frame_len) array; a (frame_len, 1) column (feature.rs:176-178 `_f_it`) is read down its column
            let v: Vec<f32> = if w.nrows() == 1 { w.row(0).to_vec() } else { w.column(0).to_vec() };
            if v.len() != flen {  // the try_ form reports, it does not panic
                return Err(Error { status: SS_ERR_ARG, detail: format!("filter({}) gave {} values", flen, v.len()) });
            }
            Some(v)
        }
    };
    let mut out = Array2::<f32>::zeros((t, flen));
    let wptr = window.as_ref().map_or(std::ptr::null(), |w| w.as_ptr());
    check(unsafe { ss_stack_frames_signal(x.as_ptr(), x.len(), sample_rate as u32, frame_length, frame_stride, wptr, zero_padding as c_int, out.as_mut_ptr()) })?;
    Ok(out)
}
pub fn stack_frames(signal: ArrayView1<f32>, sample_rate: usize, frame_length: f32, frame_stride: f32,
                    filter: Option<fn(usize) -> Array2<f32>>, zero_padding: bool) -> Array2<f32> {
    try_stack_frames(signal, sample_rate, frame_length, frame_stride, filter, zero_padding).expect("stack_frames")
}

/// The same stage with the framing taken from a config (its `framing` / `mfcc_window` / `pad_mode` switches apply: literal and
/// centred framing exist only in this form).  An extra beside the reference's signature above.
pub fn try_stack_frames_with(signal: ArrayView1<f32>, cfg: &SpeechConfig) -> Result<Array2<f32>, Error> {
    let x = contiguous(signal);
    let (mut t, mut flen, mut _step) = (0usize, 0usize, 0usize);
    check(unsafe { ss_num_frames(&cfg.params, x.len(), &mut t) })?;
    check(unsafe { ss_frame_sizes(&cfg.params, &mut flen, &mut _step) })?;
    let mut out = Array2::<f32>::zeros((t, flen));
    check(unsafe { ss_stack_frames(cfg.raw(), x.as_ptr(), x.len(), out.as_mut_ptr()) })?;
    Ok(out)
}
pub fn stack_frames_with(signal: ArrayView1<f32>, cfg: &SpeechConfig) -> Array2<f32> { try_stack_frames_with(signal, cfg).expect("stack_frames") }

/// processing.rs:179-181 with the reference's own signature: `power_spectrum(frames: Array2<f32>, fft_points: usize)`.
/// Only `fft_points` matters to this stage; the config it runs on is kept per `fft_points` in a small process-wide cache
/// (the Python front memoises the same way), so repeated calls cost one lookup.
pub fn try_power_spectrum(frames: Array2<f32>, fft_points: usize) -> Result<Array2<f32>, Error> {
    use std::collections::HashMap;
    use std::sync::{Mutex, OnceLock};
    struct Kept(*mut SsConfig);
    unsafe impl Send for Kept {}  // the handle is immutable after creation and thread-safe (speechsauce_amd.h)
    static CACHE: OnceLock<Mutex<HashMap<usize, Kept>>> = OnceLock::new();
    let cache = CACHE.get_or_init(|| Mutex::new(HashMap::new()));
    let handle = {
        let mut map = cache.lock().expect("power_spectrum config cache");
        if let Some(h) = map.get(&fft_points) {
            h.0
        } else {
            // a config that validates for this FFT length: a frame of half its length, a bank that fits its spectrum
            let mut p = SpeechConfigBuilder::new(16000).p;
            p.fft_points = fft_points as u32;
            p.frame_length = fft_points as f32 / 32000.0;
            p.frame_stride = fft_points as f32 / 64000.0;
            p.num_filters = std::cmp::max(1, std::cmp::min(40, fft_points / 8)) as u32;
            p.num_cepstral = std::cmp::min(13, p.num_filters);
            let mut h: *mut SsConfig = std::ptr::null_mut();
            check(unsafe { ss_config_create(&p, &mut h) })?;
            map.insert(fft_points, Kept(h));  // kept for the life of the process
            h
        }
    };
    let x = frames.as_standard_layout();
    let (rows, cols) = x.dim();
    let mut out = Array2::<f32>::zeros((rows, fft_points / 2 + 1));
    check(unsafe { ss_power_spectrum_frames(handle, x.as_ptr(), rows, cols, out.as_mut_ptr()) })?;
    Ok(out)
}
pub fn power_spectrum(frames: Array2<f32>, fft_points: usize) -> Array2<f32> { try_power_spectrum(frames, fft_points).expect("power_spectrum") }

/// The same stage on an existing config (`fft_points` is the config's).  An extra beside the reference's signature above.
pub fn try_power_spectrum_with(frames: Array2<f32>, cfg: &SpeechConfig) -> Result<Array2<f32>, Error> {
    let x = frames.as_standard_layout();
    let (rows, cols) = x.dim();
    let mut out = Array2::<f32>::zeros((rows, cfg.freq_size));
    check(unsafe { ss_power_spectrum_frames(cfg.raw(), x.as_ptr(), rows, cols, out.as_mut_ptr()) })?;
    Ok(out)
}
pub fn power_spectrum_with(frames: Array2<f32>, cfg: &SpeechConfig) -> Array2<f32> { try_power_spectrum_with(frames, cfg).expect("power_spectrum") }

/// stack_frames + power_spectrum fused, as mfe uses them (feature.rs:203-214): `[frames, freq_size]`
pub fn try_power_spectrum_of_signal(signal: ArrayView1<f32>, cfg: &SpeechConfig) -> Result<Array2<f32>, Error> {
    let x = contiguous(signal);
    let mut t = 0usize;
    check(unsafe { ss_num_frames(&cfg.params, x.len(), &mut t) })?;
    let mut out = Array2::<f32>::zeros((t, cfg.freq_size));
    check(unsafe { ss_power_spectrum(cfg.raw(), x.as_ptr(), x.len(), out.as_mut_ptr()) })?;
    Ok(out)
}

/// (hop, n_pad, wnorm) of the STFT path as the library computes them (functions.rs:96-97, config.rs:178); `Err` for a config whose
/// `fft_points < 2 * frame_size` (the reference's `frame_analysis` underflows there, functions.rs:136).
pub fn stft_sizes(cfg: &SpeechConfig) -> Result<(usize, usize, f32), Error> {
    let (mut hop, mut n_pad, mut wnorm) = (0usize, 0usize, 0f32);
    check(unsafe { ss_stft_sizes(&cfg.params, &mut hop, &mut n_pad, &mut wnorm) })?;
    Ok((hop, n_pad, wnorm))
}

/// Status of the asynchronous launches made on `cfg` (`Err` with status 6 after a device-side protocol error; cleared by the call).
pub fn device_status(cfg: &SpeechConfig) -> Result<(), Error> { check(unsafe { ss_config_device_status(cfg.raw()) }) }

/// processing.rs:31-53
pub fn preemphasis(signal: Array1<f32>, shift: isize, cof: f32) -> Array1<f32> {
    let x = signal.as_standard_layout();
    let mut y = Array1::<f32>::zeros(x.len());
    check(unsafe { ss_preemphasis(x.as_ptr(), x.len(), shift as c_long, cof, y.as_mut_ptr()) }).expect("preemphasis");
    y
}

/// processing.rs:265-300
pub fn cmvn(vec: ArrayView2<f32>, variance_normalization: bool) -> Array2<f32> {
    let x = vec.as_standard_layout();
    let (rows, cols) = x.dim();
    let mut out = Array2::<f32>::zeros((rows, cols));
    check(unsafe { ss_cmvn(x.as_ptr(), rows, cols, variance_normalization as c_int, out.as_mut_ptr()) }).expect("cmvn");
    out
}

/// processing.rs:315-371 (panics on an even `win_size`, like the reference's assert)
pub fn cmvnw(vec: Array2<f32>, win_size: usize, variance_normalization: bool) -> Array2<f32> {
    let x = vec.as_standard_layout();
    let (rows, cols) = x.dim();
    let mut out = Array2::<f32>::zeros((rows, cols));
    check(unsafe { ss_cmvnw(x.as_ptr(), rows, cols, win_size, variance_normalization as c_int, out.as_mut_ptr()) })
        .expect("Windows size must be odd!");
    out
}

/// `cmvn` of every clip of a packed block on its own rows (a loop over processing.rs:265-300 per clip, one launch): clip b owns rows
/// `offsets[b] .. offsets[b + 1]` of `vec`; `offsets` has n_clips + 1 non-decreasing entries and starts at 0.
pub fn try_cmvn_packed(vec: ArrayView2<f32>, offsets: &[i64], variance_normalization: bool) -> Result<Array2<f32>, Error> {
    let x = vec.as_standard_layout();
    let (rows, cols) = x.dim();
    let mut out = Array2::<f32>::zeros((rows, cols));
    check(unsafe {
        ss_cmvn_packed(x.as_ptr(), offsets.len().saturating_sub(1), offsets.as_ptr(), rows, cols, variance_normalization as c_int,
                       out.as_mut_ptr())
    })?;
    Ok(out)
}

/// `cmvnw` of every clip of a packed block on its own rows (processing.rs:315-371 per clip): the symmetric padding reflects at the
/// clip's own first and last row.  `Err` with status 2 for an even `win_size`.
pub fn try_cmvnw_packed(vec: ArrayView2<f32>, offsets: &[i64], win_size: usize, variance_normalization: bool) -> Result<Array2<f32>, Error> {
    let x = vec.as_standard_layout();
    let (rows, cols) = x.dim();
    let mut out = Array2::<f32>::zeros((rows, cols));
    check(unsafe {
        ss_cmvnw_packed(x.as_ptr(), offsets.len().saturating_sub(1), offsets.as_ptr(), rows, cols, win_size,
                        variance_normalization as c_int, out.as_mut_ptr())
    })?;
    Ok(out)
}

/// Doubles per group of a grouped-CMVN statistics block: `2 * cols + 1`, a row `[n | mean | var]`.
pub fn try_cmvn_stats_len(cols: usize) -> Result<usize, Error> {
    let mut len = 0usize;
    check(unsafe { ss_cmvn_stats_len(cols, &mut len) })?;
    Ok(len)
}

fn group_ptr(groups: Option<&[i32]>, n_clips: usize) -> Result<*const i32, Error> {
    match groups {
        None => Ok(std::ptr::null()),
        Some(g) if g.len() == n_clips => Ok(g.as_ptr()),
        Some(_) => Err(Error { status: SS_ERR_ARG, detail: "groups must name one group per clip".to_string() }),
    }
}

/// Folds every clip of a packed block into the statistics row of its group (`groups[b]`, -1 leaves a clip out, `None`: group 0 for
/// every clip).  `stats` is the caller's `[n_groups x try_cmvn_stats_len(cols)]` block, updated in place; all zeros is fresh.
pub fn try_cmvn_stats_packed(vec: ArrayView2<f32>, offsets: &[i64], groups: Option<&[i32]>, n_groups: usize, stats: &mut [f64]) -> Result<(), Error> {
    let x = vec.as_standard_layout();
    let (rows, cols) = x.dim();
    let n_clips = offsets.len().saturating_sub(1);
    if stats.len() != n_groups * try_cmvn_stats_len(cols)? {
        return Err(Error { status: SS_ERR_ARG, detail: "stats must hold n_groups rows of 2 * cols + 1 doubles".to_string() });
    }
    let g = group_ptr(groups, n_clips)?;
    check(unsafe { ss_cmvn_stats_packed(x.as_ptr(), n_clips, offsets.as_ptr(), rows, cols, g, n_groups, stats.as_mut_ptr()) })
}

/// Normalises every clip by the stored statistics of its group: `(x - mean_g) / (sqrt(var_g) + 2^-30)`, or `x - mean_g`.  Rows of
/// clips that are left out (group -1, a group that has seen no row) come back as zeros.
pub fn try_cmvn_apply_packed(vec: ArrayView2<f32>, offsets: &[i64], groups: Option<&[i32]>, n_groups: usize, stats: &[f64],
                             variance_normalization: bool) -> Result<Array2<f32>, Error> {
    let x = vec.as_standard_layout();
    let (rows, cols) = x.dim();
    let n_clips = offsets.len().saturating_sub(1);
    if stats.len() != n_groups * try_cmvn_stats_len(cols)? {
        return Err(Error { status: SS_ERR_ARG, detail: "stats must hold n_groups rows of 2 * cols + 1 doubles".to_string() });
    }
    let g = group_ptr(groups, n_clips)?;
    let mut out = Array2::<f32>::zeros((rows, cols));
    check(unsafe {
        ss_cmvn_apply_packed(x.as_ptr(), n_clips, offsets.as_ptr(), rows, cols, g, n_groups, stats.as_ptr(), variance_normalization as c_int,
                             out.as_mut_ptr())
    })?;
    Ok(out)
}

/// Per-speaker CMVN of one batch: the statistics of every group from the batch's own clips, then the apply, in one call.
pub fn try_cmvn_grouped_packed(vec: ArrayView2<f32>, offsets: &[i64], groups: Option<&[i32]>, n_groups: usize,
                               variance_normalization: bool) -> Result<Array2<f32>, Error> {
    let x = vec.as_standard_layout();
    let (rows, cols) = x.dim();
    let n_clips = offsets.len().saturating_sub(1);
    let g = group_ptr(groups, n_clips)?;
    let mut out = Array2::<f32>::zeros((rows, cols));
    check(unsafe {
        ss_cmvn_grouped_packed(x.as_ptr(), n_clips, offsets.as_ptr(), rows, cols, g, n_groups, variance_normalization as c_int, out.as_mut_ptr())
    })?;
    Ok(out)
}

/// One statistics row -> Kaldi's `[2 x (cols + 1)]` accumulator (`sum x | count`, then `sum x^2 | 0`), row-major.
pub fn try_cmvn_stats_to_kaldi(stats_row: &[f64]) -> Result<Vec<f64>, Error> {
    if stats_row.len() < 3 || stats_row.len() % 2 == 0 {
        return Err(Error { status: SS_ERR_ARG, detail: "a statistics row has 2 * cols + 1 doubles".to_string() });
    }
    let cols = (stats_row.len() - 1) / 2;
    let mut kaldi = vec![0f64; 2 * (cols + 1)];
    check(unsafe { ss_cmvn_stats_to_kaldi(stats_row.as_ptr(), cols, kaldi.as_mut_ptr()) })?;
    Ok(kaldi)
}

/// Kaldi's `[2 x (cols + 1)]` accumulator -> one statistics row; a count below 1 gives a fresh (all-zero) row.
pub fn try_cmvn_stats_from_kaldi(kaldi: &[f64]) -> Result<Vec<f64>, Error> {
    if kaldi.len() < 4 || kaldi.len() % 2 == 1 {
        return Err(Error { status: SS_ERR_ARG, detail: "a Kaldi accumulator has 2 * (cols + 1) doubles".to_string() });
    }
    let cols = kaldi.len() / 2 - 1;
    let mut row = vec![0f64; 2 * cols + 1];
    check(unsafe { ss_cmvn_stats_from_kaldi(kaldi.as_ptr(), cols, row.as_mut_ptr()) })?;
    Ok(row)
}

/// Floats per stream of the pool `try_cmvn_stream_packed` carries: `(win_size - 1) * cols + 1`.
pub fn try_cmvn_stream_state_len(cols: usize, win_size: usize) -> Result<usize, Error> {
    let mut len = 0usize;
    check(unsafe { ss_cmvn_stream_state_len(cols, win_size, &mut len) })?;
    Ok(len)
}

/// Causal sliding-window CMVN of the rows of live streams (the causal counterpart of processing.rs:315-371): entry i owns rows
/// `row_offsets[i] .. row_offsets[i + 1]` of `vec` and row `slots[i]` of `pool`, a `[pool_streams, try_cmvn_stream_state_len]`
/// block that carries every stream's last `win_size - 1` raw rows from call to call (all zeros: fresh streams).  Every row is
/// normalised over the trailing `win_size` rows of its own stream, the row itself the newest.
pub fn try_cmvn_stream_packed(vec: ArrayView2<f32>, row_offsets: &[i64], slots: &[i32], win_size: usize, variance_normalization: bool,
                              pool: &mut Array2<f32>) -> Result<Array2<f32>, Error> {
    let x = vec.as_standard_layout();
    let (rows, cols) = x.dim();
    let len = try_cmvn_stream_state_len(cols, win_size)?;
    if row_offsets.len() != slots.len() + 1 {
        return Err(Error { status: SS_ERR_ARG, detail: "row_offsets must have one entry more than slots".to_string() });
    }
    if pool.ncols() != len || !pool.is_standard_layout() {
        return Err(Error { status: SS_ERR_ARG, detail: "pool must be a standard-layout [pool_streams, state_len] block".to_string() });
    }
    if row_offsets[slots.len()] < 0 || row_offsets[slots.len()] as usize > rows {
        return Err(Error { status: SS_ERR_ARG, detail: "row_offsets ends past the block".to_string() });
    }
    let mut out = Array2::<f32>::zeros((rows, cols));
    check(unsafe {
        ss_cmvn_stream_packed(x.as_ptr(), slots.len(), row_offsets.as_ptr(), slots.as_ptr(), pool.nrows(), cols, win_size,
                              variance_normalization as c_int, pool.as_mut_ptr(), out.as_mut_ptr())
    })?;
    Ok(out)
}

/// Kaldi add-deltas of every clip of a packed block on its own rows (edge replication at the clip's own ends): row t of the result is
/// `[x[t] | delta | delta-delta]`, `(order + 1) * cols` floats.  `order` is 1 or 2, `order * window` at most 32.  A dense matrix is
/// the one-clip call `offsets = [0, rows]`.
pub fn try_add_deltas_packed(vec: ArrayView2<f32>, offsets: &[i64], order: usize, window: usize) -> Result<Array2<f32>, Error> {
    let x = vec.as_standard_layout();
    let (rows, cols) = x.dim();
    if offsets.is_empty() || order == 0 || order > 2 {
        return Err(Error { status: SS_ERR_ARG, detail: "add_deltas_packed: offsets must not be empty and order must be 1 or 2".to_string() });
    }
    let mut out = Array2::<f32>::zeros((rows, (order + 1) * cols));
    check(unsafe { ss_add_deltas_packed(x.as_ptr(), offsets.len() - 1, offsets.as_ptr(), rows, cols, order, window, out.as_mut_ptr()) })?;
    Ok(out)
}

/// Floats per stream of the pool `try_add_deltas_stream_packed` carries: `2 * order * window * cols + 1`.
pub fn try_add_deltas_stream_state_len(cols: usize, order: usize, window: usize) -> Result<usize, Error> {
    let mut len = 0usize;
    check(unsafe { ss_add_deltas_stream_state_len(cols, order, window, &mut len) })?;
    Ok(len)
}

/// Kaldi add-deltas over the rows of live streams with a fixed latency of `order * window` rows: entry i owns rows
/// `row_offsets[i] .. row_offsets[i + 1]` of `vec` and of the result, and row `slots[i]` of `pool`, a `[pool_streams,
/// try_add_deltas_stream_state_len]` block that carries every stream's last `2 * order * window` raw rows (all zeros: fresh streams).
/// Output row k of an entry is the feature row of stream time `seen + k - order * window`; rows of negative times are zeros.
pub fn try_add_deltas_stream_packed(vec: ArrayView2<f32>, row_offsets: &[i64], slots: &[i32], order: usize, window: usize,
                                    pool: &mut Array2<f32>) -> Result<Array2<f32>, Error> {
    let x = vec.as_standard_layout();
    let (rows, cols) = x.dim();
    let len = try_add_deltas_stream_state_len(cols, order, window)?;
    if row_offsets.len() != slots.len() + 1 {
        return Err(Error { status: SS_ERR_ARG, detail: "row_offsets must have one entry more than slots".to_string() });
    }
    if pool.ncols() != len || !pool.is_standard_layout() {
        return Err(Error { status: SS_ERR_ARG, detail: "pool must be a standard-layout [pool_streams, state_len] block".to_string() });
    }
    if row_offsets[slots.len()] < 0 || row_offsets[slots.len()] as usize > rows {
        return Err(Error { status: SS_ERR_ARG, detail: "row_offsets ends past the block".to_string() });
    }
    let mut out = Array2::<f32>::zeros((rows, (order + 1) * cols));
    check(unsafe {
        ss_add_deltas_stream_packed(x.as_ptr(), slots.len(), row_offsets.as_ptr(), slots.as_ptr(), pool.nrows(), cols, order, window,
                                    pool.as_mut_ptr(), out.as_mut_ptr())
    })?;
    Ok(out)
}

/// The last `order * window` rows of the streams in `slots` (entry i: rows `i * order * window ..` of the result, right clamping at
/// the stream's last row, zeros for negative times); afterwards their pool rows are zero (fresh streams).
pub fn try_add_deltas_stream_flush(slots: &[i32], cols: usize, order: usize, window: usize, pool: &mut Array2<f32>) -> Result<Array2<f32>, Error> {
    let len = try_add_deltas_stream_state_len(cols, order, window)?;
    if pool.ncols() != len || !pool.is_standard_layout() {
        return Err(Error { status: SS_ERR_ARG, detail: "pool must be a standard-layout [pool_streams, state_len] block".to_string() });
    }
    let mut out = Array2::<f32>::zeros((slots.len() * order * window, (order + 1) * cols));
    check(unsafe {
        ss_add_deltas_stream_flush(slots.len(), slots.as_ptr(), pool.nrows(), cols, order, window, pool.as_mut_ptr(), out.as_mut_ptr())
    })?;
    Ok(out)
}

/// The scalars of Kaldi's compute-vad-energy: a row is raw-voiced where its energy (column `energy_col`) is above `energy_threshold +
/// energy_mean_scale * mean energy`, and voiced where at least `proportion_threshold` of the rows `t - frames_context .. t +
/// frames_context` inside the clip are raw-voiced.  `Default` is Kaldi's (5.0 / 0.5 / 0 / 0.6); the x-vector recipes use 5.5 / 0.5 / 2
/// / 0.12.
#[derive(Clone, Copy, Debug, PartialEq)]
pub struct VadEnergyOptions {
    pub energy_col: usize,
    pub energy_threshold: f32,
    pub energy_mean_scale: f32,
    pub frames_context: usize,
    pub proportion_threshold: f32,
}

impl Default for VadEnergyOptions {
    fn default() -> Self {
        VadEnergyOptions { energy_col: 0, energy_threshold: 5.0, energy_mean_scale: 0.5, frames_context: 0, proportion_threshold: 0.6 }
    }
}

/// Kaldi compute-vad-energy of every clip of a packed block on its own rows: one byte 0 / 1 per row and the voiced rows of every
/// clip.  A dense matrix is the one-clip call `offsets = [0, rows]`.
pub fn try_vad_energy_packed(vec: ArrayView2<f32>, offsets: &[i64], opts: VadEnergyOptions) -> Result<(Array1<u8>, Array1<i64>), Error> {
    let x = vec.as_standard_layout();
    let (rows, cols) = x.dim();
    if offsets.is_empty() {
        return Err(Error { status: SS_ERR_ARG, detail: "vad_energy_packed: offsets must not be empty".to_string() });
    }
    let mut mask = Array1::<u8>::zeros(rows);
    let mut counts = Array1::<i64>::zeros(offsets.len() - 1);
    check(unsafe {
        ss_vad_energy_packed(x.as_ptr(), offsets.len() - 1, offsets.as_ptr(), rows, cols, opts.energy_col, opts.energy_threshold,
                             opts.energy_mean_scale, opts.frames_context, opts.proportion_threshold, mask.as_mut_ptr(), counts.as_mut_ptr())
    })?;
    Ok((mask, counts))
}

/// Kaldi select-voiced-frames on a packed block: the rows whose `mask` byte is not 0, clip by clip in order (bit copies), and the
/// table of the result.  `mask` is any byte mask with one entry per row.
pub fn try_select_rows_packed(vec: ArrayView2<f32>, row_offsets: &[i64], mask: &[u8]) -> Result<(Array2<f32>, Vec<i64>), Error> {
    let x = vec.as_standard_layout();
    let (rows, cols) = x.dim();
    if row_offsets.is_empty() || mask.len() != rows {
        return Err(Error { status: SS_ERR_ARG, detail: "select_rows_packed: row_offsets must not be empty and mask needs one byte per row".to_string() });
    }
    let mut full = vec![0f32; rows * cols];
    let mut out_offsets = vec![0i64; row_offsets.len()];
    check(unsafe {
        ss_select_rows_packed(x.as_ptr(), row_offsets.len() - 1, row_offsets.as_ptr(), rows, cols, mask.as_ptr(), out_offsets.as_mut_ptr(),
                              full.as_mut_ptr())
    })?;
    let kept = out_offsets[row_offsets.len() - 1] as usize;
    full.truncate(kept * cols);
    let out = Array2::from_shape_vec((kept, cols), full).map_err(|e| Error { status: SS_ERR_ARG, detail: e.to_string() })?;
    Ok((out, out_offsets))
}

/// Floats per stream of the pool `try_vad_energy_stream_packed` carries: `2 * frames_context + 4`.
pub fn try_vad_energy_stream_state_len(frames_context: usize) -> Result<usize, Error> {
    let mut len = 0usize;
    check(unsafe { ss_vad_energy_stream_state_len(frames_context, &mut len) })?;
    Ok(len)
}

/// The decision over the rows of live streams with a fixed latency of `frames_context` rows and a causal threshold: entry i owns rows
/// `row_offsets[i] .. row_offsets[i + 1]` of `vec` and the same bytes of the result, and row `slots[i]` of `pool`, a `[pool_streams,
/// try_vad_energy_stream_state_len]` block (all zeros: fresh streams).  Byte k of an entry is the decision for stream row `seen + k -
/// frames_context`, 0 while that is negative.
pub fn try_vad_energy_stream_packed(vec: ArrayView2<f32>, row_offsets: &[i64], slots: &[i32], opts: VadEnergyOptions,
                                    pool: &mut Array2<f32>) -> Result<Array1<u8>, Error> {
    let x = vec.as_standard_layout();
    let (rows, cols) = x.dim();
    let len = try_vad_energy_stream_state_len(opts.frames_context)?;
    if row_offsets.len() != slots.len() + 1 {
        return Err(Error { status: SS_ERR_ARG, detail: "row_offsets must have one entry more than slots".to_string() });
    }
    if pool.ncols() != len || !pool.is_standard_layout() {
        return Err(Error { status: SS_ERR_ARG, detail: "pool must be a standard-layout [pool_streams, state_len] block".to_string() });
    }
    if row_offsets[slots.len()] < 0 || row_offsets[slots.len()] as usize > rows {
        return Err(Error { status: SS_ERR_ARG, detail: "row_offsets ends past the block".to_string() });
    }
    let mut mask = Array1::<u8>::zeros(rows);
    check(unsafe {
        ss_vad_energy_stream_packed(x.as_ptr(), slots.len(), row_offsets.as_ptr(), slots.as_ptr(), pool.nrows(), cols, opts.energy_col,
                                    opts.energy_threshold, opts.energy_mean_scale, opts.frames_context, opts.proportion_threshold,
                                    pool.as_mut_ptr(), mask.as_mut_ptr())
    })?;
    Ok(mask)
}

/// The last `frames_context` decisions of the streams in `slots` (entry i: bytes `i * frames_context ..` of the result, the window
/// clipped at the stream's last row, 0 for negative rows); afterwards their pool rows are zero (fresh streams).
pub fn try_vad_energy_stream_flush(slots: &[i32], opts: VadEnergyOptions, pool: &mut Array2<f32>) -> Result<Array1<u8>, Error> {
    let len = try_vad_energy_stream_state_len(opts.frames_context)?;
    if pool.ncols() != len || !pool.is_standard_layout() {
        return Err(Error { status: SS_ERR_ARG, detail: "pool must be a standard-layout [pool_streams, state_len] block".to_string() });
    }
    let mut mask = Array1::<u8>::zeros(slots.len() * opts.frames_context);
    check(unsafe {
        ss_vad_energy_stream_flush(slots.len(), slots.as_ptr(), pool.nrows(), opts.energy_threshold, opts.energy_mean_scale,
                                   opts.frames_context, opts.proportion_threshold, pool.as_mut_ptr(), mask.as_mut_ptr())
    })?;
    Ok(mask)
}

/// The device forms of the five calls above (include/speechsauce_amd.h has the contracts): every pointer is a device pointer, the
/// calls are asynchronous on `stream`, and nothing is read back.  `d_counts` may be null.
///
/// # Safety
/// The pointers must be device allocations of the sizes the header names, alive until the stream has passed the call.
pub unsafe fn vad_energy_packed_device(d_vec: *const f32, n_clips: usize, d_offsets: *const i64, total_rows: usize, cols: usize,
                                       opts: VadEnergyOptions, d_mask: *mut u8, d_counts: *mut i64, stream: *mut c_void) -> Result<(), Error> {
    check(ss_vad_energy_packed_device(d_vec, n_clips, d_offsets, total_rows, cols, opts.energy_col, opts.energy_threshold, opts.energy_mean_scale,
                                      opts.frames_context, opts.proportion_threshold, d_mask, d_counts, stream))
}

/// `d_out_offsets [n_clips + 1]` is written by the call; with `total_rows` as the bound it is a valid table for the packed calls
/// behind it.  `d_out` has room for `total_rows` rows.
///
/// # Safety
/// As `vad_energy_packed_device`.
pub unsafe fn select_rows_packed_device(d_vec: *const f32, n_clips: usize, d_row_offsets: *const i64, total_rows: usize, cols: usize,
                                        d_mask: *const u8, d_out_offsets: *mut i64, d_out: *mut f32, stream: *mut c_void) -> Result<(), Error> {
    check(ss_select_rows_packed_device(d_vec, n_clips, d_row_offsets, total_rows, cols, d_mask, d_out_offsets, d_out, stream))
}

/// # Safety
/// As `vad_energy_packed_device`; no slot may be named twice in one call.
pub unsafe fn vad_energy_stream_packed_device(d_vec: *const f32, n_active: usize, d_row_offsets: *const i64, total_rows: usize,
                                              d_slots: *const i32, pool_streams: usize, cols: usize, opts: VadEnergyOptions, d_pool: *mut f32,
                                              d_mask: *mut u8, stream: *mut c_void) -> Result<(), Error> {
    check(ss_vad_energy_stream_packed_device(d_vec, n_active, d_row_offsets, total_rows, d_slots, pool_streams, cols, opts.energy_col,
                                             opts.energy_threshold, opts.energy_mean_scale, opts.frames_context, opts.proportion_threshold, d_pool,
                                             d_mask, stream))
}

/// # Safety
/// As `vad_energy_stream_packed_device`.
pub unsafe fn vad_energy_stream_flush_device(n_active: usize, d_slots: *const i32, pool_streams: usize, opts: VadEnergyOptions, d_pool: *mut f32,
                                             d_mask: *mut u8, stream: *mut c_void) -> Result<(), Error> {
    check(ss_vad_energy_stream_flush_device(n_active, d_slots, pool_streams, opts.energy_threshold, opts.energy_mean_scale, opts.frames_context,
                                            opts.proportion_threshold, d_pool, d_mask, stream))
}

/// Layout of a padded batch: `Btc` is `[n_clips, max_rows, cols]`, `Bct` is `[n_clips, cols, max_rows]` (`SS_PAD_BTC` / `SS_PAD_BCT`).
#[derive(Clone, Copy, Debug, PartialEq)]
pub enum PadLayout {
    Btc = 0,
    Bct = 1,
}

/// Element type of a padded batch (`SS_PAD_F32` / `SS_PAD_F16` / `SS_PAD_BF16`): `F32` is a bit copy, the others round to nearest even.
#[derive(Clone, Copy, Debug, PartialEq)]
pub enum PadDtype {
    F32 = 0,
    F16 = 1,
    Bf16 = 2,
}

/// Bytes of the padded batch of `n_clips` clips: `n_clips * max_rows * cols * (4 or 2)`.
pub fn try_pad_packed_out_bytes(n_clips: usize, max_rows: usize, cols: usize, dtype: PadDtype) -> Result<usize, Error> {
    let mut bytes = 0usize;
    check(unsafe { ss_pad_packed_out_bytes(n_clips, max_rows, cols, dtype as c_int, &mut bytes) })?;
    Ok(bytes)
}

/// The padded batch of a packed block, the last stage of the packed chain: clip b's first `min(T_b, max_rows)` rows with `pad_value`
/// behind them, as the raw bytes of `dtype` in `layout`, and the rows kept of every clip.
pub fn try_pad_packed(vec: ArrayView2<f32>, row_offsets: &[i64], max_rows: usize, layout: PadLayout, dtype: PadDtype,
                      pad_value: f32) -> Result<(Vec<u8>, Vec<i32>), Error> {
    let x = vec.as_standard_layout();
    let (rows, cols) = x.dim();
    if row_offsets.is_empty() {
        return Err(Error { status: SS_ERR_ARG, detail: "pad_packed: row_offsets must not be empty".to_string() });
    }
    let n_clips = row_offsets.len() - 1;
    let mut out = vec![0u8; try_pad_packed_out_bytes(n_clips, max_rows, cols, dtype)?];
    let mut lengths = vec![0i32; n_clips];
    check(unsafe {
        ss_pad_packed(x.as_ptr(), n_clips, row_offsets.as_ptr(), rows, cols, max_rows, layout as c_int, dtype as c_int, pad_value,
                      out.as_mut_ptr() as *mut c_void, lengths.as_mut_ptr())
    })?;
    Ok((out, lengths))
}

/// The device form of `try_pad_packed` (include/speechsauce_amd.h has the contract): one asynchronous launch on `stream`, nothing
/// read back; a bad segment of the device table gives an all-pad block and length -1.
///
/// # Safety
/// As `vad_energy_packed_device`; `d_out` holds `try_pad_packed_out_bytes` bytes, `d_lengths` `n_clips` words.
pub unsafe fn pad_packed_device(d_vec: *const f32, n_clips: usize, d_row_offsets: *const i64, total_rows: usize, cols: usize, max_rows: usize,
                                layout: PadLayout, dtype: PadDtype, pad_value: f32, d_out: *mut c_void, d_lengths: *mut i32,
                                stream: *mut c_void) -> Result<(), Error> {
    check(ss_pad_packed_device(d_vec, n_clips, d_row_offsets, total_rows, cols, max_rows, layout as c_int, dtype as c_int, pad_value, d_out,
                               d_lengths, stream))
}

/// The SpecAugment policy of one call: `n_time` spans of at most `min(max_time_width, time_ratio * T_b)` rows and `n_freq` spans of at
/// most `max_freq_width` columns of every clip are overwritten with `mask_value` (written as its bit pattern).  `clip_base` is the id
/// of clip 0: a shard that starts at global clip `clip_base` draws what the whole batch would.
#[derive(Clone, Copy, Debug, PartialEq)]
pub struct SpecAugPolicy {
    pub n_time: usize,
    pub max_time_width: usize,
    pub time_ratio: f32,
    pub n_freq: usize,
    pub max_freq_width: usize,
    pub mask_value: f32,
    pub clip_base: usize,
}

impl Default for SpecAugPolicy {
    /// The LibriSpeech policy: 2 x 100 rows, 2 x 27 columns, no cap by length, zeros.
    fn default() -> Self {
        SpecAugPolicy { n_time: 2, max_time_width: 100, time_ratio: 1.0, n_freq: 2, max_freq_width: 27, mask_value: 0.0, clip_base: 0 }
    }
}

/// The spans `try_spec_augment_packed` draws for `rng = [seed, epoch]`, computed on the host (no device): `(start, width)` pairs,
/// `[n_clips x (n_time + n_freq) x 2]`, time masks first; a bad segment of the table has `(-1, 0)` in every span.
pub fn try_spec_augment_spans(rng: [u64; 2], row_offsets: &[i64], total_rows: usize, cols: usize, policy: &SpecAugPolicy) -> Result<Vec<i32>, Error> {
    if row_offsets.is_empty() {
        return Err(Error { status: SS_ERR_ARG, detail: "spec_augment_spans: row_offsets must not be empty".to_string() });
    }
    let n_clips = row_offsets.len() - 1;
    let mut spans = vec![0i32; n_clips * (policy.n_time + policy.n_freq) * 2];
    check(unsafe {
        ss_specaug_spans(rng.as_ptr(), policy.clip_base, n_clips, row_offsets.as_ptr(), total_rows, cols, policy.n_time, policy.max_time_width,
                         policy.time_ratio, policy.n_freq, policy.max_freq_width, spans.as_mut_ptr())
    })?;
    Ok(spans)
}

/// Overwrite the spans of `spans` (`[n_clips x (n_time + n_freq) x 2]`, time spans first) in every clip of a packed block with
/// `mask_value`; a span outside its clip is skipped whole.  Every other element is a bit copy.
pub fn try_mask_spans_packed(vec: ArrayView2<f32>, row_offsets: &[i64], spans: &[i32], n_time: usize, n_freq: usize,
                             mask_value: f32) -> Result<Array2<f32>, Error> {
    let x = vec.as_standard_layout();
    let (rows, cols) = x.dim();
    if row_offsets.is_empty() || spans.len() != (row_offsets.len() - 1) * (n_time + n_freq) * 2 {
        return Err(Error { status: SS_ERR_ARG, detail: "mask_spans_packed: row_offsets or spans have the wrong length".to_string() });
    }
    let mut out = x.to_owned();
    check(unsafe {
        ss_mask_spans_packed(x.as_ptr(), row_offsets.len() - 1, row_offsets.as_ptr(), rows, cols, spans.as_ptr(), n_time, n_freq, mask_value,
                             out.as_mut_ptr())
    })?;
    Ok(out)
}

/// SpecAugment of every clip of a packed block: the masked block and the spans that were applied.  `rng = [seed, epoch]`; the call
/// advances `rng[1]` by one, so the next call draws other masks.
pub fn try_spec_augment_packed(vec: ArrayView2<f32>, row_offsets: &[i64], rng: &mut [u64; 2],
                               policy: &SpecAugPolicy) -> Result<(Array2<f32>, Vec<i32>), Error> {
    let x = vec.as_standard_layout();
    let (rows, cols) = x.dim();
    if row_offsets.is_empty() {
        return Err(Error { status: SS_ERR_ARG, detail: "spec_augment_packed: row_offsets must not be empty".to_string() });
    }
    let n_clips = row_offsets.len() - 1;
    let mut out = x.to_owned();
    let mut spans = vec![0i32; n_clips * (policy.n_time + policy.n_freq) * 2];
    check(unsafe {
        ss_specaug_packed(x.as_ptr(), n_clips, row_offsets.as_ptr(), rows, cols, rng.as_mut_ptr(), policy.clip_base, policy.n_time,
                          policy.max_time_width, policy.time_ratio, policy.n_freq, policy.max_freq_width, policy.mask_value, out.as_mut_ptr(),
                          spans.as_mut_ptr())
    })?;
    Ok((out, spans))
}

/// The plan launch alone (include/speechsauce_amd.h has the contract): writes the spans table, does not touch the epoch.
///
/// # Safety
/// As `vad_energy_packed_device`; `d_rng` is the 16-byte device block `{seed, epoch}`, `d_spans` holds `n_clips * (n_time + n_freq)` pairs.
pub unsafe fn spec_augment_plan_packed_device(d_rng: *const u64, n_clips: usize, d_row_offsets: *const i64, total_rows: usize, cols: usize,
                                              policy: &SpecAugPolicy, d_spans: *mut i32, stream: *mut c_void) -> Result<(), Error> {
    check(ss_specaug_plan_packed_device(d_rng, policy.clip_base, n_clips, d_row_offsets, total_rows, cols, policy.n_time, policy.max_time_width,
                                        policy.time_ratio, policy.n_freq, policy.max_freq_width, d_spans, stream))
}

/// The apply launch alone, on any spans table; `d_out == d_vec` masks in place.
///
/// # Safety
/// As `spec_augment_plan_packed_device`; `d_out` holds `total_rows * cols` floats and is `d_vec` itself or does not overlap it.
pub unsafe fn mask_spans_packed_device(d_vec: *const f32, n_clips: usize, d_row_offsets: *const i64, total_rows: usize, cols: usize,
                                       d_spans: *const i32, n_time: usize, n_freq: usize, mask_value: f32, d_out: *mut f32,
                                       stream: *mut c_void) -> Result<(), Error> {
    check(ss_mask_spans_packed_device(d_vec, n_clips, d_row_offsets, total_rows, cols, d_spans, n_time, n_freq, mask_value, d_out, stream))
}

/// Plan, apply and the epoch bump: two asynchronous launches on `stream`, nothing read back; replays of a captured graph draw fresh masks.
///
/// # Safety
/// As `mask_spans_packed_device`; one `d_rng` block serves one stream of calls (concurrent calls on one block race on its epoch).
pub unsafe fn spec_augment_packed_device(d_vec: *const f32, n_clips: usize, d_row_offsets: *const i64, total_rows: usize, cols: usize,
                                         d_rng: *mut u64, policy: &SpecAugPolicy, d_out: *mut f32, d_spans: *mut i32,
                                         stream: *mut c_void) -> Result<(), Error> {
    check(ss_specaug_packed_device(d_vec, n_clips, d_row_offsets, total_rows, cols, d_rng, policy.clip_base, policy.n_time, policy.max_time_width,
                                   policy.time_ratio, policy.n_freq, policy.max_freq_width, policy.mask_value, d_out, d_spans, stream))
}

/// One row of a noise-mix plan (`ss_noise_plan_row`): 40 bytes, 8-byte aligned.  `noise_clip` is the bank's clip, -1 for a clip that is
/// not mixed and -2 for a bad speech segment; the gains are what the mix multiplies by, the energies the f64 sums they were formed from.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq)]
pub struct NoisePlanRow {
    pub noise_clip: i32,
    pub start: i32,
    pub snr_db: f32,
    pub gain_db: f32,
    pub speech_gain: f32,
    pub noise_gain: f32,
    pub speech_energy: f64,
    pub noise_energy: f64,
}

/// The draws of one noise-mix call: a clip is mixed with probability `prob` at an SNR drawn from `snr_db` and scaled by a gain drawn
/// from `gain_db` (both `(low, high)` in dB; `(0, 0)`: no gain perturbation).  `clip_base` is the id of clip 0.
#[derive(Clone, Copy, Debug, PartialEq)]
pub struct NoisePolicy {
    pub prob: f32,
    pub snr_db: (f32, f32),
    pub gain_db: (f32, f32),
    pub clip_base: usize,
}

impl Default for NoisePolicy {
    fn default() -> Self {
        NoisePolicy { prob: 1.0, snr_db: (10.0, 30.0), gain_db: (0.0, 0.0), clip_base: 0 }
    }
}

fn noise_tables_ok(sample_offsets: &[i64], noise_offsets: &[i64], what: &str) -> Result<(), Error> {
    if sample_offsets.is_empty() || noise_offsets.is_empty() {
        return Err(Error { status: SS_ERR_ARG, detail: format!("{}: an offset table has n + 1 entries", what) });
    }
    Ok(())
}

/// The draw fields `try_noise_mix_packed` writes for `rng = [seed, epoch]`, computed on the host (no device); gains and energies are 0.
pub fn try_noise_draws(rng: [u64; 2], sample_offsets: &[i64], total_samples: usize, noise_offsets: &[i64], total_noise: usize,
                       policy: &NoisePolicy) -> Result<Vec<NoisePlanRow>, Error> {
    noise_tables_ok(sample_offsets, noise_offsets, "noise_draws")?;
    let mut plan = vec![NoisePlanRow::default(); sample_offsets.len() - 1];
    check(unsafe {
        ss_noise_draws(rng.as_ptr(), policy.clip_base, plan.len(), sample_offsets.as_ptr(), total_samples, noise_offsets.len() - 1,
                       noise_offsets.as_ptr(), total_noise, policy.prob, policy.snr_db.0, policy.snr_db.1, policy.gain_db.0, policy.gain_db.1,
                       plan.as_mut_ptr())
    })?;
    Ok(plan)
}

/// Bytes of the caller-owned scratch of the device plan and mix forms.
pub fn try_noise_mix_work_bytes(n_clips: usize, total_samples: usize) -> Result<usize, Error> {
    let mut n = 0usize;
    check(unsafe { ss_noise_mix_work_bytes(n_clips, total_samples, &mut n) })?;
    Ok(n)
}

/// The mix alone on any plan table: `out[i] = fma(noise_gain, noise[(start + i) mod N], speech_gain * x[i])` of every clip.
pub fn try_noise_apply_packed(x: &[f32], sample_offsets: &[i64], bank: &[f32], noise_offsets: &[i64],
                              plan: &[NoisePlanRow]) -> Result<Vec<f32>, Error> {
    noise_tables_ok(sample_offsets, noise_offsets, "noise_apply_packed")?;
    if plan.len() != sample_offsets.len() - 1 {
        return Err(Error { status: SS_ERR_ARG, detail: "noise_apply_packed: the plan holds one row per clip".to_string() });
    }
    let mut out = x.to_vec();
    if !x.is_empty() {
        check(unsafe {
            ss_noise_apply_packed(x.as_ptr(), plan.len(), sample_offsets.as_ptr(), x.len(), bank.as_ptr(), noise_offsets.len() - 1,
                                  noise_offsets.as_ptr(), bank.len(), plan.as_ptr(), out.as_mut_ptr())
        })?;
    }
    Ok(out)
}

/// As `try_noise_apply_packed` on 16-bit PCM: a sample is `pcm * scale`, both scales powers of two; the output is float.
pub fn try_noise_apply_packed_i16(x: &[i16], x_scale: f32, sample_offsets: &[i64], bank: &[i16], noise_scale: f32, noise_offsets: &[i64],
                                  plan: &[NoisePlanRow]) -> Result<Vec<f32>, Error> {
    noise_tables_ok(sample_offsets, noise_offsets, "noise_apply_packed_i16")?;
    if plan.len() != sample_offsets.len() - 1 {
        return Err(Error { status: SS_ERR_ARG, detail: "noise_apply_packed_i16: the plan holds one row per clip".to_string() });
    }
    let mut out: Vec<f32> = x.iter().map(|&v| v as f32 * x_scale).collect();
    if !x.is_empty() {
        check(unsafe {
            ss_noise_apply_packed_i16(x.as_ptr(), x_scale, plan.len(), sample_offsets.as_ptr(), x.len(), bank.as_ptr(), noise_scale,
                                      noise_offsets.len() - 1, noise_offsets.as_ptr(), bank.len(), plan.as_ptr(), out.as_mut_ptr())
        })?;
    }
    Ok(out)
}

/// Additive noise at a drawn SNR and gain perturbation of every clip of a packed signal: the mixed samples and the plan that was
/// applied.  `rng = [seed, epoch]`; the call advances `rng[1]` by one, so the next call draws other noise.
pub fn try_noise_mix_packed(x: &[f32], sample_offsets: &[i64], bank: &[f32], noise_offsets: &[i64], rng: &mut [u64; 2],
                            policy: &NoisePolicy) -> Result<(Vec<f32>, Vec<NoisePlanRow>), Error> {
    noise_tables_ok(sample_offsets, noise_offsets, "noise_mix_packed")?;
    let mut out = x.to_vec();
    let mut plan = vec![NoisePlanRow::default(); sample_offsets.len() - 1];
    if !x.is_empty() {
        check(unsafe {
            ss_noise_mix_packed(x.as_ptr(), plan.len(), sample_offsets.as_ptr(), x.len(), bank.as_ptr(), noise_offsets.len() - 1,
                                noise_offsets.as_ptr(), bank.len(), rng.as_mut_ptr(), policy.clip_base, policy.prob, policy.snr_db.0,
                                policy.snr_db.1, policy.gain_db.0, policy.gain_db.1, out.as_mut_ptr(), plan.as_mut_ptr())
        })?;
    }
    Ok((out, plan))
}

/// As `try_noise_mix_packed` on 16-bit PCM (see `try_noise_apply_packed_i16`).
pub fn try_noise_mix_packed_i16(x: &[i16], x_scale: f32, sample_offsets: &[i64], bank: &[i16], noise_scale: f32, noise_offsets: &[i64],
                                rng: &mut [u64; 2], policy: &NoisePolicy) -> Result<(Vec<f32>, Vec<NoisePlanRow>), Error> {
    noise_tables_ok(sample_offsets, noise_offsets, "noise_mix_packed_i16")?;
    let mut out: Vec<f32> = x.iter().map(|&v| v as f32 * x_scale).collect();
    let mut plan = vec![NoisePlanRow::default(); sample_offsets.len() - 1];
    if !x.is_empty() {
        check(unsafe {
            ss_noise_mix_packed_i16(x.as_ptr(), x_scale, plan.len(), sample_offsets.as_ptr(), x.len(), bank.as_ptr(), noise_scale,
                                    noise_offsets.len() - 1, noise_offsets.as_ptr(), bank.len(), rng.as_mut_ptr(), policy.clip_base, policy.prob,
                                    policy.snr_db.0, policy.snr_db.1, policy.gain_db.0, policy.gain_db.1, out.as_mut_ptr(), plan.as_mut_ptr())
        })?;
    }
    Ok((out, plan))
}

/// The device tables of a noise-mix call: packed speech (`total_samples` samples, `n_clips + 1` offsets) and the bank.
#[derive(Clone, Copy, Debug)]
pub struct NoiseDeviceBlocks<T> {
    pub d_x: *const T,
    pub n_clips: usize,
    pub d_sample_offsets: *const i64,
    pub total_samples: usize,
    pub d_bank: *const T,
    pub n_noise: usize,
    pub d_noise_offsets: *const i64,
    pub total_noise: usize,
}

/// Draws, energies and gains into `d_plan` (include/speechsauce_amd.h has the contract); the epoch is not touched.
///
/// # Safety
/// As `vad_energy_packed_device`; `d_rng` is the 16-byte device block `{seed, epoch}`, `d_plan` holds `n_clips` rows and `d_work`
/// `work_bytes >= try_noise_mix_work_bytes(n_clips, total_samples)` bytes, 8-byte aligned.
pub unsafe fn noise_plan_packed_device(b: &NoiseDeviceBlocks<f32>, d_rng: *const u64, policy: &NoisePolicy, d_plan: *mut NoisePlanRow,
                                       d_work: *mut c_void, work_bytes: usize, stream: *mut c_void) -> Result<(), Error> {
    check(ss_noise_plan_packed_device(b.d_x, b.n_clips, b.d_sample_offsets, b.total_samples, b.d_bank, b.n_noise, b.d_noise_offsets, b.total_noise,
                                      d_rng, policy.clip_base, policy.prob, policy.snr_db.0, policy.snr_db.1, policy.gain_db.0, policy.gain_db.1,
                                      d_plan, d_work, work_bytes, stream))
}

/// As `noise_plan_packed_device` on 16-bit PCM.
///
/// # Safety
/// As `noise_plan_packed_device`.
pub unsafe fn noise_plan_packed_i16_device(b: &NoiseDeviceBlocks<i16>, x_scale: f32, noise_scale: f32, d_rng: *const u64, policy: &NoisePolicy,
                                           d_plan: *mut NoisePlanRow, d_work: *mut c_void, work_bytes: usize,
                                           stream: *mut c_void) -> Result<(), Error> {
    check(ss_noise_plan_packed_i16_device(b.d_x, x_scale, b.n_clips, b.d_sample_offsets, b.total_samples, b.d_bank, noise_scale, b.n_noise,
                                          b.d_noise_offsets, b.total_noise, d_rng, policy.clip_base, policy.prob, policy.snr_db.0, policy.snr_db.1,
                                          policy.gain_db.0, policy.gain_db.1, d_plan, d_work, work_bytes, stream))
}

/// The mix alone, on any plan table; `d_out == d_x` mixes in place.
///
/// # Safety
/// As `noise_plan_packed_device`; `d_out` holds `total_samples` floats and is `d_x` itself or does not overlap it.
pub unsafe fn noise_apply_packed_device(b: &NoiseDeviceBlocks<f32>, d_plan: *const NoisePlanRow, d_out: *mut f32,
                                        stream: *mut c_void) -> Result<(), Error> {
    check(ss_noise_apply_packed_device(b.d_x, b.n_clips, b.d_sample_offsets, b.total_samples, b.d_bank, b.n_noise, b.d_noise_offsets, b.total_noise,
                                       d_plan, d_out, stream))
}

/// As `noise_apply_packed_device` on 16-bit PCM; `d_out` is float and overlaps nothing.
///
/// # Safety
/// As `noise_apply_packed_device`.
pub unsafe fn noise_apply_packed_i16_device(b: &NoiseDeviceBlocks<i16>, x_scale: f32, noise_scale: f32, d_plan: *const NoisePlanRow,
                                            d_out: *mut f32, stream: *mut c_void) -> Result<(), Error> {
    check(ss_noise_apply_packed_i16_device(b.d_x, x_scale, b.n_clips, b.d_sample_offsets, b.total_samples, b.d_bank, noise_scale, b.n_noise,
                                           b.d_noise_offsets, b.total_noise, d_plan, d_out, stream))
}

/// Plan, apply and the epoch bump: three asynchronous launches on `stream`, nothing read back; replays of a captured graph draw fresh noise.
///
/// # Safety
/// As `noise_apply_packed_device` and `noise_plan_packed_device`; one `d_rng` block serves one stream of calls.
pub unsafe fn noise_mix_packed_device(b: &NoiseDeviceBlocks<f32>, d_rng: *mut u64, policy: &NoisePolicy, d_out: *mut f32,
                                      d_plan: *mut NoisePlanRow, d_work: *mut c_void, work_bytes: usize,
                                      stream: *mut c_void) -> Result<(), Error> {
    check(ss_noise_mix_packed_device(b.d_x, b.n_clips, b.d_sample_offsets, b.total_samples, b.d_bank, b.n_noise, b.d_noise_offsets, b.total_noise,
                                     d_rng, policy.clip_base, policy.prob, policy.snr_db.0, policy.snr_db.1, policy.gain_db.0, policy.gain_db.1, d_out,
                                     d_plan, d_work, work_bytes, stream))
}

/// As `noise_mix_packed_device` on 16-bit PCM.
///
/// # Safety
/// As `noise_mix_packed_device`.
pub unsafe fn noise_mix_packed_i16_device(b: &NoiseDeviceBlocks<i16>, x_scale: f32, noise_scale: f32, d_rng: *mut u64, policy: &NoisePolicy,
                                          d_out: *mut f32, d_plan: *mut NoisePlanRow, d_work: *mut c_void, work_bytes: usize,
                                          stream: *mut c_void) -> Result<(), Error> {
    check(ss_noise_mix_packed_i16_device(b.d_x, x_scale, b.n_clips, b.d_sample_offsets, b.total_samples, b.d_bank, noise_scale, b.n_noise,
                                         b.d_noise_offsets, b.total_noise, d_rng, policy.clip_base, policy.prob, policy.snr_db.0, policy.snr_db.1,
                                         policy.gain_db.0, policy.gain_db.1, d_out, d_plan, d_work, work_bytes, stream))
}

/// librosa's power_to_db of every clip of a packed block with the clip's own `top_db` floor (`None`: no floor); clip b's segment
/// is elements `cols * offsets[b] .. cols * offsets[b + 1]` of `s`.
pub fn try_power_to_db_packed(s: ArrayView2<f32>, offsets: &[i64], ref_value: f32, amin: f32, top_db: Option<f32>) -> Result<Array2<f32>, Error> {
    let x = s.as_standard_layout();
    let (rows, cols) = x.dim();
    let mut out = Array2::<f32>::zeros((rows, cols));
    check(unsafe {
        ss_power_to_db_packed(x.as_ptr(), offsets.len().saturating_sub(1), offsets.as_ptr(), rows, cols, ref_value, amin,
                              top_db.unwrap_or(-1.0), out.as_mut_ptr())
    })?;
    Ok(out)
}

/// processing.rs:222-254
pub fn derivative_extraction(feat: &Array2<f32>, delta_windows: usize) -> Array2<f32> {
    let x = feat.as_standard_layout();
    let (rows, cols) = x.dim();
    let mut out = Array2::<f32>::zeros((rows, cols));
    check(unsafe { ss_derivative_extraction(x.as_ptr(), rows, cols, delta_windows, out.as_mut_ptr()) }).expect("derivative_extraction");
    out
}

/// feature.rs:253-269: N x M x 3 cube of static, first and second derivative features
pub fn extract_derivative_feature(feature: Array2<f32>) -> Array3<f32> {
    let x = feature.as_standard_layout();
    let (rows, cols) = x.dim();
    let mut cube = Array3::<f32>::zeros((rows, cols, 3));
    check(unsafe { ss_extract_derivative_feature(x.as_ptr(), rows, cols, cube.as_mut_ptr()) }).expect("extract_derivative_feature");
    cube
}

// ---------------------------------------------------------------------------------------------------------------------------
// Scalar helpers the reference exports from `functions` (functions.rs:19-71) and `util` (util.rs:372-381): host arithmetic on a
// handful of values, written here in plain Rust (nothing to launch a kernel for); the filterbank the kernels use is built by the
// library from the same formulas in the same f32 operation order (ss_filterbank).
// ---------------------------------------------------------------------------------------------------------------------------

/// functions.rs:19-21: Hz -> mel, 1127 ln(1 + f / 700)
pub fn frequency_to_mel(f: f32) -> f32 { 1127.0 * (1.0 + f / 700.0).ln() }
/// functions.rs:23-29
pub fn frequency_arr_to_mel<D: Dimension>(freq: Array<f32, D>) -> Array<f32, D> { freq.mapv(frequency_to_mel) }
/// functions.rs:31-34 (the reference's unused type parameter is kept so `mel_to_frequency::<Ix1>(m)` still compiles)
pub fn mel_to_frequency<D>(mel: f32) -> f32 { 700.0 * ((mel / 1127.0).exp() - 1.0) }
/// functions.rs:36-41
pub fn mel_arr_to_frequency<D: Dimension>(mel: Array<f32, D>) -> Array<f32, D> { mel.mapv(|m| 700.0 * ((m / 1127.0).exp() - 1.0)) }
/// functions.rs:43-60: triangular weight over the half-open range [left, right); at x == middle the falling branch wins (= 1)
pub fn triangle(arr: Array1<f32>, left: f32, middle: f32, right: f32) -> Array1<f32> {
    arr.mapv(|x| {
        if !(x >= left && x < right) {
            return 0.0;
        }
        let mut w = 0.0;
        if x <= middle { w = (x - left) / (middle - left); }
        if x >= middle { w = (right - x) / (right - middle); }
        w
    })
}
/// functions.rs:66-71: exact zeros become f32::EPSILON
pub fn zero_handling<D: Dimension>(x: Array<f32, D>) -> Array<f32, D> { x.mapv(|v| if v == 0.0 { f32::EPSILON } else { v }) }

/// util.rs:372-381: natural logarithm of every element, in place.  Two type parameters with the reference's bounds, so that caller
/// code naming `ArrayLog<f32, Ix2>` (or bounding on it) resolves unchanged.
pub trait ArrayLog<A: num_traits::real::Real, I: Dimension> {
    fn log(self) -> Array<A, I>;
}
impl<A: num_traits::real::Real, I: Dimension> ArrayLog<A, I> for Array<A, I> {
    fn log(mut self) -> Array<A, I> {
        self.map_inplace(|n| *n = (*n).ln());
        self
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// The reference's module paths (speechsauce/src/lib.rs:2-6).  Re-exports only: one implementation, two spellings.
// ---------------------------------------------------------------------------------------------------------------------------

/// `ss_kaldi_params`: the Kaldi-compatible front end's parameters (field order is ABI; see `ss_kaldi_*` in the C header).
/// `KaldiParams::new` fills torchaudio's defaults.
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct KaldiParams {
    pub struct_size: u32,
    pub sample_rate: u32,
    pub frame_length_ms: f32,
    pub frame_shift_ms: f32,
    pub num_mel_bins: u32,
    pub num_ceps: u32,
    pub low_freq: f32,
    pub high_freq: f32,
    pub preemph_coef: f32,
    pub cepstral_lifter: f32,
    pub window_type: i32,
    pub blackman_coeff: f32,
    pub remove_dc_offset: i32,
    pub use_power: i32,
    pub use_energy: i32,
    pub raw_energy: i32,
    pub energy_floor: f32,
    pub input_scale: f32,
    pub dither: f32,
}

impl KaldiParams {
    pub fn new(sample_rate: u32) -> KaldiParams {
        let mut p: KaldiParams = unsafe { std::mem::zeroed() };
        unsafe { ss_kaldi_params_default(&mut p, sample_rate) };
        p
    }
}

/// Kaldi's `compute-fbank-feats` / `compute-mfcc-feats` (as `torchaudio.compliance.kaldi` restates them) for frames that pad to 512
/// points.  Not in the reference crate.  Owns an `ss_kaldi_config`.
pub struct KaldiFrontEnd {
    raw: *mut c_void,
    params: KaldiParams,
}

unsafe impl Send for KaldiFrontEnd {}
unsafe impl Sync for KaldiFrontEnd {}

impl Drop for KaldiFrontEnd {
    fn drop(&mut self) {
        unsafe { ss_kaldi_config_destroy(self.raw) }
    }
}

impl KaldiFrontEnd {
    pub fn new(params: KaldiParams) -> Result<KaldiFrontEnd, Error> {
        let mut raw: *mut c_void = std::ptr::null_mut();
        check(unsafe { ss_kaldi_config_create(&params, &mut raw) })?;
        Ok(KaldiFrontEnd { raw, params })
    }

    pub fn num_frames(&self, n_samples: usize) -> Result<usize, Error> {
        let mut t = 0usize;
        check(unsafe { ss_kaldi_num_frames(&self.params, n_samples, &mut t) })?;
        Ok(t)
    }

    /// One clip -> (`[T x num_mel_bins]` log-mel rows, `[T]` log energies).
    pub fn fbank(&self, x: &[f32]) -> Result<(Array2<f32>, Vec<f32>), Error> {
        let t = self.num_frames(x.len())?;
        let mut out = Array2::<f32>::zeros((t, self.params.num_mel_bins as usize));
        let mut en = vec![0f32; t];
        check(unsafe { ss_kaldi_fbank(self.raw, x.as_ptr(), 1, x.len(), x.len(), out.as_mut_ptr(), en.as_mut_ptr()) })?;
        Ok((out, en))
    }

    /// One clip -> `[T x num_ceps]` cepstra.
    pub fn mfcc(&self, x: &[f32]) -> Result<Array2<f32>, Error> {
        let t = self.num_frames(x.len())?;
        let mut out = Array2::<f32>::zeros((t, self.params.num_ceps as usize));
        check(unsafe { ss_kaldi_mfcc(self.raw, x.as_ptr(), 1, x.len(), x.len(), out.as_mut_ptr()) })?;
        Ok(out)
    }

    /// Frame offsets of packed clips (`ss_kaldi_packed_frame_offsets`).
    pub fn packed_frame_offsets(&self, sample_offsets: &[i64]) -> Result<Vec<i64>, Error> {
        if sample_offsets.is_empty() {
            return Err(Error { status: SS_ERR_ARG, detail: "sample_offsets must not be empty".to_string() });
        }
        let mut fo = vec![0i64; sample_offsets.len()];
        check(unsafe { ss_kaldi_packed_frame_offsets(&self.params, sample_offsets.len() - 1, sample_offsets.as_ptr(), fo.as_mut_ptr()) })?;
        Ok(fo)
    }

    /// Clips packed end to end -> (the `[sum T_b x num_mel_bins]` rows, the `[sum T_b]` log energies, the frame offsets); one launch.
    pub fn fbank_packed(&self, x: &[f32], sample_offsets: &[i64]) -> Result<(Array2<f32>, Vec<f32>, Vec<i64>), Error> {
        let fo = self.packed_frame_offsets(sample_offsets)?;
        if sample_offsets[sample_offsets.len() - 1] as usize > x.len() {
            return Err(Error { status: SS_ERR_ARG, detail: "sample_offsets ends past the block".to_string() });
        }
        let rows = fo[fo.len() - 1] as usize;
        let mut out = Array2::<f32>::zeros((rows, self.params.num_mel_bins as usize));
        let mut en = vec![0f32; rows];
        check(unsafe { ss_kaldi_fbank_packed(self.raw, x.as_ptr(), fo.len() - 1, sample_offsets.as_ptr(), out.as_mut_ptr(), en.as_mut_ptr()) })?;
        Ok((out, en, fo))
    }

    /// Clips packed end to end -> (the `[sum T_b x num_ceps]` cepstra, the frame offsets); one launch.
    pub fn mfcc_packed(&self, x: &[f32], sample_offsets: &[i64]) -> Result<(Array2<f32>, Vec<i64>), Error> {
        let fo = self.packed_frame_offsets(sample_offsets)?;
        if sample_offsets[sample_offsets.len() - 1] as usize > x.len() {
            return Err(Error { status: SS_ERR_ARG, detail: "sample_offsets ends past the block".to_string() });
        }
        let mut out = Array2::<f32>::zeros((fo[fo.len() - 1] as usize, self.params.num_ceps as usize));
        check(unsafe { ss_kaldi_mfcc_packed(self.raw, x.as_ptr(), fo.len() - 1, sample_offsets.as_ptr(), out.as_mut_ptr()) })?;
        Ok((out, fo))
    }

    /// The stream pool's sizes (`ss_kstream_state_len`): (S, the carried samples per stream = the floats of a pool row; D, the
    /// warm-up rows after a reset).
    pub fn stream_state_len(&self) -> Result<(usize, usize), Error> {
        let (mut s, mut d) = (0usize, 0usize);
        check(unsafe { ss_kstream_state_len(&self.params, &mut s, &mut d) })?;
        Ok((s, d))
    }

    /// Row offsets of the entries of a pool call (`ss_kstream_row_offsets`): every chunk is whole hops.
    pub fn stream_row_offsets(&self, sample_offsets: &[i64]) -> Result<Vec<i64>, Error> {
        if sample_offsets.is_empty() {
            return Err(Error { status: SS_ERR_ARG, detail: "sample_offsets must not be empty".to_string() });
        }
        let mut ro = vec![0i64; sample_offsets.len()];
        check(unsafe { ss_kstream_row_offsets(&self.params, sample_offsets.len() - 1, sample_offsets.as_ptr(), ro.as_mut_ptr()) })?;
        Ok(ro)
    }

    // the checks the pool wrappers share: the tables against the block and the pool -> (row offsets, pool rows)
    fn stream_shape<T>(&self, x: &[T], sample_offsets: &[i64], slots: &[i32], pool: &[f32]) -> Result<(Vec<i64>, usize), Error> {
        let ro = self.stream_row_offsets(sample_offsets)?;
        let (s, _) = self.stream_state_len()?;
        if slots.len() != sample_offsets.len() - 1 || sample_offsets[sample_offsets.len() - 1] as usize > x.len() {
            return Err(Error { status: SS_ERR_ARG, detail: "pool call: shape mismatch".to_string() });
        }
        if s > 0 && (pool.is_empty() || pool.len() % s != 0) {
            return Err(Error { status: SS_ERR_ARG, detail: "pool call: the pool is not a whole number of rows".to_string() });
        }
        // (s == 0: a pool without state; one row stands for any slot count the caller uses)
        Ok((ro, if s > 0 { pool.len() / s } else { (slots.iter().copied().max().unwrap_or(0).max(0) as usize) + 1 }))
    }

    /// Ragged streaming fbank over a pool of stream states (`ss_kstream_fbank_packed`): entry i is the chunk
    /// `x[sample_offsets[i] .. sample_offsets[i+1])` (whole hops) of the stream whose state is pool row `slots[i]`; `pool` is
    /// `[pool_streams x S]`, all-zero rows are fresh streams.  -> (rows, log energies, row offsets); the first D rows of a fresh
    /// stream are warm-up rows.
    pub fn fbank_stream_packed(&self, x: &[f32], sample_offsets: &[i64], slots: &[i32], pool: &mut [f32]) -> Result<(Array2<f32>, Vec<f32>, Vec<i64>), Error> {
        let (ro, pool_streams) = self.stream_shape(x, sample_offsets, slots, pool)?;
        let rows = ro[ro.len() - 1] as usize;
        let mut out = Array2::<f32>::zeros((rows, self.params.num_mel_bins as usize));
        let mut en = vec![0f32; rows];
        check(unsafe {
            ss_kstream_fbank_packed(self.raw, x.as_ptr(), slots.len(), sample_offsets.as_ptr(), slots.as_ptr(), pool_streams, pool.as_mut_ptr(),
                                    out.as_mut_ptr(), en.as_mut_ptr())
        })?;
        Ok((out, en, ro))
    }

    /// Ragged streaming MFCC over a pool of stream states (`ss_kstream_mfcc_packed`); see `fbank_stream_packed`.
    pub fn mfcc_stream_packed(&self, x: &[f32], sample_offsets: &[i64], slots: &[i32], pool: &mut [f32]) -> Result<(Array2<f32>, Vec<i64>), Error> {
        let (ro, pool_streams) = self.stream_shape(x, sample_offsets, slots, pool)?;
        let mut out = Array2::<f32>::zeros((ro[ro.len() - 1] as usize, self.params.num_ceps as usize));
        check(unsafe {
            ss_kstream_mfcc_packed(self.raw, x.as_ptr(), slots.len(), sample_offsets.as_ptr(), slots.as_ptr(), pool_streams, pool.as_mut_ptr(),
                                   out.as_mut_ptr())
        })?;
        Ok((out, ro))
    }

    /// `fbank_stream_packed` fed signed 16-bit PCM: sample = `pcm as f32 * scale`, `scale` a power of two (`ss_kstream_fbank_packed_i16`).
    pub fn fbank_stream_packed_i16(&self, x: &[i16], sample_offsets: &[i64], slots: &[i32], scale: f32, pool: &mut [f32])
                                   -> Result<(Array2<f32>, Vec<f32>, Vec<i64>), Error> {
        let (ro, pool_streams) = self.stream_shape(x, sample_offsets, slots, pool)?;
        let rows = ro[ro.len() - 1] as usize;
        let mut out = Array2::<f32>::zeros((rows, self.params.num_mel_bins as usize));
        let mut en = vec![0f32; rows];
        check(unsafe {
            ss_kstream_fbank_packed_i16(self.raw, x.as_ptr(), slots.len(), sample_offsets.as_ptr(), slots.as_ptr(), pool_streams, scale,
                                        pool.as_mut_ptr(), out.as_mut_ptr(), en.as_mut_ptr())
        })?;
        Ok((out, en, ro))
    }

    /// `mfcc_stream_packed` fed signed 16-bit PCM (`ss_kstream_mfcc_packed_i16`).
    pub fn mfcc_stream_packed_i16(&self, x: &[i16], sample_offsets: &[i64], slots: &[i32], scale: f32, pool: &mut [f32])
                                  -> Result<(Array2<f32>, Vec<i64>), Error> {
        let (ro, pool_streams) = self.stream_shape(x, sample_offsets, slots, pool)?;
        let mut out = Array2::<f32>::zeros((ro[ro.len() - 1] as usize, self.params.num_ceps as usize));
        check(unsafe {
            ss_kstream_mfcc_packed_i16(self.raw, x.as_ptr(), slots.len(), sample_offsets.as_ptr(), slots.as_ptr(), pool_streams, scale,
                                       pool.as_mut_ptr(), out.as_mut_ptr())
        })?;
        Ok((out, ro))
    }
}

/// `ss_resample_info`: the sizes of one conversion (see `ss_resample_sizes` in the C header).
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct ResampleInfo {
    pub o: u32,
    pub n: u32,
    pub width: u32,
    pub taps: u32,
    pub lookback: u32,
    pub lookahead: u32,
    pub latency_periods: u32,
    pub tile_outputs: u32,
}

/// An affine transform `[out_dim x in_dim]` (+ bias) applied behind the splice stage without the spliced block ever being written:
/// Kaldi's `splice-feats | transform-feats` (LDA / LDA+MLLT), a PCA matrix, the input projection of a low-frame-rate front end.  Not in
/// the reference crate.  Owns an `ss_affine`; the matrix is uploaded by the first call that runs.
pub struct Affine {
    raw: *mut c_void,
}

unsafe impl Send for Affine {}
unsafe impl Sync for Affine {}

impl Drop for Affine {
    fn drop(&mut self) {
        unsafe { ss_affine_destroy(self.raw) }
    }
}

impl Affine {
    /// `matrix`: row-major `[out_dim x in_dim]` (1 ..= 256 by 1 ..= 4096); `bias`: `[out_dim]`.
    pub fn new(matrix: &[f32], out_dim: usize, in_dim: usize, bias: Option<&[f32]>) -> Result<Affine, Error> {
        if matrix.len() != out_dim * in_dim || bias.map_or(false, |b| b.len() != out_dim) {
            return Err(Error { status: SS_ERR_ARG, detail: "matrix must be out_dim * in_dim floats, bias out_dim".to_string() });
        }
        let mut raw: *mut c_void = std::ptr::null_mut();
        let b = bias.map_or(std::ptr::null(), |b| b.as_ptr());
        check(unsafe { ss_affine_create(matrix.as_ptr(), out_dim, in_dim, in_dim, b, &mut raw) })?;
        Ok(Affine { raw })
    }

    /// `(out_dim, in_dim)`
    pub fn dims(&self) -> Result<(usize, usize), Error> {
        let (mut o, mut i) = (0usize, 0usize);
        check(unsafe { ss_affine_dims(self.raw, &mut o, &mut i) })?;
        Ok((o, i))
    }

    /// `4 * ceil(in_dim / 4)`: the steps of every output element's fmaf chain.
    pub fn chain_len(&self) -> Result<usize, Error> {
        let mut k4 = 0usize;
        check(unsafe { ss_affine_chain_len(self.dims()?.1, &mut k4) })?;
        Ok(k4)
    }

    /// Clips packed end to end (clip b = rows `row_offsets[b] .. row_offsets[b + 1]` of `vec [total_rows x cols]`) -> the block
    /// `[sum ceil(T_b / stride) x out_dim]`: row k of a clip is the transform of its rows `k * stride - left ..= k * stride + right`
    /// side by side, clamped to the clip.  `in_dim` must be `(left + 1 + right) * cols`.
    pub fn splice_packed(&self, vec: &[f32], row_offsets: &[i64], cols: usize, left: usize, right: usize, stride: usize) -> Result<Vec<f32>, Error> {
        if row_offsets.is_empty() || cols == 0 || stride == 0 || vec.len() % cols != 0 {
            return Err(Error { status: SS_ERR_ARG, detail: "splice_packed: shape mismatch".to_string() });
        }
        let s = stride as i64;
        let out_rows: i64 = row_offsets.windows(2).map(|w| if w[1] > w[0] { (w[1] - w[0] + s - 1) / s } else { 0 }).sum();
        let mut out = vec![0f32; out_rows as usize * self.dims()?.0];
        check(unsafe {
            ss_affine_splice_packed(self.raw, vec.as_ptr(), row_offsets.len() - 1, row_offsets.as_ptr(), vec.len() / cols, cols, left, right, stride,
                                    out.as_mut_ptr())
        })?;
        Ok(out)
    }

    /// The device form on device pointers (`d_out_offsets`: `ss_splice_packed_offsets` of the row offsets); asynchronous on `stream`.
    ///
    /// # Safety
    /// Every pointer is a device pointer to a block of the size the header states.
    pub unsafe fn splice_packed_device(&self, d_vec: *const f32, n_clips: usize, d_row_offsets: *const i64, total_rows: usize, d_out_offsets: *const i64,
                                       total_out_rows: usize, cols: usize, left: usize, right: usize, stride: usize, d_out: *mut f32,
                                       stream: *mut c_void) -> Result<(), Error> {
        check(ss_affine_splice_packed_device(self.raw, d_vec, n_clips, d_row_offsets, total_rows, d_out_offsets, total_out_rows, cols, left, right,
                                             stride, d_out, stream))
    }
}

/// One row of a reverberation plan (`ss_reverb_plan_row`): 8 bytes.  `rir` is the bank's response, -1 for a clip that is not reverberated
/// and -2 for a bad speech segment; `shift` is the tap index that lands on the output sample itself.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq)]
pub struct ReverbPlanRow {
    pub rir: i32,
    pub shift: i32,
}

/// How `ReverbBank::new` scales every response: as given, to unit energy, or to a largest magnitude of 1.
#[derive(Clone, Copy, Debug, PartialEq)]
pub enum ReverbNormalize {
    AsGiven = 0,
    UnitEnergy = 1,
    UnitPeak = 2,
}

/// A bank of room impulse responses (1 ..= 16384 taps each) with their partition spectra: the convolution step of the multi-condition
/// recipes, `out[i] = sum_k h[k] * x[i + shift - k]` per clip, the clip's length kept.  Not in the reference crate.  Owns an
/// `ss_reverb_bank`; the spectra are uploaded by the first call that runs.
pub struct ReverbBank {
    raw: *mut c_void,
}

unsafe impl Send for ReverbBank {}
unsafe impl Sync for ReverbBank {}

impl Drop for ReverbBank {
    fn drop(&mut self) {
        unsafe { ss_reverb_bank_destroy(self.raw) }
    }
}

fn reverb_tables_ok(sample_offsets: &[i64], plan_len: Option<usize>, what: &str) -> Result<(), Error> {
    if sample_offsets.is_empty() || plan_len.map_or(false, |n| n != sample_offsets.len() - 1) {
        return Err(Error { status: SS_ERR_ARG, detail: format!("{}: an offset table has n + 1 entries and the plan one row per clip", what) });
    }
    Ok(())
}

impl ReverbBank {
    /// `rirs`: the responses packed; `offsets`: `n_rir + 1` entries from 0.  `align_peak`: the output is shifted by each response's peak
    /// index (the direct path stays where it was) instead of being the head of the full convolution.
    pub fn new(rirs: &[f32], offsets: &[i64], normalize: ReverbNormalize, align_peak: bool) -> Result<ReverbBank, Error> {
        if offsets.is_empty() {
            return Err(Error { status: SS_ERR_ARG, detail: "ReverbBank: an offset table has n + 1 entries".to_string() });
        }
        let mut raw: *mut c_void = std::ptr::null_mut();
        check(unsafe {
            ss_reverb_bank_create(rirs.as_ptr(), offsets.len() - 1, offsets.as_ptr(), rirs.len(), normalize as c_int, align_peak as c_int, &mut raw)
        })?;
        Ok(ReverbBank { raw })
    }

    /// `(n_rir, block, max_taps, n_partitions)`
    pub fn info(&self) -> Result<(usize, usize, usize, usize), Error> {
        let (mut n, mut b, mut k, mut p) = (0usize, 0usize, 0usize, 0usize);
        check(unsafe { ss_reverb_bank_info(self.raw, &mut n, &mut b, &mut k, &mut p) })?;
        Ok((n, b, k, p))
    }

    /// The normalised taps of response `c` exactly as the spectra were made from them, and the first index of their largest magnitude.
    pub fn rir(&self, c: usize) -> Result<(Vec<f32>, usize), Error> {
        let (mut n, mut peak) = (0usize, 0usize);
        check(unsafe { ss_reverb_bank_rir(self.raw, c, std::ptr::null_mut(), 0, &mut n, &mut peak) })?;
        let mut taps = vec![0f32; n];
        check(unsafe { ss_reverb_bank_rir(self.raw, c, taps.as_mut_ptr(), taps.len(), &mut n, &mut peak) })?;
        Ok((taps, peak))
    }

    /// Partition `p` of response `c`: `2 * block` interleaved `(re, im)` pairs, bin 0 first.
    pub fn spectrum(&self, c: usize, p: usize) -> Result<Vec<f32>, Error> {
        let mut out = vec![0f32; 4 * self.info()?.1];
        check(unsafe { ss_reverb_bank_spectrum(self.raw, c, p, out.as_mut_ptr()) })?;
        Ok(out)
    }

    /// The plan `packed` writes for `rng = [seed, epoch]`, computed on the host (no device).
    pub fn draws(&self, rng: [u64; 2], sample_offsets: &[i64], total_samples: usize, prob: f32, clip_base: usize) -> Result<Vec<ReverbPlanRow>, Error> {
        reverb_tables_ok(sample_offsets, None, "reverb_draws")?;
        let mut plan = vec![ReverbPlanRow::default(); sample_offsets.len() - 1];
        check(unsafe {
            ss_reverb_draws(rng.as_ptr(), clip_base, plan.len(), sample_offsets.as_ptr(), total_samples, self.raw, prob, plan.as_mut_ptr())
        })?;
        Ok(plan)
    }

    /// The convolution alone on any plan table; rows with `rir == -1` (or out of range for the bank) are copies.
    pub fn apply_packed(&self, x: &[f32], sample_offsets: &[i64], plan: &[ReverbPlanRow]) -> Result<Vec<f32>, Error> {
        reverb_tables_ok(sample_offsets, Some(plan.len()), "reverb_apply_packed")?;
        let mut out = x.to_vec();
        if !x.is_empty() {
            check(unsafe {
                ss_reverb_apply_packed(x.as_ptr(), plan.len(), sample_offsets.as_ptr(), x.len(), self.raw, plan.as_ptr(), out.as_mut_ptr())
            })?;
        }
        Ok(out)
    }

    /// As `apply_packed` on 16-bit PCM: a sample is `pcm * x_scale`, a power of two; the output is float.
    pub fn apply_packed_i16(&self, x: &[i16], x_scale: f32, sample_offsets: &[i64], plan: &[ReverbPlanRow]) -> Result<Vec<f32>, Error> {
        reverb_tables_ok(sample_offsets, Some(plan.len()), "reverb_apply_packed_i16")?;
        let mut out: Vec<f32> = x.iter().map(|&v| v as f32 * x_scale).collect();
        if !x.is_empty() {
            check(unsafe {
                ss_reverb_apply_packed_i16(x.as_ptr(), x_scale, plan.len(), sample_offsets.as_ptr(), x.len(), self.raw, plan.as_ptr(), out.as_mut_ptr())
            })?;
        }
        Ok(out)
    }

    /// Reverberation of every clip of a packed signal with probability `prob`: the output and the plan that was applied.  The call
    /// advances `rng[1]` by one, so the next call draws afresh.
    pub fn packed(&self, x: &[f32], sample_offsets: &[i64], rng: &mut [u64; 2], prob: f32, clip_base: usize) -> Result<(Vec<f32>, Vec<ReverbPlanRow>), Error> {
        reverb_tables_ok(sample_offsets, None, "reverb_packed")?;
        let mut out = x.to_vec();
        let mut plan = vec![ReverbPlanRow::default(); sample_offsets.len() - 1];
        if !x.is_empty() {
            check(unsafe {
                ss_reverb_packed(x.as_ptr(), plan.len(), sample_offsets.as_ptr(), x.len(), self.raw, rng.as_mut_ptr(), clip_base, prob, out.as_mut_ptr(),
                                 plan.as_mut_ptr())
            })?;
        }
        Ok((out, plan))
    }

    /// As `packed` on 16-bit PCM (see `apply_packed_i16`).
    pub fn packed_i16(&self, x: &[i16], x_scale: f32, sample_offsets: &[i64], rng: &mut [u64; 2], prob: f32,
                      clip_base: usize) -> Result<(Vec<f32>, Vec<ReverbPlanRow>), Error> {
        reverb_tables_ok(sample_offsets, None, "reverb_packed_i16")?;
        let mut out: Vec<f32> = x.iter().map(|&v| v as f32 * x_scale).collect();
        let mut plan = vec![ReverbPlanRow::default(); sample_offsets.len() - 1];
        if !x.is_empty() {
            check(unsafe {
                ss_reverb_packed_i16(x.as_ptr(), x_scale, plan.len(), sample_offsets.as_ptr(), x.len(), self.raw, rng.as_mut_ptr(), clip_base, prob,
                                     out.as_mut_ptr(), plan.as_mut_ptr())
            })?;
        }
        Ok((out, plan))
    }

    /// The plan rows on the device (include/speechsauce_amd.h has the contract); the epoch is not touched.
    ///
    /// # Safety
    /// Every pointer is a device pointer to a block of the size the header states; `d_rng` is the 16-byte device block `{seed, epoch}`.
    pub unsafe fn plan_packed_device(&self, n_clips: usize, d_sample_offsets: *const i64, total_samples: usize, d_rng: *const u64, clip_base: usize,
                                     prob: f32, d_plan: *mut ReverbPlanRow, stream: *mut c_void) -> Result<(), Error> {
        check(ss_reverb_plan_packed_device(n_clips, d_sample_offsets, total_samples, self.raw, d_rng, clip_base, prob, d_plan, stream))
    }

    /// The convolution alone, on any plan table; `d_out` does not overlap `d_x`.
    ///
    /// # Safety
    /// As `plan_packed_device`; `d_out` holds `total_samples` floats.
    pub unsafe fn apply_packed_device(&self, d_x: *const f32, n_clips: usize, d_sample_offsets: *const i64, total_samples: usize,
                                      d_plan: *const ReverbPlanRow, d_out: *mut f32, stream: *mut c_void) -> Result<(), Error> {
        check(ss_reverb_apply_packed_device(d_x, n_clips, d_sample_offsets, total_samples, self.raw, d_plan, d_out, stream))
    }

    /// As `apply_packed_device` on 16-bit PCM.
    ///
    /// # Safety
    /// As `apply_packed_device`.
    pub unsafe fn apply_packed_i16_device(&self, d_x: *const i16, x_scale: f32, n_clips: usize, d_sample_offsets: *const i64, total_samples: usize,
                                          d_plan: *const ReverbPlanRow, d_out: *mut f32, stream: *mut c_void) -> Result<(), Error> {
        check(ss_reverb_apply_packed_i16_device(d_x, x_scale, n_clips, d_sample_offsets, total_samples, self.raw, d_plan, d_out, stream))
    }

    /// Plan, apply and the epoch bump: two asynchronous launches on `stream`, nothing read back; replays of a captured graph draw afresh.
    ///
    /// # Safety
    /// As `apply_packed_device` and `plan_packed_device`; one `d_rng` block serves one stream of calls.
    pub unsafe fn packed_device(&self, d_x: *const f32, n_clips: usize, d_sample_offsets: *const i64, total_samples: usize, d_rng: *mut u64,
                                clip_base: usize, prob: f32, d_out: *mut f32, d_plan: *mut ReverbPlanRow, stream: *mut c_void) -> Result<(), Error> {
        check(ss_reverb_packed_device(d_x, n_clips, d_sample_offsets, total_samples, self.raw, d_rng, clip_base, prob, d_out, d_plan, stream))
    }

    /// As `packed_device` on 16-bit PCM.
    ///
    /// # Safety
    /// As `packed_device`.
    pub unsafe fn packed_i16_device(&self, d_x: *const i16, x_scale: f32, n_clips: usize, d_sample_offsets: *const i64, total_samples: usize,
                                    d_rng: *mut u64, clip_base: usize, prob: f32, d_out: *mut f32, d_plan: *mut ReverbPlanRow,
                                    stream: *mut c_void) -> Result<(), Error> {
        check(ss_reverb_packed_i16_device(d_x, x_scale, n_clips, d_sample_offsets, total_samples, self.raw, d_rng, clip_base, prob, d_out, d_plan, stream))
    }
}

/// Polyphase windowed-sinc resampler for one pair of rates: torchaudio's default `sinc_interp_hann` filter (`lowpass_filter_width = 6`,
/// `rolloff = 0.99`).  Not in the reference crate.  Owns an `ss_resampler`; the table is uploaded by the first call that runs.
pub struct Resampler {
    raw: *mut c_void,
    orig_rate: u32,
    new_rate: u32,
    info: ResampleInfo,
}

unsafe impl Send for Resampler {}
unsafe impl Sync for Resampler {}

impl Drop for Resampler {
    fn drop(&mut self) {
        unsafe { ss_resampler_destroy(self.raw) }
    }
}

impl Resampler {
    pub fn new(orig_rate: u32, new_rate: u32, lowpass_filter_width: u32, rolloff: f32) -> Result<Resampler, Error> {
        let mut raw: *mut c_void = std::ptr::null_mut();
        check(unsafe { ss_resampler_create(orig_rate, new_rate, lowpass_filter_width, rolloff, &mut raw) })?;
        let mut rs = Resampler { raw, orig_rate, new_rate, info: ResampleInfo::default() };
        check(unsafe { ss_resampler_info(rs.raw, &mut rs.info) })?;
        Ok(rs)
    }

    pub fn info(&self) -> ResampleInfo {
        self.info
    }

    /// `ceil(n * n_samples / o)`
    pub fn out_len(&self, n_samples: usize) -> usize {
        (n_samples * self.info.n as usize + self.info.o as usize - 1) / self.info.o as usize
    }

    /// One clip -> its `out_len` resampled samples.
    pub fn resample(&self, x: &[f32]) -> Result<Vec<f32>, Error> {
        let mut out = vec![0f32; self.out_len(x.len())];
        check(unsafe { ss_resample(self.raw, x.as_ptr(), 1, x.len(), x.len(), out.as_mut_ptr(), out.len()) })?;
        Ok(out)
    }

    /// Out offsets of packed clips: also the sample offsets of the packed feature calls on the resampled block.
    pub fn packed_offsets(&self, sample_offsets: &[i64]) -> Result<Vec<i64>, Error> {
        if sample_offsets.is_empty() {
            return Err(Error { status: SS_ERR_ARG, detail: "sample_offsets must not be empty".to_string() });
        }
        let mut oo = vec![0i64; sample_offsets.len()];
        check(unsafe { ss_resample_packed_offsets(self.orig_rate, self.new_rate, sample_offsets.len() - 1, sample_offsets.as_ptr(), oo.as_mut_ptr()) })?;
        Ok(oo)
    }

    /// Clips packed end to end (clip b = `x[sample_offsets[b] .. sample_offsets[b + 1]]`) -> (the resampled block, its offsets); every
    /// clip is resampled on its own samples, one launch for all.
    pub fn resample_packed(&self, x: &[f32], sample_offsets: &[i64]) -> Result<(Vec<f32>, Vec<i64>), Error> {
        let oo = self.packed_offsets(sample_offsets)?;
        if sample_offsets[sample_offsets.len() - 1] as usize > x.len() {
            return Err(Error { status: SS_ERR_ARG, detail: "sample_offsets ends past the block".to_string() });
        }
        let mut out = vec![0f32; oo[oo.len() - 1] as usize];
        check(unsafe { ss_resample_packed(self.raw, x.as_ptr(), oo.len() - 1, sample_offsets.as_ptr(), oo.as_ptr(), out.as_mut_ptr()) })?;
        Ok((out, oo))
    }

    /// The same from 16-bit PCM: sample = `pcm * scale`, `scale` a power of two (`2^-15` for normalised audio).
    pub fn resample_packed_i16(&self, x: &[i16], sample_offsets: &[i64], scale: f32) -> Result<(Vec<f32>, Vec<i64>), Error> {
        let oo = self.packed_offsets(sample_offsets)?;
        if sample_offsets[sample_offsets.len() - 1] as usize > x.len() {
            return Err(Error { status: SS_ERR_ARG, detail: "sample_offsets ends past the block".to_string() });
        }
        let mut out = vec![0f32; oo[oo.len() - 1] as usize];
        check(unsafe { ss_resample_packed_i16(self.raw, x.as_ptr(), oo.len() - 1, sample_offsets.as_ptr(), scale, oo.as_ptr(), out.as_mut_ptr()) })?;
        Ok((out, oo))
    }

    /// Floats per stream of the pool `stream_packed` carries: `latency_periods * o + lookback + 1`.
    pub fn stream_state_len(&self) -> Result<usize, Error> {
        let mut len = 0usize;
        check(unsafe { ss_resample_stream_state_len(self.raw, &mut len) })?;
        Ok(len)
    }

    /// Live streams fed whole periods of `o` samples: entry i owns `x[sample_offsets[i] .. sample_offsets[i + 1]]`, row `slots[i]` of
    /// `pool` (`[pool_streams, stream_state_len]`, all zeros: fresh streams) and `n` outputs per period, `latency_periods * n` outputs
    /// late (zeros while the stream's output time is negative).
    pub fn stream_packed(&self, x: &[f32], sample_offsets: &[i64], slots: &[i32], pool: &mut Array2<f32>) -> Result<Vec<f32>, Error> {
        let len = self.stream_state_len()?;
        if sample_offsets.len() != slots.len() + 1 {
            return Err(Error { status: SS_ERR_ARG, detail: "sample_offsets must have one entry more than slots".to_string() });
        }
        if pool.ncols() != len || !pool.is_standard_layout() {
            return Err(Error { status: SS_ERR_ARG, detail: "pool must be a standard-layout [pool_streams, state_len] block".to_string() });
        }
        let total = sample_offsets[slots.len()];
        if total < 0 || total as usize > x.len() {
            return Err(Error { status: SS_ERR_ARG, detail: "sample_offsets ends past the block".to_string() });
        }
        let mut out = vec![0f32; total as usize / self.info.o as usize * self.info.n as usize];
        check(unsafe {
            ss_resample_stream_packed(self.raw, x.as_ptr(), slots.len(), sample_offsets.as_ptr(), slots.as_ptr(), pool.nrows(), pool.as_mut_ptr(),
                                      out.as_mut_ptr())
        })?;
        Ok(out)
    }

    /// The last `latency_periods * n` outputs of the streams in `slots` (entry i: that many outputs from `i * latency_periods * n` on);
    /// afterwards their pool rows are zero (fresh streams).
    pub fn stream_flush(&self, slots: &[i32], pool: &mut Array2<f32>) -> Result<Vec<f32>, Error> {
        let len = self.stream_state_len()?;
        if pool.ncols() != len || !pool.is_standard_layout() {
            return Err(Error { status: SS_ERR_ARG, detail: "pool must be a standard-layout [pool_streams, state_len] block".to_string() });
        }
        let mut out = vec![0f32; slots.len() * self.info.latency_periods as usize * self.info.n as usize];
        check(unsafe { ss_resample_stream_flush(self.raw, slots.len(), slots.as_ptr(), pool.nrows(), pool.as_mut_ptr(), out.as_mut_ptr()) })?;
        Ok(out)
    }
}

/// speechsauce::config (config.rs)
/// `ss_whisper_params`: the Whisper log-mel front end's parameters (field order is ABI; see `ss_whisper_*` in the C header).
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct SsWhisperParams {
    pub struct_size: u32,
    pub sample_rate: u32,
    pub n_fft: u32,
    pub hop_length: u32,
    pub n_mels: u32,
}

impl SsWhisperParams {
    /// 16000 / 400 / 160 with `n_mels` mels (80, or 128 for large-v3).
    pub fn new(n_mels: u32) -> SsWhisperParams {
        let mut p: SsWhisperParams = unsafe { std::mem::zeroed() };
        unsafe { ss_whisper_params_default(&mut p, n_mels) };
        p
    }
}

/// Element type of the output block (`SS_PAD_F32` / `SS_PAD_F16` / `SS_PAD_BF16`).
pub const SS_PAD_F32: c_int = 0;
pub const SS_PAD_F16: c_int = 1;
pub const SS_PAD_BF16: c_int = 2;

/// The Whisper log-mel block (`whisper.audio.log_mel_spectrogram`): `[n_mels x n_frames]` per clip, every clip padded or trimmed to
/// `n_frames * 160` samples.  Not in the reference crate.  Owns an `ss_whisper_config`; calls on one front end must be ordered on one
/// stream.
pub struct WhisperFrontEnd {
    raw: *mut c_void,
    params: SsWhisperParams,
}

unsafe impl Send for WhisperFrontEnd {}

impl Drop for WhisperFrontEnd {
    fn drop(&mut self) {
        unsafe { ss_whisper_config_destroy(self.raw) }
    }
}

impl WhisperFrontEnd {
    pub fn new(n_mels: u32) -> Result<WhisperFrontEnd, Error> {
        let params = SsWhisperParams::new(n_mels);
        let mut raw: *mut c_void = std::ptr::null_mut();
        check(unsafe { ss_whisper_config_create(&params, &mut raw) })?;
        Ok(WhisperFrontEnd { raw, params })
    }

    pub fn n_mels(&self) -> usize {
        self.params.n_mels as usize
    }

    /// `n_samples / 160`: the frames Whisper keeps of a clip.
    pub fn num_frames(n_samples: usize) -> Result<usize, Error> {
        let mut t = 0usize;
        check(unsafe { ss_whisper_num_frames(n_samples, &mut t) })?;
        Ok(t)
    }

    /// Bytes of f32 scratch the device calls take for a 16-bit `dtype` (0 for `SS_PAD_F32`).
    pub fn work_bytes(&self, batch: usize, n_frames: usize, dtype: c_int) -> Result<usize, Error> {
        let mut n = 0usize;
        check(unsafe { ss_whisper_work_bytes(&self.params, batch, n_frames, dtype, &mut n) })?;
        Ok(n)
    }

    /// `SS_ERR_DEVICE` once if a packed launch has met a bad table entry since the last look.
    pub fn device_status(&self) -> Result<(), Error> {
        check(unsafe { ss_whisper_config_device_status(self.raw) })
    }

    /// One clip -> `[n_mels x n_frames]`, f32.
    pub fn log_mel(&self, x: &[f32], n_frames: usize) -> Result<Array2<f32>, Error> {
        let mut out = Array2::<f32>::zeros((self.n_mels(), n_frames));
        let keep = [0f32; 4]; // an empty clip reads nothing: any address will do
        let ptr = if x.is_empty() { keep.as_ptr() } else { x.as_ptr() };
        check(unsafe { ss_whisper_log_mel(self.raw, ptr, 1, x.len(), x.len(), n_frames, SS_PAD_F32, out.as_mut_ptr() as *mut c_void) })?;
        Ok(out)
    }

    /// Clips packed end to end -> (`[n_clips * n_mels x n_frames]`, block b = rows `b * n_mels ..`; the `[n_clips]` lengths
    /// `min(len / 160, n_frames)`).
    pub fn log_mel_packed(&self, x: &[f32], sample_offsets: &[i64], n_frames: usize) -> Result<(Array2<f32>, Vec<i32>), Error> {
        if sample_offsets.is_empty() || sample_offsets[sample_offsets.len() - 1] as usize > x.len() {
            return Err(Error { status: SS_ERR_ARG, detail: "sample_offsets is empty or ends past the block".to_string() });
        }
        let n = sample_offsets.len() - 1;
        let mut out = Array2::<f32>::zeros((n * self.n_mels(), n_frames));
        let mut lens = vec![0i32; n];
        let keep = [0f32; 4];
        let ptr = if x.is_empty() { keep.as_ptr() } else { x.as_ptr() };
        check(unsafe {
            ss_whisper_log_mel_packed(self.raw, ptr, n, sample_offsets.as_ptr(), n_frames, SS_PAD_F32, out.as_mut_ptr() as *mut c_void, lens.as_mut_ptr())
        })?;
        Ok((out, lens))
    }

    /// The dense device call on `stream`: device pointers, nothing is copied or allocated (`ss_whisper_log_mel_device`).
    pub unsafe fn log_mel_device(&self, d_x: *const f32, batch: usize, n_samples: usize, ld: usize, n_frames: usize, dtype: c_int, d_work: *mut c_void,
                                 d_out: *mut c_void, stream: *mut c_void) -> Result<(), Error> {
        check(ss_whisper_log_mel_device(self.raw, d_x, batch, n_samples, ld, n_frames, dtype, d_work, d_out, stream))
    }

    /// The packed device call on `stream` (`ss_whisper_log_mel_packed_device`): replays as a captured graph over changed tables.
    pub unsafe fn log_mel_packed_device(&self, d_x: *const f32, n_clips: usize, d_sample_offsets: *const i64, n_frames: usize, dtype: c_int,
                                        d_work: *mut c_void, d_out: *mut c_void, d_lengths: *mut i32, stream: *mut c_void) -> Result<(), Error> {
        check(ss_whisper_log_mel_packed_device(self.raw, d_x, n_clips, d_sample_offsets, n_frames, dtype, d_work, d_out, d_lengths, stream))
    }
}

/// `ss_nemo_params`: the NeMo / Parakeet log-mel front end's parameters (field order is ABI; see `ss_nemo_*` in the C header).
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct SsNemoParams {
    pub struct_size: u32,
    pub sample_rate: u32,
    pub n_fft: u32,
    pub win_length: u32,
    pub hop_length: u32,
    pub n_mels: u32,
    pub normalize: i32,
    pub preemph: f32,
    pub log_guard: f32,
    pub norm_eps: f32,
}

pub const SS_NEMO_NORM_NONE: i32 = 0;
pub const SS_NEMO_NORM_PER_FEATURE: i32 = 1;

impl SsNemoParams {
    /// 16000 / 512 / 400 / 160 with `n_mels` mels (80 or 128), pre-emphasis 0.97, per-feature normalisation.
    pub fn new(n_mels: u32) -> SsNemoParams {
        let mut p: SsNemoParams = unsafe { std::mem::zeroed() };
        unsafe { ss_nemo_params_default(&mut p, n_mels) };
        p
    }
}

/// The NeMo / Parakeet log-mel rows (`[len / 160 x n_mels]` per clip; NeMo's `AudioToMelSpectrogramPreprocessor`).  Not in the
/// reference crate.  Owns an `ss_nemo_config`.
pub struct NemoFrontEnd {
    raw: *mut c_void,
    params: SsNemoParams,
}

unsafe impl Send for NemoFrontEnd {}

impl Drop for NemoFrontEnd {
    fn drop(&mut self) {
        unsafe { ss_nemo_config_destroy(self.raw) }
    }
}

impl NemoFrontEnd {
    pub fn new(params: SsNemoParams) -> Result<NemoFrontEnd, Error> {
        let mut raw: *mut c_void = std::ptr::null_mut();
        check(unsafe { ss_nemo_config_create(&params, &mut raw) })?;
        Ok(NemoFrontEnd { raw, params })
    }

    pub fn n_mels(&self) -> usize {
        self.params.n_mels as usize
    }

    /// `n_samples / 160`: the rows kept of a clip (0 for a clip shorter than one hop).
    pub fn num_frames(&self, n_samples: usize) -> Result<usize, Error> {
        let mut t = 0usize;
        check(unsafe { ss_nemo_num_frames(&self.params, n_samples, &mut t) })?;
        Ok(t)
    }

    /// `SS_ERR_DEVICE` once if a packed launch has skipped an inconsistent clip since the last look.
    pub fn device_status(&self) -> Result<(), Error> {
        check(unsafe { ss_nemo_config_device_status(self.raw) })
    }

    /// One clip -> `[len / 160 x n_mels]`.
    pub fn log_mel(&self, x: &[f32]) -> Result<Array2<f32>, Error> {
        let mut out = Array2::<f32>::zeros((self.num_frames(x.len())?, self.n_mels()));
        if !out.is_empty() {
            check(unsafe { ss_nemo_log_mel(self.raw, x.as_ptr(), 1, x.len(), x.len(), out.as_mut_ptr()) })?;
        }
        Ok(out)
    }

    /// Clips packed end to end -> (the rows `[sum T_b x n_mels]`, the `[n_clips + 1]` frame offsets).
    pub fn log_mel_packed(&self, x: &[f32], sample_offsets: &[i64]) -> Result<(Array2<f32>, Vec<i64>), Error> {
        if sample_offsets.is_empty() || sample_offsets[sample_offsets.len() - 1] as usize > x.len() {
            return Err(Error { status: SS_ERR_ARG, detail: "sample_offsets is empty or ends past the block".to_string() });
        }
        let n = sample_offsets.len() - 1;
        let mut fo = vec![0i64; n + 1];
        check(unsafe { ss_nemo_packed_frame_offsets(&self.params, n, sample_offsets.as_ptr(), fo.as_mut_ptr()) })?;
        let mut out = Array2::<f32>::zeros((fo[n] as usize, self.n_mels()));
        if !out.is_empty() {
            check(unsafe { ss_nemo_log_mel_packed(self.raw, x.as_ptr(), n, sample_offsets.as_ptr(), out.as_mut_ptr()) })?;
        }
        Ok((out, fo))
    }

    /// The dense device call on `stream`: device pointers, nothing is copied or allocated (`ss_nemo_log_mel_device`).
    pub unsafe fn log_mel_device(&self, d_x: *const f32, batch: usize, n_samples: usize, ld: usize, d_out: *mut f32,
                                 stream: *mut c_void) -> Result<(), Error> {
        check(ss_nemo_log_mel_device(self.raw, d_x, batch, n_samples, ld, d_out, stream))
    }

    /// The packed device call on `stream` (`ss_nemo_log_mel_packed_device`): replays as a captured graph over changed tables.
    pub unsafe fn log_mel_packed_device(&self, d_x: *const f32, n_clips: usize, d_sample_offsets: *const i64, d_frame_offsets: *const i64,
                                        total_frames: usize, d_out: *mut f32, stream: *mut c_void) -> Result<(), Error> {
        check(ss_nemo_log_mel_packed_device(self.raw, d_x, n_clips, d_sample_offsets, d_frame_offsets, total_frames, d_out, stream))
    }

    /// The stream pool's sizes (`ss_nstream_state_len`): (S, the carried samples per stream = the floats of a pool row; L, the
    /// warm-up rows after a reset and the rows a flush returns per stream).
    pub fn stream_state_len(&self) -> Result<(usize, usize), Error> {
        let (mut s, mut l) = (0usize, 0usize);
        check(unsafe { ss_nstream_state_len(&self.params, &mut s, &mut l) })?;
        Ok((s, l))
    }

    /// Row offsets of the entries of a pool call (`ss_nstream_row_offsets`): every chunk is whole 160-sample hops.
    pub fn stream_row_offsets(&self, sample_offsets: &[i64]) -> Result<Vec<i64>, Error> {
        if sample_offsets.is_empty() {
            return Err(Error { status: SS_ERR_ARG, detail: "sample_offsets must not be empty".to_string() });
        }
        let mut ro = vec![0i64; sample_offsets.len()];
        check(unsafe { ss_nstream_row_offsets(&self.params, sample_offsets.len() - 1, sample_offsets.as_ptr(), ro.as_mut_ptr()) })?;
        Ok(ro)
    }

    // the checks the pool wrappers share: the tables against the block and the pool -> (row offsets, pool rows)
    fn stream_shape<T>(&self, x: &[T], sample_offsets: &[i64], slots: &[i32], pool: &[f32]) -> Result<(Vec<i64>, usize), Error> {
        let ro = self.stream_row_offsets(sample_offsets)?;
        let (s, _) = self.stream_state_len()?;
        if slots.len() != sample_offsets.len() - 1 || sample_offsets[sample_offsets.len() - 1] as usize > x.len() {
            return Err(Error { status: SS_ERR_ARG, detail: "pool call: shape mismatch".to_string() });
        }
        if pool.is_empty() || pool.len() % s != 0 {
            return Err(Error { status: SS_ERR_ARG, detail: "pool call: the pool is not a whole number of rows".to_string() });
        }
        Ok((ro, pool.len() / s))
    }

    /// Ragged streaming log-mel over a pool of stream states (`ss_nstream_log_mel_packed`; a handle with `normalize` none): entry i
    /// is the chunk `x[sample_offsets[i] .. sample_offsets[i+1])` (whole hops) of the stream whose state is pool row `slots[i]`;
    /// `pool` is `[pool_streams x S]`, all-zero rows are fresh streams.  -> (rows, row offsets); the first L rows of a fresh stream
    /// are warm-up rows.
    pub fn log_mel_stream_packed(&self, x: &[f32], sample_offsets: &[i64], slots: &[i32], pool: &mut [f32]) -> Result<(Array2<f32>, Vec<i64>), Error> {
        let (ro, pool_streams) = self.stream_shape(x, sample_offsets, slots, pool)?;
        let mut out = Array2::<f32>::zeros((ro[ro.len() - 1] as usize, self.n_mels()));
        check(unsafe {
            ss_nstream_log_mel_packed(self.raw, x.as_ptr(), slots.len(), sample_offsets.as_ptr(), slots.as_ptr(), pool_streams, pool.as_mut_ptr(),
                                      out.as_mut_ptr())
        })?;
        Ok((out, ro))
    }

    /// `log_mel_stream_packed` fed signed 16-bit PCM: sample = `pcm as f32 * scale`, `scale` a power of two (`ss_nstream_log_mel_packed_i16`).
    pub fn log_mel_stream_packed_i16(&self, x: &[i16], sample_offsets: &[i64], slots: &[i32], scale: f32, pool: &mut [f32])
                                     -> Result<(Array2<f32>, Vec<i64>), Error> {
        let (ro, pool_streams) = self.stream_shape(x, sample_offsets, slots, pool)?;
        let mut out = Array2::<f32>::zeros((ro[ro.len() - 1] as usize, self.n_mels()));
        check(unsafe {
            ss_nstream_log_mel_packed_i16(self.raw, x.as_ptr(), slots.len(), sample_offsets.as_ptr(), slots.as_ptr(), pool_streams, scale,
                                          pool.as_mut_ptr(), out.as_mut_ptr())
        })?;
        Ok((out, ro))
    }

    /// The end of the named streams (`ss_nstream_flush`): `[slots.len() * L x n_mels]`, stream i's last L rows at rows `i * L ..`;
    /// the named pool rows are zero (fresh streams) afterwards.
    pub fn stream_flush(&self, slots: &[i32], pool: &mut [f32]) -> Result<Array2<f32>, Error> {
        let (s, l) = self.stream_state_len()?;
        if pool.is_empty() || pool.len() % s != 0 {
            return Err(Error { status: SS_ERR_ARG, detail: "flush: the pool is not a whole number of rows".to_string() });
        }
        let mut out = Array2::<f32>::zeros((slots.len() * l, self.n_mels()));
        check(unsafe { ss_nstream_flush(self.raw, slots.len(), slots.as_ptr(), pool.len() / s, pool.as_mut_ptr(), out.as_mut_ptr()) })?;
        Ok(out)
    }
}

pub mod config {
    pub use super::{SpeechConfig, SpeechConfigBuilder};
}
/// speechsauce::feature (feature.rs): mfcc, mfe, mel_spectrogram1 / 2 (+ the private lmfe / extract_derivative_feature, public here)
pub mod feature {
    pub use super::{extract_derivative_feature, lmfe, mel_spectrogram1, mel_spectrogram2, mfcc, mfe};
    pub use super::{mfcc_batch_device, mfcc_batches_device, try_lmfe, try_mel_spectrogram2, try_mfcc, try_mfcc_batch, try_mfe};
}
/// speechsauce::processing (processing.rs)
pub mod processing {
    pub use super::{cmvn, cmvnw, derivative_extraction, power_spectrum, preemphasis, stack_frames};
    pub use super::{power_spectrum_with, stack_frames_with, try_power_spectrum, try_power_spectrum_of_signal, try_power_spectrum_with,
                    try_stack_frames, try_stack_frames_with};
}
/// speechsauce::functions (functions.rs)
pub mod functions {
    pub use super::{frequency_arr_to_mel, frequency_to_mel, mel_arr_to_frequency, mel_to_frequency, stft1, stft2, triangle, try_stft2,
                    zero_handling};
}
/// speechsauce::util: the `ArrayLog` trait of the hot path (util.rs:372-381).  The pad helpers of util.rs are not part of the path
///  and are not provided.
pub mod util {
    pub use super::ArrayLog;
}
/// Not in the reference: the clip-sharding helpers and the RCCL gather of the final blocks.
pub mod distributed {
    pub use super::{all_gather_features, gather_features, shard_bounds};
}
