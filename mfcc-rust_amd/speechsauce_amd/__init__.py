"""speechsauce_amd -- Python front of the MI355X-native MFCC / mel-spectrogram hot path.

Drop-in for the hot-path functions of the reference's ``speechsauce`` package
(py-speechsauce/speechsauce/__init__.py:37-132): the same names, keyword arguments, defaults,
dtype rule (float32 only) and output shapes, served by hand-written HIP kernels through the C ABI
in ``include/speechsauce_amd.h``.  ``import speechsauce_amd as speechsauce`` is the intended use.

Inputs may be numpy arrays (host path: H2D, kernels, D2H inside the library) or torch tensors on
a ROCm device (zero-copy device path on torch's current stream; the result is a torch tensor).
There is no CPU compute path: without the built library and a HIP device these functions raise.
"""
from __future__ import annotations

import ctypes as C
from functools import lru_cache
from typing import Optional

import numpy as np

from . import _lib
from ._lib import SpeechSauceError, SsKaldiParams, SsNemoParams, SsParams, SsResampleInfo, SsWhisperParams, make_params  # noqa: F401

__all__ = ["mfcc", "mel_spectrogram", "preemphasis", "cmvn", "cmvnw", "derivative_extraction", "extract_derivative_feature",
           "mfe", "mfcc_batch", "mfe_batch", "lmfe", "lmfe_batch", "power_to_db", "stft", "stack_frames", "power_spectrum",
           "power_spectrum_of_signal", "mfcc_packed", "mfe_packed", "mfcc_list", "mel_spectrogram_packed",
           "mel_spectrogram_list", "log_mel_spectrogram", "log_mel_spectrogram_packed", "log_mel_spectrogram_list", "stft_packed", "cmvn_packed", "cmvnw_packed", "cmvn_stats_packed", "cmvn_apply_packed", "cmvn_grouped_packed",
           "cmvn_stats_to_kaldi", "cmvn_stats_from_kaldi", "power_to_db_packed", "lmfe_packed",
           "MelSpectrogramStream", "StftStream",
           "MfccStream", "MfeStream", "MfccStreamPool", "MfeStreamPool", "MelSpectrogramStreamPool", "StftStreamPool", "CmvnStreamPool",
           "add_deltas", "add_deltas_packed", "AddDeltasStreamPool",
           "splice", "splice_packed", "lfr", "lfr_packed", "SpliceStreamPool",
           "Affine", "splice_affine", "splice_affine_packed", "transform_feats_packed",
           "vad_energy", "vad_energy_packed", "select_rows", "select_rows_packed", "VadEnergyStreamPool",
           "pad", "pad_packed",
           "spec_augment_spans", "mask_spans_packed", "spec_augment_packed", "SpecAugment",
           "NOISE_PLAN_DTYPE", "noise_plan_rows", "noise_draws", "noise_plan_packed", "noise_apply_packed", "noise_mix_packed", "NoiseMix",
           "REVERB_PLAN_DTYPE", "reverb_plan_rows", "reverb_draws", "reverb_plan_packed", "reverb_apply_packed", "reverb_packed", "ReverbBank", "Reverb",
           "resample", "resample_packed", "resample_list", "ResampleStreamPool", "Resampler",
           "kaldi_fbank", "kaldi_mfcc", "kaldi_fbank_packed", "kaldi_mfcc_packed", "kaldi_fbank_list", "kaldi_mfcc_list", "KaldiConfig",
           "KaldiFbankStreamPool", "KaldiMfccStreamPool",
           "whisper_log_mel", "whisper_log_mel_packed", "whisper_log_mel_list", "whisper_num_frames", "WhisperConfig",
           "nemo_log_mel", "nemo_log_mel_packed", "nemo_log_mel_list", "nemo_num_frames", "NemoConfig", "NemoLogMelStreamPool",
           "SpeechConfig", "SpeechSauceError"]


def _is_torch(x) -> bool:
    return type(x).__module__.split(".")[0] == "torch"


class _Handle:
    """What the owners of a handle of the C ABI share: the handle ``_h`` (null until the class's create call has filled it), the
    build ``_owner`` that creates it and therefore destroys it (tests run the front on the lab build too), and its release through
    the entry point ``_destroy`` names."""

    _destroy = ""

    def __init__(self):
        self._h = C.c_void_p()
        self._owner = _lib.lib()

    def __del__(self):  # (a half-built object has no handle, or a null one; a failing destroy must not raise from here)
        h, self._h = getattr(self, "_h", None), None
        if h:
            try:
                getattr(self._owner, self._destroy)(h)
            except Exception:
                pass

    @property
    def handle(self) -> C.c_void_p:
        return self._h


class SpeechConfig(_Handle):
    """Owns an ``ss_config`` handle: the counterpart of ``PySpeechSauce(SpeechConfig)``
    (py-speechsauce/src/lib.rs:7-10; speechsauce/src/config.rs:99-185)."""

    _destroy = "ss_config_destroy"

    def __init__(self, params: SsParams):
        super().__init__()
        self.params = params
        _lib.check(self._owner.ss_config_create(C.byref(params), C.byref(self._h)))

    # ---- derived sizes -------------------------------------------------------------------
    def num_frames(self, n_samples: int) -> int:
        t = C.c_size_t()
        _lib.check(_lib.lib().ss_num_frames(C.byref(self.params), n_samples, C.byref(t)))
        return t.value

    def stft_rows(self, n_samples: int) -> tuple[int, int]:
        r, rr = C.c_size_t(), C.c_size_t()
        _lib.check(_lib.lib().ss_stft_rows(C.byref(self.params), n_samples, C.byref(r), C.byref(rr)))
        return r.value, rr.value

    def device_status(self) -> None:
        """Raises SpeechSauceError (SS_ERR_DEVICE) if a kernel of an asynchronous launch on this config has reported a
        device-side protocol error since the last call.  Meaningful after the stream has been synchronised; the numpy
        (host-pointer) calls check it themselves."""
        _lib.check(_lib.lib().ss_config_device_status(self._h))


def _speech_config(sampling_frequency, frame_length, frame_stride, num_cepstral, num_filters, fft_length,
                   low_frequency, dc_elimination, high_frequency=None, **switches) -> SpeechConfig:
    """Same positional order as ``_internal._speech_config`` (py-speechsauce/src/lib.rs:226-254)."""
    return SpeechConfig(make_params(
        sample_rate=sampling_frequency, fft_points=fft_length, frame_length=frame_length,
        frame_stride=frame_stride, num_cepstral=num_cepstral, num_filters=num_filters,
        low_frequency=low_frequency, high_frequency=high_frequency, dc_elimination=dc_elimination, **switches))


@lru_cache(maxsize=32)
def _get_speech_config(sampling_frequency, frame_length=0.020, frame_stride=0.01, num_cepstral=13, num_filters=40,
                       fft_length=512, low_frequency=0, high_frequency: Optional[float] = None,
                       dc_elimination=True, switches: tuple = (), device: int = -1) -> SpeechConfig:
    """Memoised config factory (py-speechsauce/speechsauce/__init__.py:8-34).

    ``device`` is part of the key: a config owns tables in the memory of the HIP device that was current when it was
    created, so each device gets its own (-1 = whichever device is current, the host-array path)."""
    if device >= 0:
        import torch

        with torch.cuda.device(device):
            return _speech_config(sampling_frequency, frame_length, frame_stride, num_cepstral, num_filters, fft_length,
                                  low_frequency, dc_elimination, high_frequency, **dict(switches))
    return _speech_config(sampling_frequency, frame_length, frame_stride, num_cepstral, num_filters, fft_length,
                          low_frequency, dc_elimination, high_frequency, **dict(switches))


_lib._on_switch.append(_get_speech_config.cache_clear)  # a config belongs to the library that created it


def _device_key(signal) -> int:
    """Index of the ROCm device a tensor lives on; -1 for host arrays (the library's current device)."""
    if _is_torch(signal) and signal.is_cuda:
        return signal.device.index if signal.device.index is not None else -1
    if not _is_torch(signal):
        try:  # host arrays run on the current device: key the config by it, so that a later ss_set_device gets its own
            import torch

            if torch.cuda.is_initialized():
                return torch.cuda.current_device()
        except Exception:
            pass
    return -1


def _require_f32(signal, ndims: tuple[int, ...], what: str):
    """The binding takes PyReadonlyArray<f32> only (py-speechsauce/src/lib.rs:170,182): no silent casts."""
    if _is_torch(signal):
        import torch

        if signal.dtype != torch.float32:
            raise TypeError(f"{what}: signal must be float32, got {signal.dtype}")
        if signal.dim() not in ndims:
            raise ValueError(f"{what}: Input signal must be {' or '.join(str(d) + 'd' for d in ndims)}")
        if not signal.is_cuda:
            signal = signal.detach().numpy()
        return signal
    arr = np.asarray(signal)
    if arr.dtype != np.float32:
        raise TypeError(f"{what}: signal must be float32, got {arr.dtype}")
    if arr.ndim not in ndims:
        raise ValueError(f"{what}: Input signal must be {' or '.join(str(d) + 'd' for d in ndims)}")
    return arr


def _require_i16(signal, what: str, ndims: tuple[int, ...] = (1,)):
    """The PCM forms (``pcm_scale=``) take int16 only, of the dimensions the call takes: no silent casts."""
    if _is_torch(signal):
        import torch

        if signal.dtype != torch.int16:
            raise TypeError(f"{what}: with pcm_scale the signal must be int16, got {signal.dtype}")
        if signal.dim() not in ndims:
            raise ValueError(f"{what}: Input signal must be {' or '.join(str(d) + 'd' for d in ndims)}")
        if not signal.is_cuda:
            signal = signal.detach().numpy()
        return signal
    arr = np.asarray(signal)
    if arr.dtype != np.int16:
        raise TypeError(f"{what}: with pcm_scale the signal must be int16, got {arr.dtype}")
    if arr.ndim not in ndims:
        raise ValueError(f"{what}: Input signal must be {' or '.join(str(d) + 'd' for d in ndims)}")
    return arr


def _check_pcm_scale(pcm_scale, what: str) -> float:
    """``pcm_scale`` of the PCM forms: a power of two in [2**-64, 2**64] (the product with an int16 is then exact)."""
    import math

    v = float(pcm_scale)
    if not (math.isfinite(v) and v > 0.0 and math.frexp(v)[0] == 0.5 and -64 <= math.frexp(v)[1] - 1 <= 64):
        raise ValueError(f"{what}: pcm_scale must be a power of two in [2**-64, 2**64], got {pcm_scale!r}")
    return v


def _require_signal(signal, ndims: tuple[int, ...], what: str, pcm_scale):
    """The signal of a one-shot call and its scale: float32 and None, or -- with ``pcm_scale`` -- int16 and the checked scale."""
    if pcm_scale is None:
        return _require_f32(signal, ndims, what), None
    scale = _check_pcm_scale(pcm_scale, what)
    return _require_i16(signal, what, ndims), scale


def _stream_ptr():
    import torch

    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _launch(device, fn, *args):
    """One device call that holds temporaries: ``fn(*args, stream)`` with ``device`` current, on torch's current stream there, run
    through ``_lib.check``.  A tensor among ``args`` is an input: it goes in as its address.  A numpy array is a host table: it is
    uploaded to ``device`` first.  Everything else passes through -- outputs and carried state go in as ``data_ptr()``, which also
    keeps them out of what follows.  The launch is asynchronous, so once the call went through every input and every uploaded table
    is recorded on the stream: they are often temporaries, and the allocator must keep them until the stream has passed them.
    -> the uploaded tables, in the order of ``args``."""
    import torch

    with torch.cuda.device(device):
        held, tables, call = [], [], []
        for a in args:
            if isinstance(a, np.ndarray):
                a = torch.from_numpy(a).to(device)
                tables.append(a)
            if isinstance(a, torch.Tensor):
                held.append(a)
                a = a.data_ptr()
            call.append(a)
        stream = torch.cuda.current_stream()  # (looked up once: what ``_stream_ptr()`` would hand over is what gets recorded)
        _lib.check(fn(*call, C.c_void_p(stream.cuda_stream)))
        for t in held:
            t.record_stream(stream)
    return tables


# ---- internal entry points (the `_internal` pyfns, py-speechsauce/src/lib.rs:167-204) -------------

def _internal_mfcc_batch(signal, config: SpeechConfig, scale=None):
    """signal [B, L] -> [B, T, num_cepstral]; scale: the signal is int16 PCM, sample = int16 * scale (the ``_i16`` entry points)"""
    lib = _lib.lib()
    i16, sc = ("", []) if scale is None else ("_i16", [scale])
    B, L = signal.shape
    T = config.num_frames(L)
    Cc = config.params.num_cepstral
    if _is_torch(signal):
        import torch

        x = signal if signal.stride(1) == 1 else signal.contiguous()
        out = torch.empty((B, T, Cc), dtype=torch.float32, device=x.device)
        with torch.cuda.device(x.device):
            _lib.check(getattr(lib, f"ss_mfcc_batch{i16}_device")(config.handle, x.data_ptr(), B, L, x.stride(0) if B > 1 else L, *sc,
                                                                  out.data_ptr(), _stream_ptr()))
        return out
    x = np.ascontiguousarray(signal)
    out = np.empty((B, T, Cc), dtype=np.float32)
    _lib.check(getattr(lib, f"ss_mfcc_batch{i16}")(config.handle, x.ctypes.data, B, L, L, *sc, out.ctypes.data))
    return out


def _internal_mfe_batch(signal, config: SpeechConfig, scale=None):
    lib = _lib.lib()
    i16, sc = ("", []) if scale is None else ("_i16", [scale])
    B, L = signal.shape
    T = config.num_frames(L)
    M = config.params.num_filters
    if _is_torch(signal):
        import torch

        x = signal if signal.stride(1) == 1 else signal.contiguous()
        feat = torch.empty((B, T, M), dtype=torch.float32, device=x.device)
        en = torch.empty((B, T), dtype=torch.float32, device=x.device)
        with torch.cuda.device(x.device):
            _lib.check(getattr(lib, f"ss_mfe_batch{i16}_device")(config.handle, x.data_ptr(), B, L, x.stride(0) if B > 1 else L, *sc,
                                                                 feat.data_ptr(), en.data_ptr(), _stream_ptr()))
        return feat, en
    x = np.ascontiguousarray(signal)
    feat = np.empty((B, T, M), dtype=np.float32)
    en = np.empty((B, T), dtype=np.float32)
    _lib.check(getattr(lib, f"ss_mfe_batch{i16}")(config.handle, x.ctypes.data, B, L, L, *sc, feat.ctypes.data, en.ctypes.data))
    return feat, en


def _internal_mel_spectrogram(signal, config: SpeechConfig, scale=None, db=None):
    """1-D -> [n_mels, rows]; 2-D [C, L] -> [C, n_mels, rows] (py-speechsauce/src/lib.rs:179-204); scale: the signal is int16
    PCM, sample = int16 * scale (the ``_i16`` entry points); db: [ref, amin, top_db] of the ``ss_log_mel_spectrogram*`` forms."""
    lib = _lib.lib()
    i16, sc = ("", []) if scale is None else ("_i16", [scale])
    name, dbargs = ("ss_mel_spectrogram", []) if db is None else ("ss_log_mel_spectrogram", db)
    one_d = signal.ndim == 1
    sig2 = signal[None, :] if one_d else signal
    ch, L = sig2.shape
    R, _ = config.stft_rows(L)
    M = config.params.num_filters
    if _is_torch(sig2):
        import torch

        x = sig2 if sig2.stride(1) == 1 else sig2.contiguous()
        out = torch.empty((ch, M, R), dtype=torch.float32, device=x.device)
        with torch.cuda.device(x.device):
            _lib.check(getattr(lib, f"{name}{i16}_device")(config.handle, x.data_ptr(), ch, L, x.stride(0) if ch > 1 else L, *sc, *dbargs,
                                                           out.data_ptr(), _stream_ptr()))
    else:
        x = np.ascontiguousarray(sig2)
        out = np.empty((ch, M, R), dtype=np.float32)
        _lib.check(getattr(lib, f"{name}{i16}")(config.handle, x.ctypes.data, ch, L, *sc, *dbargs, out.ctypes.data))
    return out[0] if one_d else out


def _internal_mel_spectrogram_batches(signals, config: SpeechConfig):
    """Several [C_i, L] blocks (same L) -> list of [C_i, n_mels, rows]."""
    if not all(_is_torch(x) and x.is_cuda for x in signals):
        return [_internal_mel_spectrogram(x, config) for x in signals]
    import torch

    lib = _lib.lib()
    dev = signals[0].device
    L = signals[0].shape[1]
    if any(x.device != dev or x.shape[1] != L for x in signals):
        raise ValueError("mel_spectrogram: the blocks of one call must live on one device and hold clips of one length")
    R, _ = config.stft_rows(L)
    M = config.params.num_filters
    xs = [x if (x.stride(1) == 1 and (x.shape[0] <= 1 or x.stride(0) == L)) else x.contiguous() for x in signals]
    outs = [torch.empty((x.shape[0], M, R), dtype=torch.float32, device=dev) for x in xs]
    n = len(xs)
    px = (C.c_void_p * n)(*[x.data_ptr() for x in xs])
    po = (C.c_void_p * n)(*[o.data_ptr() for o in outs])
    nb = (C.c_size_t * n)(*[x.shape[0] for x in xs])
    with torch.cuda.device(dev):
        _lib.check(lib.ss_mel_spectrogram_batches_device(config.handle, n, px, nb, L, L, po, _stream_ptr()))
    return outs


# ---- public API (py-speechsauce/speechsauce/__init__.py:37-132) ------------------------------------

def _cfg(sampling_frequency, frame_length, frame_stride, num_cepstral, num_filters, fft_length, low_frequency,
         high_frequency, dc_elimination, switches, signal=None) -> SpeechConfig:
    return _get_speech_config(sampling_frequency, frame_length, frame_stride, num_cepstral, num_filters, fft_length,
                              low_frequency, high_frequency, dc_elimination, tuple(sorted(switches.items())),
                              _device_key(signal) if signal is not None else -1)


def mfcc(signal, sampling_frequency, frame_length=0.020, frame_stride=0.01, num_cepstral=13, num_filters=40,
         fft_length=512, low_frequency=0, high_frequency=None, dc_elimination=True, pcm_scale=None, **switches):
    """MFCC features of a 1-D float32 signal -> (num_frames, num_cepstral).

    Mirrors ``speechsauce.mfcc`` (py-speechsauce/speechsauce/__init__.py:37-83 -> feature.rs:99-148).
    ``switches`` are the SURVEY section-0 options (framing, spectrum_exponent, dct_norm, dct2_gain,
    mfcc_window, preemph_coef, preemph_shift); none given == reference mode.

    ``pcm_scale``: the signal is int16 PCM, converted on load as ``int16 * pcm_scale`` (a power of two in [2**-64, 2**64]:
    2**-15 for normalised audio, 1.0 for integer-valued floats) -- bit for bit the features of that float32 signal, without the
    conversion pass and with half the bytes over the link for host arrays.  ``mfcc_batch``, ``mfe``, ``mfe_batch``,
    ``mfcc_packed``, ``mfe_packed`` and ``mfcc_list`` take it too.  Without it an int16 signal is a ``TypeError``.
    """
    sig, scale = _require_signal(signal, (1,), "mfcc", pcm_scale)
    config = _cfg(sampling_frequency, frame_length, frame_stride, num_cepstral, num_filters, fft_length,
                  low_frequency, high_frequency, dc_elimination, switches, sig)
    return _internal_mfcc_batch(sig[None, :], config, scale)[0]


def _internal_mfcc_batches(signals, config: SpeechConfig):
    """Several [B_i, L] batches (same L) -> list of [B_i, T, num_cepstral]: ONE ss_mfcc_batches_device call for device tensors
    (one launch for up to 8 batches where the kernel takes a batch table), one host call per batch for numpy arrays."""
    if not all(_is_torch(x) and x.is_cuda for x in signals):
        return [_internal_mfcc_batch(x, config) for x in signals]
    import torch

    lib = _lib.lib()
    dev = signals[0].device
    L = signals[0].shape[1]
    if any(x.device != dev or x.shape[1] != L for x in signals):
        raise ValueError("mfcc_batch: the batches of one call must live on one device and hold clips of one length")
    T = config.num_frames(L)
    Cc = config.params.num_cepstral
    xs = [x if (x.stride(1) == 1 and (x.shape[0] <= 1 or x.stride(0) == L)) else x.contiguous() for x in signals]
    outs = [torch.empty((x.shape[0], T, Cc), dtype=torch.float32, device=dev) for x in xs]
    n = len(xs)
    px = (C.c_void_p * n)(*[x.data_ptr() for x in xs])
    po = (C.c_void_p * n)(*[o.data_ptr() for o in outs])
    nb = (C.c_size_t * n)(*[x.shape[0] for x in xs])
    with torch.cuda.device(dev):
        _lib.check(lib.ss_mfcc_batches_device(config.handle, n, px, nb, L, L, po, _stream_ptr()))
    return outs


def mfcc_batch(signals, sampling_frequency, frame_length=0.020, frame_stride=0.01, num_cepstral=13, num_filters=40,
               fft_length=512, low_frequency=0, high_frequency=None, dc_elimination=True, pcm_scale=None, **switches):
    """Batch form: [B, L] float32 -> [B, num_frames, num_cepstral] in one launch.  A list / tuple of such batches (same clip
    length; e.g. the blocks a data loader hands over) -> the list of their feature blocks from ONE call: device tensors share one
    kernel launch where the configuration's kernel takes a batch table (ss_mfcc_batches_device).  ``pcm_scale`` (see ``mfcc``):
    a single [B, L] int16 block only."""
    if isinstance(signals, (list, tuple)):
        if pcm_scale is not None:
            raise ValueError("mfcc_batch: pcm_scale takes a single [B, L] block, not a list of batches")
        sigs = [_require_f32(x, (2,), "mfcc_batch") for x in signals]
        if not sigs:
            return []
        config = _cfg(sampling_frequency, frame_length, frame_stride, num_cepstral, num_filters, fft_length,
                      low_frequency, high_frequency, dc_elimination, switches, sigs[0])
        return _internal_mfcc_batches(sigs, config)
    sig, scale = _require_signal(signals, (2,), "mfcc_batch", pcm_scale)
    config = _cfg(sampling_frequency, frame_length, frame_stride, num_cepstral, num_filters, fft_length,
                  low_frequency, high_frequency, dc_elimination, switches, sig)
    return _internal_mfcc_batch(sig, config, scale)


def mfe(signal, sampling_frequency, frame_length=0.020, frame_stride=0.01, num_filters=40, fft_length=512,
        low_frequency=0, high_frequency=None, pcm_scale=None, **switches):
    """Mel filterbank energies and frame energies (feature.rs:200-233): ((T, num_filters), (T,)).  ``pcm_scale``: see ``mfcc``."""
    sig, scale = _require_signal(signal, (1,), "mfe", pcm_scale)
    config = _cfg(sampling_frequency, frame_length, frame_stride, min(13, num_filters), num_filters, fft_length,
                  low_frequency, high_frequency, True, switches, sig)
    feat, en = _internal_mfe_batch(sig[None, :], config, scale)
    return feat[0], en[0]


def mfe_batch(signals, sampling_frequency, frame_length=0.020, frame_stride=0.01, num_filters=40, fft_length=512,
              low_frequency=0, high_frequency=None, pcm_scale=None, **switches):
    sig, scale = _require_signal(signals, (2,), "mfe_batch", pcm_scale)
    config = _cfg(sampling_frequency, frame_length, frame_stride, min(13, num_filters), num_filters, fft_length,
                  low_frequency, high_frequency, True, switches, sig)
    return _internal_mfe_batch(sig, config, scale)


# ---- packed variable-length clips (ss_*_packed*): one call over clips of different lengths ------------------------

def _sample_offsets(lengths, n_buffer: int, what: str):
    """Clip lengths (list, ndarray or tensor on any device) -> sample offsets, an int64 host array of n + 1 (no device needed)."""
    if _is_torch(lengths):
        lengths = lengths.detach().cpu().numpy()
    lens = np.asarray(lengths)
    if lens.ndim != 1:
        raise ValueError(f"{what}: lengths must be 1-D")
    if lens.size and not np.issubdtype(lens.dtype, np.integer):
        raise TypeError(f"{what}: lengths must be integers, got {lens.dtype}")
    lens = lens.astype(np.int64)
    if (lens < 0).any():
        raise ValueError(f"{what}: negative clip length")
    so = np.zeros(lens.size + 1, dtype=np.int64)
    np.cumsum(lens, out=so[1:])
    if so[-1] > n_buffer:
        raise ValueError(f"{what}: the lengths sum to {so[-1]} samples, the signal holds {n_buffer}")
    return so


def _frame_offsets(config: SpeechConfig, so):
    """Sample offsets -> frame offsets (ss_packed_frame_offsets), an int64 host array of n + 1."""
    fo = np.empty_like(so)
    _lib.check(_lib.lib().ss_packed_frame_offsets(C.byref(config.params), so.size - 1, so.ctypes.data, fo.ctypes.data))
    return fo


def _packed_offsets(config: SpeechConfig, lengths, n_buffer: int, what: str):
    """-> sample offsets and frame offsets, int64 host arrays of n + 1."""
    so = _sample_offsets(lengths, n_buffer, what)
    return so, _frame_offsets(config, so)


def _internal_packed(signal, so, config: SpeechConfig, mfe: bool, scale=None):
    """signal [N] packed clips, sample offsets so -> (features [sum T_b, cols], energy [sum T_b] or None, frame_offsets [n + 1]);
    scale: the signal is int16 PCM (the ``_i16`` entry points)."""
    lib = _lib.lib()
    i16, sc = ("", []) if scale is None else ("_i16", [scale])
    fo = _frame_offsets(config, so)
    n, rows = so.size - 1, int(fo[-1])
    cols = config.params.num_filters if mfe else config.params.num_cepstral
    if _is_torch(signal):
        import torch

        x = signal.contiguous()
        with torch.cuda.device(x.device):
            dso, dfo = torch.from_numpy(so).to(x.device), torch.from_numpy(fo).to(x.device)
            out = torch.empty((rows, cols), dtype=torch.float32, device=x.device)
            en = torch.empty((rows,), dtype=torch.float32, device=x.device) if mfe else None
            if mfe:
                _lib.check(getattr(lib, f"ss_mfe_packed{i16}_device")(config.handle, x.data_ptr(), n, dso.data_ptr(), *sc, dfo.data_ptr(),
                                                                      rows, out.data_ptr(), en.data_ptr(), _stream_ptr()))
            else:
                _lib.check(getattr(lib, f"ss_mfcc_packed{i16}_device")(config.handle, x.data_ptr(), n, dso.data_ptr(), *sc, dfo.data_ptr(),
                                                                       rows, out.data_ptr(), _stream_ptr()))
        return out, en, dfo
    x = np.ascontiguousarray(signal)
    out = np.empty((rows, cols), dtype=np.float32)
    en = np.empty((rows,), dtype=np.float32) if mfe else None
    if mfe:
        _lib.check(getattr(lib, f"ss_mfe_packed{i16}")(config.handle, x.ctypes.data, n, so.ctypes.data, *sc, out.ctypes.data, en.ctypes.data))
    else:
        _lib.check(getattr(lib, f"ss_mfcc_packed{i16}")(config.handle, x.ctypes.data, n, so.ctypes.data, *sc, out.ctypes.data))
    return out, en, fo


def mfcc_packed(signal, lengths, sampling_frequency, frame_length=0.020, frame_stride=0.01, num_cepstral=13, num_filters=40,
                fft_length=512, low_frequency=0, high_frequency=None, dc_elimination=True, pcm_scale=None, **switches):
    """MFCC of clips of different lengths packed end to end in one 1-D float32 signal (clip b = the lengths[b] samples after
    the clips before it) -> (features [sum T_b, num_cepstral], frame_offsets [n + 1] int64): clip b's rows are
    frame_offsets[b] : frame_offsets[b + 1], each what ``mfcc`` returns for that clip alone.  One launch for all clips.
    ``pcm_scale``: the packed signal is int16 PCM (see ``mfcc``)."""
    sig, scale = _require_signal(signal, (1,), "mfcc_packed", pcm_scale)
    so = _sample_offsets(lengths, sig.shape[0], "mfcc_packed")
    config = _cfg(sampling_frequency, frame_length, frame_stride, num_cepstral, num_filters, fft_length,
                  low_frequency, high_frequency, dc_elimination, switches, sig)
    out, _, fo = _internal_packed(sig, so, config, False, scale)
    return out, fo


def mfe_packed(signal, lengths, sampling_frequency, frame_length=0.020, frame_stride=0.01, num_filters=40, fft_length=512,
               low_frequency=0, high_frequency=None, pcm_scale=None, **switches):
    """``mfe`` of packed clips (see mfcc_packed) -> (feat [sum T_b, num_filters], energy [sum T_b], frame_offsets [n + 1])."""
    sig, scale = _require_signal(signal, (1,), "mfe_packed", pcm_scale)
    so = _sample_offsets(lengths, sig.shape[0], "mfe_packed")
    config = _cfg(sampling_frequency, frame_length, frame_stride, min(13, num_filters), num_filters, fft_length,
                  low_frequency, high_frequency, True, switches, sig)
    return _internal_packed(sig, so, config, True, scale)


def mfcc_list(signals, sampling_frequency, frame_length=0.020, frame_stride=0.01, num_cepstral=13, num_filters=40,
              fft_length=512, low_frequency=0, high_frequency=None, dc_elimination=True, pcm_scale=None, **switches):
    """A list of 1-D float32 clips of any lengths -> the list of their [T_b, num_cepstral] features (views of one block): the
    clips are packed once and served by one mfcc_packed call.  ``pcm_scale``: the clips are int16 PCM (see ``mfcc``)."""
    sigs = [_require_signal(x, (1,), "mfcc_list", pcm_scale)[0] for x in signals]
    if not sigs:
        return []
    on_device = [_is_torch(x) for x in sigs]  # (_require_f32 turns host tensors into arrays)
    if any(on_device) and not all(on_device):
        raise ValueError("mfcc_list: the clips of one call must all be device tensors or all host arrays")
    if all(on_device):
        import torch

        if any(x.device != sigs[0].device for x in sigs):
            raise ValueError("mfcc_list: the clips of one call must live on one device")
        packed = torch.cat(sigs)
    else:
        packed = np.concatenate(sigs)
    lengths = [int(x.shape[0]) for x in sigs]
    out, fo = mfcc_packed(packed, lengths, sampling_frequency, frame_length, frame_stride, num_cepstral, num_filters,
                          fft_length, low_frequency, high_frequency, dc_elimination, pcm_scale, **switches)
    fo = fo.tolist()
    return [out[fo[b]:fo[b + 1]] for b in range(len(sigs))]


def _row_offsets(config: SpeechConfig, so):
    """Sample offsets -> spectrogram row offsets (ss_packed_row_offsets), an int64 host array of n + 1."""
    ro = np.empty_like(so)
    _lib.check(_lib.lib().ss_packed_row_offsets(C.byref(config.params), so.size - 1, so.ctypes.data, ro.ctypes.data))
    return ro


def _internal_stft_packed(signal, so, config: SpeechConfig, stft: bool, scale=None, db=None):
    """signal [N] packed clips, sample offsets so -> (flat float32 block, row_offsets [n + 1]): mel [num_filters * sum R_b] or stft
    [sum R_b, F, 2].  The row offsets are a device tensor where the signal is one.  scale: the signal is int16 PCM (the ``_i16``
    entry points); db: [ref, amin, top_db] of the ``ss_log_mel_spectrogram_packed*`` forms (mel only)."""
    lib = _lib.lib()
    i16, sc = ("", []) if scale is None else ("_i16", [scale])
    name = "ss_stft_packed" if stft else ("ss_mel_spectrogram_packed" if db is None else "ss_log_mel_spectrogram_packed")
    dbargs = [] if db is None else db
    ro = _row_offsets(config, so)
    n, rows = so.size - 1, int(ro[-1])
    F = config.params.fft_points // 2 + 1
    shape = (rows, F, 2) if stft else (config.params.num_filters * rows,)
    if _is_torch(signal):
        import torch

        x = signal.contiguous()
        with torch.cuda.device(x.device):
            dso, dro = torch.from_numpy(so).to(x.device), torch.from_numpy(ro).to(x.device)
            out = torch.empty(shape, dtype=torch.float32, device=x.device)
            _lib.check(getattr(lib, f"{name}{i16}_device")(config.handle, x.data_ptr(), n, dso.data_ptr(), *sc, dro.data_ptr(), rows, *dbargs,
                                                           out.data_ptr(), _stream_ptr()))
        return out, dro
    x = np.ascontiguousarray(signal)
    out = np.empty(shape, dtype=np.float32)
    _lib.check(getattr(lib, f"{name}{i16}")(config.handle, x.ctypes.data, n, so.ctypes.data, *sc, *dbargs, out.ctypes.data))
    return out, ro


def mel_spectrogram_packed(signal, lengths, sampling_frequency, frame_length=0.020, frame_stride=0.01, num_cepstral=13,
                           num_filters=40, fft_length=512, low_frequency=0, high_frequency=None, dc_elimination=True, pcm_scale=None,
                           _db=None, _what="mel_spectrogram_packed", **switches):
    """Mel spectrogram of clips of different lengths packed end to end in one 1-D float32 signal (clip b = the lengths[b]
    samples after the clips before it) -> (out, row_offsets [n + 1] int64).  ``out`` is the flat float32 block of
    num_filters * sum R_b values: clip b's [num_filters, R_b] block, what ``mel_spectrogram`` returns for that clip alone, starts
    at num_filters * row_offsets[b].  One launch for all clips.  ``pcm_scale``: the packed signal is int16 PCM (see
    ``mel_spectrogram``)."""
    sig, scale = _require_signal(signal, (1,), _what, pcm_scale)
    so = _sample_offsets(lengths, sig.shape[0], _what)
    config = _cfg(sampling_frequency, frame_length, frame_stride, num_cepstral, num_filters, fft_length,
                  low_frequency, high_frequency, dc_elimination, switches, sig)
    return _internal_stft_packed(sig, so, config, False, scale, _db)


def mel_spectrogram_list(signals, sampling_frequency, frame_length=0.020, frame_stride=0.01, num_cepstral=13, num_filters=40,
                         fft_length=512, low_frequency=0, high_frequency=None, dc_elimination=True, pcm_scale=None, _db=None,
                         _what="mel_spectrogram_list", **switches):
    """A list of 1-D float32 clips of any lengths -> the list of their [num_filters, R_b] mel spectrograms (views of one block):
    the clips are packed once and served by one mel_spectrogram_packed call.  ``pcm_scale``: the clips are int16 PCM (see
    ``mel_spectrogram``)."""
    sigs = [_require_signal(x, (1,), _what, pcm_scale)[0] for x in signals]
    if not sigs:
        return []
    on_device = [_is_torch(x) for x in sigs]  # (_require_f32 turns host tensors into arrays)
    if any(on_device) and not all(on_device):
        raise ValueError(f"{_what}: the clips of one call must all be device tensors or all host arrays")
    if all(on_device):
        import torch

        if any(x.device != sigs[0].device for x in sigs):
            raise ValueError(f"{_what}: the clips of one call must live on one device")
        packed = torch.cat(sigs)
    else:
        packed = np.concatenate(sigs)
    lengths = [int(x.shape[0]) for x in sigs]
    out, ro = mel_spectrogram_packed(packed, lengths, sampling_frequency, frame_length, frame_stride, num_cepstral, num_filters,
                                     fft_length, low_frequency, high_frequency, dc_elimination, pcm_scale, _db,
                                     "mel_spectrogram_packed" if _db is None else "log_mel_spectrogram_packed", **switches)
    ro = ro.tolist()
    M = int(num_filters)
    return [out[M * ro[b]:M * ro[b + 1]].reshape(M, ro[b + 1] - ro[b]) for b in range(len(sigs))]


def stft_packed(signal, lengths, sampling_frequency, frame_length=0.020, fft_length=512, pcm_scale=None, **switches):
    """``stft`` of packed clips (see mel_spectrogram_packed) -> (complex64 [sum R_b, fft_length // 2 + 1], row_offsets [n + 1]):
    clip b's rows are row_offsets[b] : row_offsets[b + 1], what ``stft`` returns for that clip alone.  numpy in -> numpy out; a
    ROCm tensor stays on the device (torch.complex64 view of the interleaved block).  ``pcm_scale``: the packed signal is int16
    PCM (see ``mel_spectrogram``)."""
    sig, scale = _require_signal(signal, (1,), "stft_packed", pcm_scale)
    so = _sample_offsets(lengths, sig.shape[0], "stft_packed")
    config = _cfg(sampling_frequency, frame_length, 0.01, 13, 40, fft_length, 0, None, True, switches, sig)
    out, ro = _internal_stft_packed(sig, so, config, True, scale)
    if _is_torch(out):
        import torch

        return torch.view_as_complex(out), ro
    return out.view(np.complex64)[..., 0], ro


def _internal_lmfe_batch(signal, config: SpeechConfig):
    lib = _lib.lib()
    B, L = signal.shape
    T = config.num_frames(L)
    M = config.params.num_filters
    if _is_torch(signal):
        import torch

        x = signal if signal.stride(1) == 1 else signal.contiguous()
        feat = torch.empty((B, T, M), dtype=torch.float32, device=x.device)
        with torch.cuda.device(x.device):
            _lib.check(lib.ss_lmfe_batch_device(config.handle, x.data_ptr(), B, L, x.stride(0) if B > 1 else L,
                                                feat.data_ptr(), None, _stream_ptr()))
        return feat
    x = np.ascontiguousarray(signal)
    feat = np.empty((B, T, M), dtype=np.float32)
    _lib.check(lib.ss_lmfe_batch(config.handle, x.ctypes.data, B, L, L, feat.ctypes.data))
    return feat


def lmfe(signal, sampling_frequency, frame_length=0.020, frame_stride=0.01, num_filters=40, fft_length=512,
         low_frequency=0, high_frequency=None, **switches):
    """Log mel-filterbank energies (feature.rs:242-245; README.md:14): ln of mfe's features, (T, num_filters)."""
    sig = _require_f32(signal, (1,), "lmfe")
    config = _cfg(sampling_frequency, frame_length, frame_stride, min(13, num_filters), num_filters, fft_length,
                  low_frequency, high_frequency, True, switches, sig)
    return _internal_lmfe_batch(sig[None, :], config)[0]


def lmfe_batch(signals, sampling_frequency, frame_length=0.020, frame_stride=0.01, num_filters=40, fft_length=512,
               low_frequency=0, high_frequency=None, **switches):
    sig = _require_f32(signals, (2,), "lmfe_batch")
    config = _cfg(sampling_frequency, frame_length, frame_stride, min(13, num_filters), num_filters, fft_length,
                  low_frequency, high_frequency, True, switches, sig)
    return _internal_lmfe_batch(sig, config)


def lmfe_packed(signal, lengths, sampling_frequency, frame_length=0.020, frame_stride=0.01, num_filters=40, fft_length=512,
                low_frequency=0, high_frequency=None, **switches):
    """``lmfe`` of packed clips (see mfcc_packed) -> (feat [sum T_b, num_filters], frame_offsets [n + 1]): clip b's rows are what
    ``lmfe`` returns for that clip alone."""
    lib = _lib.lib()
    sig = _require_f32(signal, (1,), "lmfe_packed")
    so = _sample_offsets(lengths, sig.shape[0], "lmfe_packed")
    config = _cfg(sampling_frequency, frame_length, frame_stride, min(13, num_filters), num_filters, fft_length,
                  low_frequency, high_frequency, True, switches, sig)
    fo = _frame_offsets(config, so)
    n, rows, M = so.size - 1, int(fo[-1]), config.params.num_filters
    if _is_torch(sig):
        import torch

        x = sig.contiguous()
        with torch.cuda.device(x.device):
            dso, dfo = torch.from_numpy(so).to(x.device), torch.from_numpy(fo).to(x.device)
            feat = torch.empty((rows, M), dtype=torch.float32, device=x.device)
            _lib.check(lib.ss_lmfe_packed_device(config.handle, x.data_ptr(), n, dso.data_ptr(), dfo.data_ptr(), rows,
                                                 feat.data_ptr(), None, _stream_ptr()))
        return feat, dfo
    x = np.ascontiguousarray(sig)
    feat = np.empty((rows, M), dtype=np.float32)
    _lib.check(lib.ss_lmfe_packed(config.handle, x.ctypes.data, n, so.ctypes.data, feat.ctypes.data))
    return feat, fo


def power_to_db(S, ref=1.0, amin=1e-10, top_db=80.0):
    """librosa.power_to_db: 10 log10(max(amin, S)) - 10 log10(max(amin, |ref|)), floored at max - top_db (None: no floor).
    The reference lists librosa's mel-spectrogram conventions as its remaining work (README.md:44-46).  numpy in -> numpy
    out; a ROCm tensor stays on the device (current stream)."""
    lib = _lib.lib()
    td = -1.0 if top_db is None else float(top_db)
    if top_db is not None and top_db < 0:
        raise ValueError("top_db must be non-negative")
    if _is_torch(S) and S.is_cuda:
        import torch

        if S.dtype != torch.float32:
            raise TypeError("power_to_db: expected float32")
        x = S.contiguous()
        out = torch.empty_like(x)
        with torch.cuda.device(x.device):
            _lib.check(lib.ss_power_to_db_device(x.data_ptr(), x.numel(), float(ref), float(amin), td, out.data_ptr(), _stream_ptr()))
        return out
    arr = np.ascontiguousarray(S.numpy() if _is_torch(S) else S)
    if arr.dtype != np.float32:
        raise TypeError("power_to_db: expected float32")
    out = np.empty_like(arr)
    _lib.check(lib.ss_power_to_db(arr.ctypes.data, arr.size, float(ref), float(amin), td, out.ctypes.data))
    return out


def mel_spectrogram(signal, sampling_frequency, frame_length=0.020, frame_stride=0.01, num_cepstral=13,
                    num_filters=40, fft_length=512, low_frequency=0, high_frequency=None, dc_elimination=True,
                    pcm_scale=None, **switches):
    """Mel spectrogram of a 1-D or 2-D float32 signal -> (..., n_mels, time).

    Mirrors ``speechsauce.mel_spectrogram`` (py-speechsauce/speechsauce/__init__.py:85-132 ->
    feature.rs:151-174).  The STFT hop is ``frame_length * sampling_frequency`` samples and the
    window is ``fft_length`` samples (config.rs:154, functions.rs:96-101); the reference panics
    unless ``fft_length >= 2 * hop`` -- that raises SpeechSauceError here.

    ``pcm_scale``: the signal is int16 PCM, converted on load as ``int16 * pcm_scale`` (see ``mfcc``); the result is bit for bit
    that of the float call on ``signal.astype(float32) * pcm_scale`` (``ss_mel_spectrogram_i16*``).
    """
    if isinstance(signal, (list, tuple)):
        if pcm_scale is not None:
            raise ValueError("mel_spectrogram: pcm_scale takes a single signal, not a list of blocks")
        # several [C_i, L] blocks (same L) -> the list of their [C_i, n_mels, time] spectrograms from ONE call (device tensors:
        # ss_mel_spectrogram_batches_device -- one launch where the configuration's kernel takes a batch table)
        sigs = [_require_f32(x, (2,), "mel_spectrogram") for x in signal]
        if not sigs:
            return []
        config = _cfg(sampling_frequency, frame_length, frame_stride, num_cepstral, num_filters, fft_length,
                      low_frequency, high_frequency, dc_elimination, switches, sigs[0])
        return _internal_mel_spectrogram_batches(sigs, config)
    sig, scale = _require_signal(signal, (1, 2), "mel_spectrogram", pcm_scale)
    config = _cfg(sampling_frequency, frame_length, frame_stride, num_cepstral, num_filters, fft_length,
                  low_frequency, high_frequency, dc_elimination, switches, sig)
    return _internal_mel_spectrogram(sig, config, scale)


def _db_args(what, ref, amin, top_db):
    """[ref, amin, top_db] of the ``ss_log_mel_spectrogram*`` calls; the argument rules of ``power_to_db`` (top_db None: no floor,
    -1 in the ABI), checked before a device is touched."""
    if top_db is not None and top_db < 0:
        raise ValueError(f"{what}: top_db must be non-negative")
    if not float(amin) > 0:
        raise ValueError(f"{what}: amin must be strictly positive")
    if float(ref) != float(ref):
        raise ValueError(f"{what}: ref must not be NaN")
    return [float(ref), float(amin), -1.0 if top_db is None else float(top_db)]


def log_mel_spectrogram(signal, sampling_frequency, frame_length=0.020, frame_stride=0.01, num_cepstral=13,
                        num_filters=40, fft_length=512, low_frequency=0, high_frequency=None, dc_elimination=True,
                        ref=1.0, amin=1e-10, top_db=80.0, pcm_scale=None, **switches):
    """Log-mel spectrogram of a 1-D or 2-D float32 signal -> (..., n_mels, time) in decibels: ``mel_spectrogram`` with librosa's
    ``power_to_db`` applied PER CLIP (channel) in the mel kernel's epilogue (``ss_log_mel_spectrogram*``).  Bit for bit
    ``power_to_db_packed(mel_spectrogram(...))`` with every clip as its own segment: the ``top_db`` floor is each clip's own
    maximum - top_db (``None``: no floor), and the trailing zero rows come out as 10 log10(amin) - ref_db.  This is not
    ``power_to_db`` of a multi-channel block, which takes one maximum over the whole block.  ``ref`` / ``amin`` / ``top_db`` follow
    ``power_to_db``'s rules; ``pcm_scale``: the signal is int16 PCM (see ``mel_spectrogram``).  numpy in -> numpy out; a ROCm
    tensor stays on the device (current stream)."""
    db = _db_args("log_mel_spectrogram", ref, amin, top_db)
    sig, scale = _require_signal(signal, (1, 2), "log_mel_spectrogram", pcm_scale)
    config = _cfg(sampling_frequency, frame_length, frame_stride, num_cepstral, num_filters, fft_length,
                  low_frequency, high_frequency, dc_elimination, switches, sig)
    return _internal_mel_spectrogram(sig, config, scale, db)


def log_mel_spectrogram_packed(signal, lengths, sampling_frequency, frame_length=0.020, frame_stride=0.01, num_cepstral=13,
                               num_filters=40, fft_length=512, low_frequency=0, high_frequency=None, dc_elimination=True,
                               ref=1.0, amin=1e-10, top_db=80.0, pcm_scale=None, **switches):
    """``log_mel_spectrogram`` of packed clips -> (out, row_offsets), the layout of ``mel_spectrogram_packed``: clip b's
    [num_filters, R_b] block in decibels, floored at its own maximum - top_db, starts at num_filters * row_offsets[b].  Bit for bit
    ``power_to_db_packed(out, row_offsets, cols=num_filters, ...)`` of ``mel_spectrogram_packed``'s result, without that pass."""
    db = _db_args("log_mel_spectrogram_packed", ref, amin, top_db)
    return mel_spectrogram_packed(signal, lengths, sampling_frequency, frame_length, frame_stride, num_cepstral, num_filters, fft_length,
                                  low_frequency, high_frequency, dc_elimination, pcm_scale, db, "log_mel_spectrogram_packed", **switches)


def log_mel_spectrogram_list(signals, sampling_frequency, frame_length=0.020, frame_stride=0.01, num_cepstral=13, num_filters=40,
                             fft_length=512, low_frequency=0, high_frequency=None, dc_elimination=True, ref=1.0, amin=1e-10,
                             top_db=80.0, pcm_scale=None, **switches):
    """A list of 1-D clips of any lengths -> the list of their [num_filters, R_b] log-mel spectrograms (views of one block): the
    clips are packed once and served by one ``log_mel_spectrogram_packed`` call."""
    db = _db_args("log_mel_spectrogram_list", ref, amin, top_db)
    return mel_spectrogram_list(signals, sampling_frequency, frame_length, frame_stride, num_cepstral, num_filters, fft_length,
                                low_frequency, high_frequency, dc_elimination, pcm_scale, db, "log_mel_spectrogram_list", **switches)


# ---- stage outputs the reference exposes as pub fns: processing::{stack_frames, power_spectrum}, functions::{stft1, stft2} ----

def stft(signal, sampling_frequency, frame_length=0.020, fft_length=512, pcm_scale=None, **switches):
    """``speechsauce::functions::stft1`` (1-D signal, functions.rs:199-233) / ``stft2`` (2-D [C, L], functions.rs:86-123):
    complex64 spectrum rows ``(..., rows, fft_length // 2 + 1)`` of the Vorbis-windowed chunks, scaled by wnorm, from zero
    state per clip.  The hop is ``frame_length * sampling_frequency`` samples, the window ``fft_length`` samples
    (config.rs:154); ``fft_length >= 2 * hop`` as in ``mel_spectrogram``.  numpy in -> numpy out; a ROCm tensor stays on
    the device (torch.complex64 view of the interleaved block).  ``pcm_scale``: the signal is int16 PCM (see
    ``mel_spectrogram``)."""
    sig, scale = _require_signal(signal, (1, 2), "stft", pcm_scale)
    config = _cfg(sampling_frequency, frame_length, 0.01, 13, 40, fft_length, 0, None, True, switches, sig)
    lib = _lib.lib()
    i16, sc = ("", []) if scale is None else ("_i16", [scale])
    one_d = sig.ndim == 1
    sig2 = sig[None, :] if one_d else sig
    ch, L = sig2.shape
    R, _ = config.stft_rows(L)
    F = config.params.fft_points // 2 + 1
    if _is_torch(sig2):
        import torch

        x = sig2 if sig2.stride(1) == 1 else sig2.contiguous()
        out = torch.empty((ch, R, F, 2), dtype=torch.float32, device=x.device)
        with torch.cuda.device(x.device):
            _lib.check(getattr(lib, f"ss_stft{i16}_device")(config.handle, x.data_ptr(), ch, L, x.stride(0) if ch > 1 else L, *sc, out.data_ptr(),
                                                            _stream_ptr()))
        z = torch.view_as_complex(out)
    else:
        x = np.ascontiguousarray(sig2)
        out = np.empty((ch, R, F, 2), dtype=np.float32)
        _lib.check(getattr(lib, f"ss_stft{i16}")(config.handle, x.ctypes.data, ch, L, *sc, out.ctypes.data))
        z = out.view(np.complex64)[..., 0]
    return z[0] if one_d else z


# ---- streaming STFT / mel spectrogram with carried state (functions.rs:86-170, config.rs:126,162) --------------------------

STREAM_MODES = {"reference": 0, "continuous": 1}  # SS_STREAM_REFERENCE, SS_STREAM_CONTINUOUS


class _StreamBase:
    """Chunks of ``n_streams`` live audio streams in, spectrogram rows out, with the last ``fft_length - hop`` samples of every
    stream carried from call to call (the reference's ``analysis_mem``).  ``mode="continuous"``: chunks of whole hops, one real
    row per hop; ``mode="reference"``: exactly what the reference's ``stft1`` / ``mel_spectrogram1`` return on a ``SpeechConfig``
    that has seen the earlier chunks.  See ``ss_mel_spectrogram_stream`` in ``include/speechsauce_amd.h``."""

    _what = ""

    def __init__(self, n_streams, sampling_frequency, frame_length, frame_stride, num_cepstral, num_filters, fft_length,
                 low_frequency, high_frequency, dc_elimination, mode, switches):
        if mode not in STREAM_MODES:
            raise ValueError(f"{self._what}: mode must be one of {sorted(STREAM_MODES)}, got {mode!r}")
        if int(n_streams) < 1:
            raise ValueError(f"{self._what}: n_streams must be at least 1")
        self.n_streams = int(n_streams)
        self.mode = mode
        self._args = (sampling_frequency, frame_length, frame_stride, num_cepstral, num_filters, fft_length, low_frequency,
                      high_frequency, dc_elimination, dict(switches))
        self._params = make_params(sample_rate=sampling_frequency, fft_points=fft_length, frame_length=frame_length,
                                   frame_stride=frame_stride, num_cepstral=num_cepstral, num_filters=num_filters,
                                   low_frequency=low_frequency, high_frequency=high_frequency, dc_elimination=dc_elimination,
                                   **switches)
        S = C.c_size_t()
        _lib.check(_lib.lib().ss_stream_state_len(C.byref(self._params), C.byref(S)))  # no STFT path: SS_ERR_BAD_CONFIG here
        self.state_len = S.value
        self.hop = int(fft_length) - self.state_len
        self._state = None
        self._where = None

    @property
    def state(self):
        """[n_streams, fft_length - hop] float32: a torch tensor on the device of the first chunk, or a numpy array; None before
        the first call."""
        return self._state

    def reset(self, streams=None):
        """Zero the state of every stream, or of the given stream indices (a fresh stream)."""
        if self._state is None:
            return
        if streams is None:
            self._state[...] = 0
        else:
            idx = list(np.atleast_1d(np.asarray(streams, dtype=np.int64)))
            if idx:
                self._state[idx] = 0

    def _rows(self, n):
        r, rr = C.c_size_t(), C.c_size_t()
        _lib.check(_lib.lib().ss_stream_rows(C.byref(self._params), STREAM_MODES[self.mode], n, C.byref(r), C.byref(rr)))
        return r.value

    def _prepare(self, chunk):
        sig = _require_f32(chunk, (1, 2), self._what)
        if sig.ndim == 1:
            if self.n_streams != 1:
                raise ValueError(f"{self._what}: a 1-D chunk needs n_streams == 1, this object has {self.n_streams}")
            sig = sig[None, :]
        if sig.shape[0] != self.n_streams:
            raise ValueError(f"{self._what}: chunk has {sig.shape[0]} streams, expected {self.n_streams}")
        n = sig.shape[1]
        if n == 0:
            raise ValueError(f"{self._what}: empty chunk")
        if self.mode == "continuous" and n % self.hop:
            raise ValueError(f"{self._what}: continuous mode takes whole hops: {n} samples is not a multiple of {self.hop}")
        on_dev = _is_torch(sig)
        where = ("cuda", sig.device.index) if on_dev else ("host",)
        if self._state is None:
            if on_dev:
                import torch

                self._state = torch.zeros((self.n_streams, self.state_len), dtype=torch.float32, device=sig.device)
            else:
                self._state = np.zeros((self.n_streams, self.state_len), dtype=np.float32)
            self._where = where
        elif where != self._where:
            raise ValueError(f"{self._what}: the state lives on {self._where}, this chunk on {where}")
        a = self._args
        config = _cfg(*a[:9], a[9], sig)
        return sig, n, self._rows(n), config

    def _launch(self, sig, n, config, out, dev_fn, host_fn):
        lib = _lib.lib()
        B = self.n_streams
        mode = STREAM_MODES[self.mode]
        if _is_torch(sig):
            import torch

            x = sig if sig.stride(1) == 1 else sig.contiguous()
            with torch.cuda.device(x.device):
                _lib.check(getattr(lib, dev_fn)(config.handle, mode, x.data_ptr(), B, n, x.stride(0) if B > 1 else n,
                                                self._state.data_ptr(), out.data_ptr(), _stream_ptr()))
        else:
            x = np.ascontiguousarray(sig)
            _lib.check(getattr(lib, host_fn)(config.handle, mode, x.ctypes.data, B, n, n, self._state.ctypes.data, out.ctypes.data))


class MelSpectrogramStream(_StreamBase):
    """Streaming ``mel_spectrogram``: ``__call__(chunk [n_streams, n])`` -> ``[n_streams, num_filters, rows]``."""

    _what = "MelSpectrogramStream"

    def __init__(self, n_streams, sampling_frequency, frame_length=0.020, num_filters=40, fft_length=512, low_frequency=0,
                 high_frequency=None, mode="continuous", **switches):
        super().__init__(n_streams, sampling_frequency, frame_length, 0.01, 13, num_filters, fft_length, low_frequency,
                         high_frequency, True, mode, switches)

    def __call__(self, chunk):
        sig, n, R, config = self._prepare(chunk)
        M = config.params.num_filters
        if _is_torch(sig):
            import torch

            out = torch.empty((self.n_streams, M, R), dtype=torch.float32, device=sig.device)
        else:
            out = np.empty((self.n_streams, M, R), dtype=np.float32)
        self._launch(sig, n, config, out, "ss_mel_spectrogram_stream_device", "ss_mel_spectrogram_stream")
        return out


class StftStream(_StreamBase):
    """Streaming ``stft``: ``__call__(chunk [n_streams, n])`` -> complex64 ``[n_streams, rows, fft_length // 2 + 1]``."""

    _what = "StftStream"

    def __init__(self, n_streams, sampling_frequency, frame_length=0.020, fft_length=512, mode="continuous", **switches):
        super().__init__(n_streams, sampling_frequency, frame_length, 0.01, 13, 40, fft_length, 0, None, True, mode, switches)

    def __call__(self, chunk):
        sig, n, R, config = self._prepare(chunk)
        F = config.params.fft_points // 2 + 1
        if _is_torch(sig):
            import torch

            out = torch.empty((self.n_streams, R, F, 2), dtype=torch.float32, device=sig.device)
            self._launch(sig, n, config, out, "ss_stft_stream_device", "ss_stft_stream")
            return torch.view_as_complex(out)
        out = np.empty((self.n_streams, R, F, 2), dtype=np.float32)
        self._launch(sig, n, config, out, "ss_stft_stream_device", "ss_stft_stream")
        return out.view(np.complex64)[..., 0]


# ---- streaming MFCC / mfe with carried frame state (feature.rs:99-233 over live audio) --------------------------------------

class _FrameStreamBase(_StreamBase):
    """Chunks of whole hops of ``n_streams`` live audio streams in, one MFCC / mfe row per hop out, with the last
    ``max(frame_len + preemph_shift - hop, 0)`` samples of every stream carried from call to call (continuous mode only: the
    reference's ``mfcc`` / ``mfe`` keep no state).  The state handling and chunk checks are ``_StreamBase``'s.  See
    ``ss_mfcc_stream`` in ``include/speechsauce_amd.h``."""

    def __init__(self, n_streams, sampling_frequency, frame_length, frame_stride, num_cepstral, num_filters, fft_length,
                 low_frequency, high_frequency, dc_elimination, switches):
        if int(n_streams) < 1:
            raise ValueError(f"{self._what}: n_streams must be at least 1")
        self.n_streams = int(n_streams)
        self.mode = "continuous"
        self._args = (sampling_frequency, frame_length, frame_stride, num_cepstral, num_filters, fft_length, low_frequency,
                      high_frequency, dc_elimination, dict(switches))
        self._params = make_params(sample_rate=sampling_frequency, fft_points=fft_length, frame_length=frame_length,
                                   frame_stride=frame_stride, num_cepstral=num_cepstral, num_filters=num_filters,
                                   low_frequency=low_frequency, high_frequency=high_frequency, dc_elimination=dc_elimination,
                                   **switches)
        lib = _lib.lib()
        S, fl, st = C.c_size_t(), C.c_size_t(), C.c_size_t()
        _lib.check(lib.ss_frame_stream_state_len(C.byref(self._params), C.byref(S)))  # literal / centred framing: SS_ERR_BAD_CONFIG
        _lib.check(lib.ss_frame_sizes(C.byref(self._params), C.byref(fl), C.byref(st)))
        self.state_len = S.value
        self.frame_len = fl.value
        self.hop = st.value
        self._state = None
        self._where = None

    def _rows(self, n):
        r = C.c_size_t()
        _lib.check(_lib.lib().ss_frame_stream_rows(C.byref(self._params), n, C.byref(r)))
        return r.value

    def _call(self, sig, n, config, outs, dev_fn, host_fn, extra):
        lib = _lib.lib()
        B = self.n_streams
        ptrs = [o.data_ptr() if _is_torch(o) else o.ctypes.data for o in outs]
        if _is_torch(sig):
            import torch

            x = sig if sig.stride(1) == 1 else sig.contiguous()
            with torch.cuda.device(x.device):
                st = self._state.data_ptr() if self.state_len else None
                _lib.check(getattr(lib, dev_fn)(config.handle, x.data_ptr(), B, n, x.stride(0) if B > 1 else n, *extra, st, *ptrs,
                                                _stream_ptr()))
        else:
            x = np.ascontiguousarray(sig)
            st = self._state.ctypes.data if self.state_len else None
            _lib.check(getattr(lib, host_fn)(config.handle, x.ctypes.data, B, n, n, *extra, st, *ptrs))


class MfccStream(_FrameStreamBase):
    """Streaming ``mfcc``: ``__call__(chunk [n_streams, n])`` -> ``[n_streams, n // hop, num_cepstral]``, one row per hop.
    ``norm_frames``: the frame count T of the reference DCT scaling n = T * num_filters (feature.rs:126-131), typically the
    frame count of the model's input window; required under the reference DCT, ignored with ``dct_norm="ortho"``."""

    _what = "MfccStream"

    def __init__(self, n_streams, sampling_frequency, frame_length=0.020, frame_stride=0.01, num_cepstral=13, num_filters=40,
                 fft_length=512, low_frequency=0, high_frequency=None, dc_elimination=True, norm_frames=None, **switches):
        super().__init__(n_streams, sampling_frequency, frame_length, frame_stride, num_cepstral, num_filters, fft_length,
                         low_frequency, high_frequency, dc_elimination, switches)
        if self._params.dct_norm == 0:  # SS_DCT_REFERENCE
            if norm_frames is None or int(norm_frames) < 1:
                raise ValueError("MfccStream: the reference DCT scaling needs norm_frames >= 1 (the frame count it scales by)")
            self.norm_frames = int(norm_frames)
        else:
            self.norm_frames = int(norm_frames) if norm_frames is not None else 1

    def __call__(self, chunk):
        sig, n, R, config = self._prepare(chunk)
        Cc = config.params.num_cepstral
        if _is_torch(sig):
            import torch

            out = torch.empty((self.n_streams, R, Cc), dtype=torch.float32, device=sig.device)
        else:
            out = np.empty((self.n_streams, R, Cc), dtype=np.float32)
        self._call(sig, n, config, [out], "ss_mfcc_stream_device", "ss_mfcc_stream", [self.norm_frames])
        return out


class MfeStream(_FrameStreamBase):
    """Streaming ``mfe``: ``__call__(chunk [n_streams, n])`` -> ``(feat [n_streams, n // hop, num_filters], energy [n_streams,
    n // hop])``, one row per hop."""

    _what = "MfeStream"

    def __init__(self, n_streams, sampling_frequency, frame_length=0.020, frame_stride=0.01, num_filters=40, fft_length=512,
                 low_frequency=0, high_frequency=None, **switches):
        super().__init__(n_streams, sampling_frequency, frame_length, frame_stride, min(13, num_filters), num_filters, fft_length,
                         low_frequency, high_frequency, True, switches)

    def __call__(self, chunk):
        sig, n, R, config = self._prepare(chunk)
        M = config.params.num_filters
        if _is_torch(sig):
            import torch

            feat = torch.empty((self.n_streams, R, M), dtype=torch.float32, device=sig.device)
            energy = torch.empty((self.n_streams, R), dtype=torch.float32, device=sig.device)
        else:
            feat = np.empty((self.n_streams, R, M), dtype=np.float32)
            energy = np.empty((self.n_streams, R), dtype=np.float32)
        self._call(sig, n, config, [feat, energy], "ss_mfe_stream_device", "ss_mfe_stream", [])
        return feat, energy

# ---- ragged streaming over a pool of stream states ---------------------------------------------------------------------------

def _pool_slots(slots, pool_streams, what, entry="entry"):
    """The slot rule of every pool call: integers inside the pool, none named twice -> the list."""
    slot_list = [int(v) for v in slots]
    seen = set()
    for i, v in enumerate(slot_list):
        if not 0 <= v < pool_streams:
            raise ValueError(f"{what}: slot {v} of {entry} {i} is outside the pool of {pool_streams} streams")
        if v in seen:
            raise ValueError(f"{what}: slot {v} is named twice in one call")
        seen.add(v)
    return slot_list


class _StreamPoolMixin:
    """The pool plumbing of the ragged streaming classes, in front of a dense streaming base (``_FrameStreamBase`` or
    ``_StreamBase``) whose ``n_streams`` is the pool size: the argument rules of ``pool(chunks, slots, lengths=None)``, the pool
    block and its place, the offset tables and the call itself."""

    def __init__(self, pool_streams, *args):
        super().__init__(pool_streams, *args)
        self.pool_streams = self.n_streams

    @property
    def state(self):
        """[pool_streams, state_len] float32: a torch tensor on the device of the first chunks, or a numpy array; None before
        the first call."""
        return self._state

    def reset(self, slots=None):
        """Zero the state of every stream of the pool, or of the given slots (fresh streams)."""
        super().reset(slots)

    def _prepare_pool(self, chunks, slots, lengths, pcm=False):
        what = self._what
        require = (lambda c: _require_i16(c, what)) if pcm else (lambda c: _require_f32(c, (1,), what))
        if lengths is None:
            if _is_torch(chunks) or isinstance(chunks, np.ndarray):
                raise TypeError(f"{what}: chunks must be a list of 1-D arrays (or pass a packed buffer with lengths=)")
            parts = [require(c) for c in chunks]
            lens = [int(c.shape[0]) for c in parts]
            kinds = {_is_torch(c) for c in parts}
            if len(kinds) > 1:
                raise TypeError(f"{what}: chunks must be all numpy arrays or all tensors on one device")
            packed = None
        else:
            packed = require(chunks)
            parts = None
            lens = [int(v) for v in lengths]
            if any(v < 0 for v in lens) or sum(lens) != int(packed.shape[0]):
                raise ValueError(f"{what}: lengths must be non-negative and sum to the packed buffer's {int(packed.shape[0])} samples")
        slot_list = [int(v) for v in slots]
        if len(slot_list) != len(lens):
            raise ValueError(f"{what}: {len(lens)} chunks but {len(slot_list)} slots")
        for i, n in enumerate(lens):
            if n % self.hop:
                raise ValueError(f"{what}: chunk {i} has {n} samples, not a multiple of the hop {self.hop}")
        _pool_slots(slot_list, self.pool_streams, what, "chunk")
        first = packed if packed is not None else (parts[0] if parts else None)
        on_dev = first is not None and _is_torch(first)
        if first is None:  # nothing to serve: the place of the pool decides, the host before any call
            on_dev = self._where is not None and self._where[0] == "cuda"
        if on_dev:
            import torch

            dev = first.device if first is not None else self._state.device
            if packed is None:
                if any(c.device != dev for c in parts):
                    raise TypeError(f"{what}: chunks must be all numpy arrays or all tensors on one device")
                packed = torch.cat(parts) if parts else torch.empty(0, dtype=torch.int16 if pcm else torch.float32, device=dev)
            where = ("cuda", dev.index)
        else:
            if packed is None:
                packed = np.concatenate(parts) if parts else np.empty(0, dtype=np.int16 if pcm else np.float32)
            where = ("host",)
        if self._where is not None and where != self._where:
            raise ValueError(f"{what}: the pool lives on {self._where}, these chunks on {where}")
        config = self._config_for(packed)
        if self._state is None:
            if on_dev:
                self._state = torch.zeros((self.pool_streams, self.state_len), dtype=torch.float32, device=packed.device)
            else:
                self._state = np.zeros((self.pool_streams, self.state_len), dtype=np.float32)
            self._where = where
        so = np.zeros(len(lens) + 1, dtype=np.int64)
        np.cumsum(lens, out=so[1:])
        ro = so // self.hop
        return packed, so, ro, np.asarray(slot_list, dtype=np.int32), config

    def _config_for(self, packed):
        """The handle that serves ``packed`` where it lives."""
        a = self._args
        return _cfg(*a[:9], a[9], packed)

    def _prepare_pcm(self, chunks, slots, lengths, pcm_scale):
        """``_prepare_pool`` of either chunk format, and what ``_call_pool`` needs for it: the suffix of the entry points' names
        and the arguments between ``pool_streams`` and the state."""
        if pcm_scale is None:
            return self._prepare_pool(chunks, slots, lengths), "", []
        scale = _check_pcm_scale(pcm_scale, self._what)
        return self._prepare_pool(chunks, slots, lengths, pcm=True), "_i16", [scale]

    def _call_pool(self, packed, so, ro, sl, config, outs, dev_fn, host_fn, extra):
        lib = _lib.lib()
        n_active = sl.size
        if n_active == 0:
            return
        ptrs = [o.data_ptr() if _is_torch(o) else o.ctypes.data for o in outs]
        if _is_torch(packed):
            x = packed.contiguous()
            if x.data_ptr() & 3:  # (int16 only: the device form reads sample pairs as dwords)
                x = x.clone()
            st = self._state.data_ptr() if self.state_len else None
            _launch(x.device, getattr(lib, dev_fn), config.handle, x, n_active, so, ro, int(ro[-1]), sl, self.pool_streams, *extra, st, *ptrs)
        else:
            x = np.ascontiguousarray(packed)
            st = self._state.ctypes.data if self.state_len else None
            _lib.check(getattr(lib, host_fn)(config.handle, x.ctypes.data, n_active, so.ctypes.data, sl.ctypes.data, self.pool_streams,
                                             *extra, st, *ptrs))


class _FrameStreamPoolBase(_StreamPoolMixin, _FrameStreamBase):
    """A pool of ``pool_streams`` live audio streams, each with the carried state of ``MfccStream`` / ``MfeStream``.  One call
    serves any subset of them, each with its own number of whole hops (zero included): ``pool(chunks, slots)`` with ``chunks`` a
    list of 1-D float32 arrays / tensors, or one packed 1-D buffer plus ``lengths=``, and ``slots`` the pool row of each chunk
    (distinct).  Per stream the rows and the carried state are those of the dense class on that stream alone.  numpy in -> the
    host-pointer call, ROCm tensors in -> the device call on the current stream.  See ``ss_mfcc_stream_packed`` in
    ``include/speechsauce_amd.h``.

    ``pool(chunks, slots, pcm_scale=2**-15)`` takes the chunks (or the packed buffer) as signed 16-bit PCM instead -- int16
    arrays / tensors only -- and converts on load: stream sample = ``int16 * pcm_scale``, ``pcm_scale`` a power of two in
    ``[2**-64, 2**64]``.  The rows and the state are bit for bit those of the float call on ``chunk.astype(float32) * pcm_scale``;
    the state stays float32, so a stream may be fed PCM on one call and floats on the next (``ss_mfcc_stream_packed_i16``)."""


class MfccStreamPool(_FrameStreamPoolBase):
    """Ragged streaming ``mfcc``: ``pool(chunks, slots)`` -> ``(rows [total_rows, num_cepstral], row_offsets)``; chunk ``i``'s
    ``len(chunk) // hop`` rows are ``rows[row_offsets[i]:row_offsets[i + 1]]`` (``row_offsets``: int64 numpy array).
    ``norm_frames`` as for ``MfccStream``."""

    _what = "MfccStreamPool"

    def __init__(self, pool_streams, sampling_frequency, frame_length=0.020, frame_stride=0.01, num_cepstral=13, num_filters=40,
                 fft_length=512, low_frequency=0, high_frequency=None, dc_elimination=True, norm_frames=None, **switches):
        super().__init__(pool_streams, sampling_frequency, frame_length, frame_stride, num_cepstral, num_filters, fft_length,
                         low_frequency, high_frequency, dc_elimination, switches)
        if self._params.dct_norm == 0:  # SS_DCT_REFERENCE
            if norm_frames is None or int(norm_frames) < 1:
                raise ValueError("MfccStreamPool: the reference DCT scaling needs norm_frames >= 1 (the frame count it scales by)")
            self.norm_frames = int(norm_frames)
        else:
            self.norm_frames = int(norm_frames) if norm_frames is not None else 1

    def __call__(self, chunks, slots, lengths=None, pcm_scale=None):
        (packed, so, ro, sl, config), i16, scale = self._prepare_pcm(chunks, slots, lengths, pcm_scale)
        Cc, R = config.params.num_cepstral, int(ro[-1])
        if _is_torch(packed):
            import torch

            out = torch.empty((R, Cc), dtype=torch.float32, device=packed.device)
        else:
            out = np.empty((R, Cc), dtype=np.float32)
        self._call_pool(packed, so, ro, sl, config, [out], f"ss_mfcc_stream_packed{i16}_device", f"ss_mfcc_stream_packed{i16}",
                        scale + [self.norm_frames])
        return out, ro


class MfeStreamPool(_FrameStreamPoolBase):
    """Ragged streaming ``mfe``: ``pool(chunks, slots)`` -> ``(feat [total_rows, num_filters], energy [total_rows],
    row_offsets)``."""

    _what = "MfeStreamPool"

    def __init__(self, pool_streams, sampling_frequency, frame_length=0.020, frame_stride=0.01, num_filters=40, fft_length=512,
                 low_frequency=0, high_frequency=None, **switches):
        super().__init__(pool_streams, sampling_frequency, frame_length, frame_stride, min(13, num_filters), num_filters, fft_length,
                         low_frequency, high_frequency, True, switches)

    def __call__(self, chunks, slots, lengths=None, pcm_scale=None):
        (packed, so, ro, sl, config), i16, scale = self._prepare_pcm(chunks, slots, lengths, pcm_scale)
        M, R = config.params.num_filters, int(ro[-1])
        if _is_torch(packed):
            import torch

            feat = torch.empty((R, M), dtype=torch.float32, device=packed.device)
            energy = torch.empty((R,), dtype=torch.float32, device=packed.device)
        else:
            feat = np.empty((R, M), dtype=np.float32)
            energy = np.empty((R,), dtype=np.float32)
        self._call_pool(packed, so, ro, sl, config, [feat, energy], f"ss_mfe_stream_packed{i16}_device", f"ss_mfe_stream_packed{i16}", scale)
        return feat, energy, ro


# ---- ragged streaming STFT / mel spectrogram over a pool of stream states ----------------------------------------------------

class _StftStreamPoolBase(_StreamPoolMixin, _StreamBase):
    """A pool of ``pool_streams`` live audio streams, each with the carried state of ``MelSpectrogramStream`` / ``StftStream`` in
    continuous mode.  Called as the frame-path pools are: ``pool(chunks, slots, lengths=None)``, every chunk a whole number of
    hops (zero included).  Per stream the rows and the carried state are those of the dense class on that stream alone.  See
    ``ss_mel_spectrogram_stream_packed`` in ``include/speechsauce_amd.h``.  ``pool(chunks, slots, pcm_scale=2**-15)`` takes int16
    PCM chunks as the frame-path pools do (``ss_mel_spectrogram_stream_packed_i16``): same rows, same state, bit for bit; the state
    stays float32, so a stream may be fed PCM on one call and floats on the next."""


class MelSpectrogramStreamPool(_StftStreamPoolBase):
    """Ragged streaming ``mel_spectrogram``: ``pool(chunks, slots)`` -> ``(out, row_offsets)``.  ``out`` is the flat float32 block
    of ``num_filters * total_rows`` values in the layout of ``mel_spectrogram_packed``: chunk ``i``'s ``[num_filters, R_i]`` block,
    ``R_i = len(chunk) // hop``, is ``out[num_filters * row_offsets[i]:num_filters * row_offsets[i + 1]]`` (``row_offsets``: int64
    numpy array)."""

    _what = "MelSpectrogramStreamPool"

    def __init__(self, pool_streams, sampling_frequency, frame_length=0.020, num_filters=40, fft_length=512, low_frequency=0,
                 high_frequency=None, **switches):
        super().__init__(pool_streams, sampling_frequency, frame_length, 0.01, 13, num_filters, fft_length, low_frequency,
                         high_frequency, True, "continuous", switches)

    def __call__(self, chunks, slots, lengths=None, pcm_scale=None):
        (packed, so, ro, sl, config), i16, scale = self._prepare_pcm(chunks, slots, lengths, pcm_scale)
        n = config.params.num_filters * int(ro[-1])
        if _is_torch(packed):
            import torch

            out = torch.empty((n,), dtype=torch.float32, device=packed.device)
        else:
            out = np.empty((n,), dtype=np.float32)
        self._call_pool(packed, so, ro, sl, config, [out], f"ss_mel_spectrogram_stream_packed{i16}_device",
                        f"ss_mel_spectrogram_stream_packed{i16}", scale)
        return out, ro


class StftStreamPool(_StftStreamPoolBase):
    """Ragged streaming ``stft``: ``pool(chunks, slots)`` -> ``(complex64 [total_rows, fft_length // 2 + 1], row_offsets)``; chunk
    ``i``'s rows are ``row_offsets[i]:row_offsets[i + 1]``."""

    _what = "StftStreamPool"

    def __init__(self, pool_streams, sampling_frequency, frame_length=0.020, fft_length=512, **switches):
        super().__init__(pool_streams, sampling_frequency, frame_length, 0.01, 13, 40, fft_length, 0, None, True, "continuous",
                         switches)

    def __call__(self, chunks, slots, lengths=None, pcm_scale=None):
        (packed, so, ro, sl, config), i16, scale = self._prepare_pcm(chunks, slots, lengths, pcm_scale)
        shape = (int(ro[-1]), config.params.fft_points // 2 + 1, 2)
        dev_fn, host_fn = f"ss_stft_stream_packed{i16}_device", f"ss_stft_stream_packed{i16}"
        if _is_torch(packed):
            import torch

            out = torch.empty(shape, dtype=torch.float32, device=packed.device)
            self._call_pool(packed, so, ro, sl, config, [out], dev_fn, host_fn, scale)
            return torch.view_as_complex(out), ro
        out = np.empty(shape, dtype=np.float32)
        self._call_pool(packed, so, ro, sl, config, [out], dev_fn, host_fn, scale)
        return out.view(np.complex64)[..., 0], ro


# ---- the pools of the side stages (CMVN, add-deltas, splice, VAD, resampling): a block, its offset table and the slots of its entries ------

class _SidePool:
    """The skeleton of ``CmvnStreamPool``, ``AddDeltasStreamPool``, ``SpliceStreamPool``, ``VadEnergyStreamPool`` and
    ``ResampleStreamPool``: the argument rules, the place of the pool and its allocation by the first call, the counter, ``reset``,
    and the two calls ``ss_<_stem>_stream_packed*`` (``_run``) and ``ss_<_stem>_stream_flush*`` (``_flush``) in their host and device
    forms.  A pool class checks its own parameters, sets ``state_len`` and describes its calls: ``_stem``; ``_scalars()``, what stands
    between ``pool_streams`` and the state in ``include/speechsauce_amd.h`` (``_flush_scalars()`` where the flush takes others);
    ``_out_shape(n)`` and ``_flush_shape(n_active)`` of ``_dtype``; ``_period``, what every entry must be a multiple of; ``_counter``,
    the name of its int64 per-slot counter on the host (None: none), which moves by ``_count(np.diff(offsets))``.  What one pool
    does differently from the others (``_table_first``, ``_whole_block``, ``_owner_for``, its own ``reset``) is stated at that pool.

    State, place and counter move only once a call went through ``_lib.check``, in this order and on both paths, also where there
    was nothing to launch: a failed first call leaves the pool unplaced and unallocated."""

    _table, _noun, _verb = "row_offsets", "rows", "takes"
    _stem, _dtype, _period, _counter = "", "float32", 1, "rows_seen"
    _table_first = False  # the slot rule is decided before the values of the offset table
    _whole_block = True  # a call counts every row of the block it is handed, not only those the table covers

    def __init__(self, pool_streams, cols=None):
        if int(pool_streams) < 1:
            raise ValueError(f"{self._what}: pool_streams must be at least 1")
        if cols is not None and int(cols) < 1:
            raise ValueError(f"{self._what}: cols must be at least 1")
        self.pool_streams = int(pool_streams)
        if cols is not None:
            self.cols = int(cols)
        if self._counter:
            setattr(self, self._counter, np.zeros(self.pool_streams, dtype=np.int64))
        self._state = None
        self._where = None

    @property
    def state(self):
        """[pool_streams, state_len] float32: a torch tensor on the device of the first call's block, or a numpy array; None before
        the first call."""
        return self._state

    def reset(self, slots=None):
        """Zero the state (and the counter) of every stream of the pool, or of the given slots (fresh streams)."""
        if slots is None:
            idx = ...
        else:
            idx = self._slots(np.atleast_1d(np.asarray(slots, dtype=np.int64)))
            if not idx:
                return
        getattr(self, self._counter)[idx] = 0
        if self._state is not None:
            self._state[idx] = 0

    def _scalars(self):
        return ()

    def _flush_scalars(self):
        return self._scalars()

    def _count(self, diff):
        return diff

    def _owner_for(self, x):
        """The owner of the handle that leads the calls' arguments, for the place of ``x``: these calls take none."""
        return None

    def __call__(self, rows, row_offsets, slots):
        x = _require_f32(rows, (2,), self._what)
        if int(x.shape[1]) != self.cols:
            raise ValueError(f"{self._what}: rows has {int(x.shape[1])} columns, this pool {self._verb} {self.cols}")
        return self._run(x, row_offsets, slots)

    def _run(self, x, offsets, slots, suffix="", scalars=None):
        """The block ``x`` with its offset table and slots through ``ss_<_stem>_stream_packed<suffix>[_device]``; ``scalars``
        stand in for ``_scalars()``."""
        off = self._offsets(offsets)
        slot_list = [int(v) for v in slots]
        if not self._table_first:
            self._slots(slot_list)
        self._check_offsets(off, len(slot_list), int(x.shape[0]))
        if self._table_first:
            self._slots(slot_list)
        if (np.diff(off) % self._period).any():
            raise ValueError(f"{self._what}: every entry must bring whole periods of {self._period} {self._noun}")
        where = self._place(x)
        lib, n_active = _lib.lib(), len(slot_list)
        owner = self._owner_for(x)
        head = () if owner is None else (owner.handle,)
        sl = np.asarray(slot_list, dtype=np.int32)
        n = int(x.shape[0]) if self._whole_block else int(off[-1])
        name = f"ss_{self._stem}_stream_packed{suffix}"
        scalars = (self.pool_streams, *(self._scalars() if scalars is None else scalars))
        state = self._state_for(x)
        if _is_torch(x):
            import torch

            x = x.contiguous()
            out = torch.empty(self._out_shape(n), dtype=getattr(torch, self._dtype), device=x.device)
            if n_active and n:
                _launch(x.device, getattr(lib, name + "_device"), *head, x, n_active, off, n, sl, *scalars, state.data_ptr(), out.data_ptr())
        else:
            x = np.ascontiguousarray(x)
            out = np.empty(self._out_shape(n), dtype=self._dtype)
            if n_active and n:
                _lib.check(getattr(lib, name)(*head, x.ctypes.data, n_active, off.ctypes.data, sl.ctypes.data, *scalars, state.ctypes.data,
                                              out.ctypes.data))
        self._state, self._where = state, where  # only once the call went through
        if n_active and self._counter:
            getattr(self, self._counter)[sl] += self._count(np.diff(off))
        return out

    def _flush(self, slots):
        """The given slots through ``ss_<_stem>_stream_flush[_device]``, where the pool lives; before the first call there is no
        state anywhere and nothing is called: zeros in a numpy array.  Afterwards the slots' counter is zero."""
        slot_list = self._slots(slots)
        lib, n_active = _lib.lib(), len(slot_list)
        sl = np.asarray(slot_list, dtype=np.int32)
        state, shape = self._state, self._flush_shape(n_active)
        name = f"ss_{self._stem}_stream_flush"
        scalars = (self.pool_streams, *self._flush_scalars())
        owner = self._owner_for(state) if n_active and state is not None else None
        head = () if owner is None else (owner.handle,)
        if not _is_torch(state):
            out = np.zeros(shape, dtype=self._dtype)
            if n_active and state is not None:
                _lib.check(getattr(lib, name)(*head, n_active, sl.ctypes.data, *scalars, state.ctypes.data, out.ctypes.data))
        else:
            import torch

            out = torch.empty(shape, dtype=getattr(torch, self._dtype), device=state.device)
            if n_active:
                _launch(state.device, getattr(lib, name + "_device"), *head, n_active, sl, *scalars, state.data_ptr(), out.data_ptr())
        if n_active:
            getattr(self, self._counter)[sl] = 0
        return out

    def _slots(self, slots):
        return _pool_slots(slots, self.pool_streams, self._what)

    def _offsets(self, offsets):
        """The offset table as a host int64 array (its shape and dtype checked, not yet its values)."""
        off = np.asarray(offsets.cpu() if _is_torch(offsets) else offsets)
        if off.ndim != 1 or off.size < 1:
            raise ValueError(f"{self._what}: {self._table} must be 1-D with one entry more than slots")
        if not np.issubdtype(off.dtype, np.integer):
            raise TypeError(f"{self._what}: {self._table} must be integers, got {off.dtype}")
        return np.ascontiguousarray(off, dtype=np.int64)

    def _check_offsets(self, off, n_slots, total):
        if n_slots != off.size - 1:
            raise ValueError(f"{self._what}: {off.size - 1} entries in {self._table} but {n_slots} slots")
        if off[0] != 0 or (np.diff(off) < 0).any() or off[-1] > total:
            raise ValueError(f"{self._what}: {self._table} must start at 0, not decrease and end within the block's {total} {self._noun}")

    def _place(self, x):
        """Where ``x`` lives; it must be where the pool lives once a call has placed it."""
        where = ("cuda", x.device.index) if _is_torch(x) else ("host",)
        if self._where is not None and where != self._where:
            raise ValueError(f"{self._what}: the pool lives on {self._where}, these {self._noun} on {where}")
        return where

    def _state_for(self, x):
        """The pool's state, or zeros next to ``x`` for the first call (which keeps them only once it went through)."""
        if self._state is not None:
            return self._state
        if _is_torch(x):
            import torch

            return torch.zeros((self.pool_streams, self.state_len), dtype=torch.float32, device=x.device)
        return np.zeros((self.pool_streams, self.state_len), dtype=np.float32)


# ---- causal sliding-window CMVN over a pool of stream states (ss_cmvn_stream_packed*) ---------------------------------------

class CmvnStreamPool(_SidePool):
    """Causal mean (and variance) normalisation of the rows of live streams: every row over the trailing ``win_size`` rows of its
    own stream (the row itself the newest, no padding at a stream's start), with the last ``win_size - 1`` raw rows of each of
    ``pool_streams`` streams carried from call to call.  ``pool(rows, row_offsets, slots)`` takes the ``(rows, row_offsets)`` pair
    a ``MfccStreamPool`` / ``MfeStreamPool`` call returned and the ``slots`` that call was given, and returns the normalised
    ``[total_rows, cols]`` block (rows past ``row_offsets[-1]`` are left uninitialised).  numpy in -> the host-pointer call, ROCm
    tensors in -> the device call on the current stream.  A row's bits depend on its window's values only, however the stream was
    cut into calls.  See ``ss_cmvn_stream_packed`` in ``include/speechsauce_amd.h``."""

    _what, _stem, _verb = "CmvnStreamPool", "cmvn", "normalises"
    _counter = None  # the window needs no dates: no counter, and with nothing delayed no ``flush``
    _table_first = True  # this pool decides the offset table before the slots

    def __init__(self, pool_streams, cols, win_size=301, variance_normalization=False):
        super().__init__(pool_streams, cols)
        if int(win_size) < 1:
            raise ValueError(f"{self._what}: win_size must be at least 1")
        self.win_size = int(win_size)
        self.variance_normalization = bool(variance_normalization)
        L = C.c_size_t()
        _lib.check(_lib.lib().ss_cmvn_stream_state_len(self.cols, self.win_size, C.byref(L)))
        self.state_len = L.value  # (win_size - 1) * cols + 1

    def reset(self, slots=None):
        """Zero the state of every stream of the pool, or of the given slots (fresh streams)."""
        if self._state is None:  # (nothing to zero and no counter: the slots are not even looked at, and never held to the slot rule)
            return
        if slots is None:
            self._state[...] = 0
        else:
            idx = list(np.atleast_1d(np.asarray(slots, dtype=np.int64)))
            if idx:
                self._state[idx] = 0

    def _scalars(self):
        return self.cols, self.win_size, int(self.variance_normalization)

    def _out_shape(self, n):
        return n, self.cols


def stack_frames(signal, sampling_frequency, frame_length=0.020, frame_stride=0.020, filter=None, zero_padding=False, **switches):
    """``speechsauce::processing::stack_frames(signal, sample_rate, frame_length, frame_stride, filter, zero_padding)``
    (processing.rs:65-129): (num_frames, frame_len) frames of a 1-D signal, any sampling rate and frame length (the function
    has no FFT dependency: 44.1 kHz x 25 ms = round(1102.5) = 1103-sample frames are fine).  ``filter``: as in the reference, a callable that
    gets frame_len and returns the window as a (1, frame_len) array (row 0 is used; a 1-D array of frame_len works too), or an
    array; ``zero_padding=True`` is the reference's flag (ceil instead of floor frames, the tail reading appended zeros).
    ``switches`` (``framing="literal" | "center"``, ``mfcc_window=``, ``pad_mode=``) go through a SpeechConfig instead and then
    need frame_len <= 8192."""
    sig = _require_f32(signal, (1,), "stack_frames")
    if isinstance(filter, (bool, np.bool_)):
        # round 3's signature had zero_padding in this position: an old positional call must fail clearly, not index a bool
        raise TypeError("stack_frames: the fifth argument is `filter` (a callable or an array), as in the reference "
                        "(processing.rs:65-76); pass zero_padding=... by keyword or as the sixth argument")
    lib = _lib.lib()
    L = sig.shape[0]
    if switches:
        if filter is not None:
            raise ValueError("stack_frames: pass either filter= or the mfcc_window switch")
        if zero_padding:
            switches = dict(switches, framing="padded")
        flen = int(np.floor(np.float32(np.float32(sampling_frequency) * np.float32(frame_length)) + np.float32(0.5)))  # f32::round
        n_fft = 512
        while n_fft < flen and n_fft < 8192:  # the config needs an FFT length that holds the frame; nothing else uses it here
            n_fft *= 2
        config = _cfg(sampling_frequency, frame_length, frame_stride, 13, 40, n_fft, 0, None, True, switches, sig)
        T = config.num_frames(L)
        fl, st = C.c_size_t(), C.c_size_t()
        _lib.check(lib.ss_frame_sizes(C.byref(config.params), C.byref(fl), C.byref(st)))
        if _is_torch(sig):
            import torch

            x = sig.contiguous()
            out = torch.empty((T, fl.value), dtype=torch.float32, device=x.device)
            with torch.cuda.device(x.device):
                _lib.check(lib.ss_stack_frames_device(config.handle, x.data_ptr(), 1, L, L, out.data_ptr(), _stream_ptr()))
            return out
        x = np.ascontiguousarray(sig)
        out = np.empty((T, fl.value), dtype=np.float32)
        _lib.check(lib.ss_stack_frames(config.handle, x.ctypes.data, L, out.ctypes.data))
        return out
    T, fl = C.c_size_t(), C.c_size_t()
    _lib.check(lib.ss_stack_frames_shape(L, int(sampling_frequency), float(frame_length), float(frame_stride), int(bool(zero_padding)),
                                         C.byref(T), C.byref(fl)))
    win = None
    if filter is not None:
        w = filter(fl.value) if callable(filter) else filter
        w = w.detach().cpu().numpy() if _is_torch(w) else np.asarray(w)
        w = np.ascontiguousarray(w.reshape(-1)[: fl.value] if w.ndim == 1 or w.shape[0] != 1 else w[0], dtype=np.float32)
        if w.shape[0] != fl.value:
            raise ValueError(f"stack_frames: filter gave {w.shape[0]} values for frames of {fl.value} samples")
        win = w
    if _is_torch(sig):
        import torch

        x = sig.contiguous()
        out = torch.empty((T.value, fl.value), dtype=torch.float32, device=x.device)
        _launch(x.device, lib.ss_stack_frames_signal_device, x, L, int(sampling_frequency), float(frame_length), float(frame_stride), win,
                int(bool(zero_padding)), out.data_ptr())
        return out
    x = np.ascontiguousarray(sig)
    out = np.empty((T.value, fl.value), dtype=np.float32)
    _lib.check(lib.ss_stack_frames_signal(x.ctypes.data, L, int(sampling_frequency), float(frame_length), float(frame_stride),
                                          win.ctypes.data if win is not None else None, int(bool(zero_padding)), out.ctypes.data))
    return out


def power_spectrum(frames, fft_points=512):
    """``speechsauce::processing::power_spectrum(frames, fft_points)`` (processing.rs:179-181): |rfft(row)| / fft_points of
    every row of a 2-D float32 frames matrix (rows shorter than fft_points are zero-padded, processing.rs:147-156) ->
    (num_frames, fft_points // 2 + 1).  The name is the reference's; the values are magnitudes, as written there."""
    if _is_torch(frames):
        import torch

        if frames.dtype != torch.float32:
            raise TypeError("power_spectrum: frames must be float32")
        if frames.dim() != 2:
            raise ValueError("power_spectrum: frames must be 2d")
        fr = frames if frames.is_cuda else frames.detach().numpy()
    else:
        fr = np.asarray(frames)
        if fr.dtype != np.float32:
            raise TypeError(f"power_spectrum: frames must be float32, got {fr.dtype}")
        if fr.ndim != 2:
            raise ValueError("power_spectrum: frames must be 2d")
    # only fft_points of the config matters here; the other fields are chosen so that the config validates with it
    # (a frame of half the FFT length, a bank that fits the spectrum)
    n = int(fft_points)
    nf = max(1, min(40, n // 8))
    config = _cfg(16000, n / 32000.0, n / 64000.0, min(13, nf), nf, n, 0, None, True, {}, fr)
    lib = _lib.lib()
    rows, cols = fr.shape
    F = int(fft_points) // 2 + 1
    if _is_torch(fr):
        import torch

        x = fr if fr.stride(1) == 1 else fr.contiguous()
        out = torch.empty((rows, F), dtype=torch.float32, device=x.device)
        with torch.cuda.device(x.device):
            _lib.check(lib.ss_power_spectrum_frames_device(config.handle, x.data_ptr(), rows, cols, x.stride(0) if rows > 1 else cols,
                                                           out.data_ptr(), _stream_ptr()))
        return out
    x = np.ascontiguousarray(fr)
    out = np.empty((rows, F), dtype=np.float32)
    _lib.check(lib.ss_power_spectrum_frames(config.handle, x.ctypes.data, rows, cols, out.ctypes.data))
    return out


def power_spectrum_of_signal(signal, sampling_frequency, frame_length=0.020, frame_stride=0.01, fft_length=512, **switches):
    """stack_frames + power_spectrum fused, as mfe uses them (feature.rs:203-214): 1-D -> (T, F), 2-D [B, L] -> (B, T, F)."""
    sig = _require_f32(signal, (1, 2), "power_spectrum_of_signal")
    config = _cfg(sampling_frequency, frame_length, frame_stride, 13, 40, fft_length, 0, None, True, switches, sig)
    lib = _lib.lib()
    one_d = sig.ndim == 1
    sig2 = sig[None, :] if one_d else sig
    B, L = sig2.shape
    T = config.num_frames(L)
    F = config.params.fft_points // 2 + 1
    if _is_torch(sig2):
        import torch

        x = sig2 if sig2.stride(1) == 1 else sig2.contiguous()
        out = torch.empty((B, T, F), dtype=torch.float32, device=x.device)
        with torch.cuda.device(x.device):
            _lib.check(lib.ss_power_spectrum_batch_device(config.handle, x.data_ptr(), B, L, x.stride(0) if B > 1 else L, out.data_ptr(), _stream_ptr()))
    else:
        x = np.ascontiguousarray(sig2)
        out = np.empty((B, T, F), dtype=np.float32)
        _lib.check(lib.ss_power_spectrum_batch(config.handle, x.ctypes.data, B, L, L, out.ctypes.data))
    return out[0] if one_d else out


def preemphasis(signal, shift=1, cof=0.98):
    """y[n] = x[n] - cof * x[(n - shift) mod N]  (processing.rs:31-53; py lib.rs:207-215)."""
    sig = _require_f32(signal, (1,), "preemphasis")
    lib = _lib.lib()
    n = sig.shape[0]
    if _is_torch(sig):
        import torch

        x = sig.contiguous()
        y = torch.empty_like(x)
        with torch.cuda.device(x.device):
            _lib.check(lib.ss_preemphasis_device(x.data_ptr(), n, int(shift), float(cof), y.data_ptr(), _stream_ptr()))
        return y
    x = np.ascontiguousarray(sig)
    y = np.empty_like(x)
    _lib.check(lib.ss_preemphasis(x.ctypes.data, n, int(shift), float(cof), y.ctypes.data))
    return y


# ---- post-processing on the feature matrix (processing.rs:222-371, feature.rs:253-269; `cmvn` is exported by the
# reference's Python package, py lib.rs:217-224).  numpy [rows, cols] in -> numpy out; a ROCm tensor of shape
# [rows, cols] or [batch, rows, cols] stays on the device (current stream). ----

def _feature_matrix(vec, what):
    if _is_torch(vec):
        import torch

        if vec.dtype != torch.float32:
            raise TypeError(f"{what}: expected float32")
        if vec.dim() not in (2, 3):
            raise ValueError(f"{what}: expected a [rows, cols] or [batch, rows, cols] tensor")
        if not vec.is_cuda:
            return np.ascontiguousarray(vec.numpy()), False
        return vec.contiguous(), True
    arr = np.asarray(vec)
    if arr.dtype != np.float32:
        raise TypeError(f"{what}: expected float32 (the reference binding takes PyReadonlyArray2<f32>)")
    if arr.ndim != 2:
        raise ValueError(f"{what}: expected a 2-D [rows, cols] array")
    return np.ascontiguousarray(arr), False


def _post(vec, what, host_fn, dev_fn, out_tail=()):
    x, on_device = _feature_matrix(vec, what)
    if on_device:
        import torch

        batch = x.shape[0] if x.dim() == 3 else 1
        rows, cols = x.shape[-2], x.shape[-1]
        out = torch.empty(tuple(x.shape) + tuple(out_tail), dtype=torch.float32, device=x.device)
        with torch.cuda.device(x.device):
            _lib.check(dev_fn(x.data_ptr(), batch, rows, cols, out.data_ptr(), _stream_ptr()))
        return out
    if x.ndim == 3:  # CPU tensor with a batch axis: one matrix at a time through the host entry point
        return np.stack([_post(m, what, host_fn, dev_fn, out_tail) for m in x])
    out = np.empty(x.shape + tuple(out_tail), dtype=np.float32)
    _lib.check(host_fn(x.ctypes.data, x.shape[0], x.shape[1], out.ctypes.data))
    return out


def cmvn(vec, variance_normalization=False):
    """Global cepstral mean (and variance) normalisation, one observation per row (processing.rs:265-300)."""
    lib, var = _lib.lib(), int(bool(variance_normalization))
    return _post(vec, "cmvn", lambda p, r, c, o: lib.ss_cmvn(p, r, c, var, o),
                 lambda p, b, r, c, o, s: lib.ss_cmvn_batch_device(p, b, r, c, var, o, s))


def cmvnw(vec, win_size=301, variance_normalization=False):
    """Sliding-window mean (and variance) normalisation over win_size rows (processing.rs:315-371)."""
    lib, var, w = _lib.lib(), int(bool(variance_normalization)), int(win_size)
    return _post(vec, "cmvnw", lambda p, r, c, o: lib.ss_cmvnw(p, r, c, w, var, o),
                 lambda p, b, r, c, o, s: lib.ss_cmvnw_batch_device(p, b, r, c, w, var, o, s))


def derivative_extraction(feat, delta_windows):
    """Derivative features along the feature axis (processing.rs:222-254)."""
    lib, dw = _lib.lib(), int(delta_windows)
    return _post(feat, "derivative_extraction", lambda p, r, c, o: lib.ss_derivative_extraction(p, r, c, dw, o),
                 lambda p, b, r, c, o, s: lib.ss_derivative_extraction_device(p, b * r, c, dw, o, s))


def extract_derivative_feature(feature):
    """[..., rows, cols] -> [..., rows, cols, 3]: static, first and second derivative features (feature.rs:253-269)."""
    lib = _lib.lib()
    return _post(feature, "extract_derivative_feature", lambda p, r, c, o: lib.ss_extract_derivative_feature(p, r, c, o),
                 lambda p, b, r, c, o, s: lib.ss_extract_derivative_feature_device(p, b * r, c, o, s), out_tail=(3,))


# ---- the same steps on packed variable-length clips (ss_*_packed*): `offsets` is the table mfcc_packed / mfe_packed /
# mel_spectrogram_packed returned (n + 1 int64, offsets[0] = 0); clip b owns rows offsets[b] : offsets[b + 1] of the block ----

def _packed_block(S, cols, what):
    """-> (contiguous float32 block, on_device, total_rows, cols); a 2-D block is [total_rows, cols], a flat one needs cols."""
    if _is_torch(S):
        import torch

        if S.dtype != torch.float32:
            raise TypeError(f"{what}: expected float32, got {S.dtype}")
        on_device = S.is_cuda
        x = S.contiguous() if on_device else np.ascontiguousarray(S.detach().numpy())
    else:
        x = np.asarray(S)
        if x.dtype != np.float32:
            raise TypeError(f"{what}: expected float32, got {x.dtype}")
        x, on_device = np.ascontiguousarray(x), False
    ndim = x.dim() if on_device else x.ndim
    if ndim == 2:
        if cols is not None and int(cols) != x.shape[1]:
            raise ValueError(f"{what}: cols = {cols} but the block has {x.shape[1]} columns")
        return x, on_device, int(x.shape[0]), int(x.shape[1])
    if ndim != 1:
        raise ValueError(f"{what}: expected a [total_rows, cols] block (or a flat block and cols)")
    if cols is None:
        raise ValueError(f"{what}: a flat block needs cols")
    cols = int(cols)
    if cols <= 0 or x.shape[0] % cols:
        raise ValueError(f"{what}: the block of {x.shape[0]} values is not a whole number of rows of {cols}")
    return x, on_device, int(x.shape[0]) // cols, cols


def _segment_table(offsets, on_device, device, total_rows, what):
    """-> (table for the call, n_clips): a device int64 tensor is used as it is (the kernels contain a bad table, nothing of it is
    read back); a host table is validated here and, for a device block, uploaded."""
    if _is_torch(offsets):
        import torch

        if offsets.dtype != torch.int64:
            raise TypeError(f"{what}: offsets must be int64, got {offsets.dtype}")
        if offsets.dim() != 1 or offsets.numel() < 1:
            raise ValueError(f"{what}: offsets must be 1-D with n_clips + 1 entries")
        if offsets.is_cuda:
            if not on_device:
                offsets = offsets.cpu()  # host block: the host entry point validates a host table
            elif offsets.device != device:
                raise ValueError(f"{what}: offsets and the block live on different devices")
            else:
                return offsets.contiguous(), offsets.numel() - 1
        offsets = offsets.numpy()
    off = np.asarray(offsets)
    if off.ndim != 1 or off.size < 1:
        raise ValueError(f"{what}: offsets must be 1-D with n_clips + 1 entries")
    if not np.issubdtype(off.dtype, np.integer):
        raise TypeError(f"{what}: offsets must be integers, got {off.dtype}")
    off = np.ascontiguousarray(off, dtype=np.int64)
    if off[0] != 0 or (np.diff(off) < 0).any() or off[-1] > total_rows:
        raise ValueError(f"{what}: offsets must start at 0, not decrease and end within the block's {total_rows} rows")
    if on_device:
        import torch

        return torch.from_numpy(off).to(device), off.size - 1
    return off, off.size - 1


def _post_packed(S, offsets, cols, what, host_fn, dev_fn):
    x, on_device, rows, cols = _packed_block(S, cols, what)
    table, n = _segment_table(offsets, on_device, x.device if on_device else None, rows, what)
    if on_device:
        import torch

        out = torch.empty_like(x)
        with torch.cuda.device(x.device):
            _lib.check(dev_fn(x.data_ptr(), n, table.data_ptr(), rows, cols, out.data_ptr(), _stream_ptr()))
        return out
    out = np.empty_like(x)
    _lib.check(host_fn(x.ctypes.data, n, table.ctypes.data, rows, cols, out.ctypes.data))
    return out


def cmvn_packed(vec, offsets, variance_normalization=False):
    """``cmvn`` of every clip of a packed block [sum T_b, cols] on its own rows, one launch for all clips.  numpy in -> numpy out; a
    ROCm tensor stays on the device (current stream), and ``offsets`` may be the device tensor ``mfcc_packed`` returned (used as it
    is) or a host array (validated, uploaded).  Rows that the table does not cover are left uninitialised."""
    lib, var = _lib.lib(), int(bool(variance_normalization))
    return _post_packed(vec, offsets, None, "cmvn_packed", lambda p, n, t, r, c, o: lib.ss_cmvn_packed(p, n, t, r, c, var, o),
                        lambda p, n, t, r, c, o, s: lib.ss_cmvn_packed_device(p, n, t, r, c, var, o, s))


def cmvnw_packed(vec, offsets, win_size=301, variance_normalization=False):
    """``cmvnw`` of every clip of a packed block on its own rows: the symmetric padding reflects at the clip's own first and last
    row.  See cmvn_packed."""
    lib, var, w = _lib.lib(), int(bool(variance_normalization)), int(win_size)
    return _post_packed(vec, offsets, None, "cmvnw_packed", lambda p, n, t, r, c, o: lib.ss_cmvnw_packed(p, n, t, r, c, w, var, o),
                        lambda p, n, t, r, c, o, s: lib.ss_cmvnw_packed_device(p, n, t, r, c, w, var, o, s))


def _group_table(groups, n, on_device, device, what):
    """-> the int32 table of a grouped-CMVN call on the block's side (None stays None: every clip in group 0)"""
    if groups is None:
        return None
    if _is_torch(groups):
        import torch

        if groups.dtype != torch.int32:
            raise TypeError(f"{what}: groups must be int32, got {groups.dtype}")
        if groups.dim() != 1 or groups.numel() != n:
            raise ValueError(f"{what}: groups must be 1-D with n_clips = {n} entries")
        if on_device:
            return groups.to(device).contiguous()
        groups = groups.cpu().numpy()
    g = np.asarray(groups)
    if g.ndim != 1 or g.size != n:
        raise ValueError(f"{what}: groups must be 1-D with n_clips = {n} entries")
    if not np.issubdtype(g.dtype, np.integer):
        raise TypeError(f"{what}: groups must be integers, got {g.dtype}")
    g = np.ascontiguousarray(g, dtype=np.int32)
    if on_device:
        import torch

        return torch.from_numpy(g).to(device)
    return g


def _stats_block(stats, n_groups, cols, on_device, device, what, fresh):
    """-> the float64 [n_groups, 2 * cols + 1] block on the block's side; None gives a zeroed one where `fresh` allows it"""
    shape = (int(n_groups), 2 * cols + 1)
    if stats is None:
        if not fresh:
            raise ValueError(f"{what}: stats is required")
        if on_device:
            import torch

            return torch.zeros(shape, dtype=torch.float64, device=device)
        return np.zeros(shape, np.float64)
    if _is_torch(stats):
        import torch

        if stats.dtype != torch.float64:
            raise TypeError(f"{what}: stats must be float64, got {stats.dtype}")
        st = stats.to(device) if on_device else stats.detach().cpu().numpy()
    else:
        st = np.asarray(stats)
        if st.dtype != np.float64:
            raise TypeError(f"{what}: stats must be float64, got {st.dtype}")
        if on_device:
            import torch

            st = torch.from_numpy(np.ascontiguousarray(st)).to(device)
    if tuple(st.shape) == shape[1:]:
        st = st.reshape(shape) if shape[0] == 1 else st
    if tuple(st.shape) != shape:
        raise ValueError(f"{what}: stats must be [n_groups, 2 * cols + 1] = {list(shape)}, got {list(st.shape)}")
    return st.contiguous() if on_device else np.ascontiguousarray(st)


def _ptr(a):
    return None if a is None else a.data_ptr() if _is_torch(a) else a.ctypes.data


def cmvn_stats_packed(vec, offsets, groups, n_groups, stats=None):
    """Fold every clip of a packed block [sum T_b, cols] into the statistics row of its group: ``stats`` is the float64 block
    [n_groups, 2 * cols + 1] of rows ``[n | mean | var]`` (None: a fresh, zeroed one) and the updated block is returned -- a device
    tensor or a writable numpy array handed in is updated in place and returned itself.  ``groups`` is an int32 table with one group
    id per clip (-1 leaves a clip out; None puts every clip into group 0).  Statistics can be accumulated batch by batch, stored,
    and applied with ``cmvn_apply_packed``: per-speaker CMVN with one group per speaker, global CMVN with n_groups = 1."""
    what = "cmvn_stats_packed"
    x, on_device, rows, cols = _packed_block(vec, None, what)
    dev = x.device if on_device else None
    table, n = _segment_table(offsets, on_device, dev, rows, what)
    g = _group_table(groups, n, on_device, dev, what)
    st = _stats_block(stats, n_groups, cols, on_device, dev, what, True)
    lib = _lib.lib()
    if on_device:
        import torch

        with torch.cuda.device(dev):
            _lib.check(lib.ss_cmvn_stats_packed_device(x.data_ptr(), n, table.data_ptr(), rows, cols, _ptr(g), int(n_groups), st.data_ptr(),
                                                       _stream_ptr()))
        return st
    if not st.flags.writeable:
        st = st.copy()
    _lib.check(lib.ss_cmvn_stats_packed(x.ctypes.data, n, table.ctypes.data, rows, cols, _ptr(g), int(n_groups), st.ctypes.data))
    return st


def cmvn_apply_packed(vec, offsets, stats, groups=None, variance_normalization=False, out=None):
    """Normalise every clip of a packed block by the stored statistics of its group: ``(x - mean_g) / (sqrt(var_g) + 2^-30)``, or
    ``x - mean_g`` without variance normalisation.  ``stats`` is the block ``cmvn_stats_packed`` returns (or one row, for
    ``groups=None``: global CMVN); ``out`` may be the block itself (in place).  Clips with group id -1, or whose group has seen no
    row, are left as ``out`` held them (uninitialised for a fresh ``out``).  A pool tick's rows with its ``row_offsets`` are a
    packed block too: this is the online global CMVN of a stream pool."""
    what = "cmvn_apply_packed"
    x, on_device, rows, cols = _packed_block(vec, None, what)
    dev = x.device if on_device else None
    table, n = _segment_table(offsets, on_device, dev, rows, what)
    g = _group_table(groups, n, on_device, dev, what)
    n_groups = int(stats.shape[0]) if getattr(stats, "ndim", 0) == 2 else 1
    st = _stats_block(stats, n_groups, cols, on_device, dev, what, False)
    var, lib = int(bool(variance_normalization)), _lib.lib()
    if on_device:
        import torch

        if out is None:
            out = torch.empty_like(x)
        elif not (_is_torch(out) and out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.shape == x.shape):
            raise ValueError(f"{what}: out must be a contiguous float32 device tensor of the block's shape")
        with torch.cuda.device(dev):
            _lib.check(lib.ss_cmvn_apply_packed_device(x.data_ptr(), n, table.data_ptr(), rows, cols, _ptr(g), n_groups, st.data_ptr(), var,
                                                       out.data_ptr(), _stream_ptr()))
        return out
    if out is None:
        out = np.empty_like(x)
    elif not (isinstance(out, np.ndarray) and out.dtype == np.float32 and out.flags.c_contiguous and out.shape == x.shape):
        raise ValueError(f"{what}: out must be a contiguous float32 array of the block's shape")
    _lib.check(lib.ss_cmvn_apply_packed(x.ctypes.data, n, table.ctypes.data, rows, cols, _ptr(g), n_groups, st.ctypes.data, var, out.ctypes.data))
    return out


def cmvn_grouped_packed(vec, offsets, groups, n_groups=None, variance_normalization=False):
    """Per-speaker CMVN of one batch: statistics of every group from the batch's own clips, then ``cmvn_apply_packed``, in one call.
    ``n_groups`` defaults to max(groups) + 1 for a host table (a device table needs it stated: nothing is read back)."""
    what = "cmvn_grouped_packed"
    x, on_device, rows, cols = _packed_block(vec, None, what)
    dev = x.device if on_device else None
    table, n = _segment_table(offsets, on_device, dev, rows, what)
    if n_groups is None:
        if groups is None:
            n_groups = 1
        elif _is_torch(groups) and groups.is_cuda:
            raise ValueError(f"{what}: a device table of groups needs n_groups")
        else:
            n_groups = max(1, int(np.asarray(groups.cpu() if _is_torch(groups) else groups).max(initial=-1)) + 1)
    g = _group_table(groups, n, on_device, dev, what)
    var, lib = int(bool(variance_normalization)), _lib.lib()
    if on_device:
        import torch

        out = torch.empty_like(x)
        with torch.cuda.device(dev):
            _lib.check(lib.ss_cmvn_grouped_packed_device(x.data_ptr(), n, table.data_ptr(), rows, cols, _ptr(g), int(n_groups), var, out.data_ptr(),
                                                         _stream_ptr()))
        return out
    out = np.empty_like(x)
    _lib.check(lib.ss_cmvn_grouped_packed(x.ctypes.data, n, table.ctypes.data, rows, cols, _ptr(g), int(n_groups), var, out.ctypes.data))
    return out


def _kaldi_convert(a, what, fn, in_len, out_len):
    a = np.ascontiguousarray(np.asarray(a.detach().cpu().numpy() if _is_torch(a) else a), dtype=np.float64)
    cols = in_len(a.size)
    if cols is None or cols < 1:
        raise ValueError(f"{what}: not a statistics row or a Kaldi accumulator ({a.size} values)")
    out = np.empty(out_len(cols), np.float64)
    _lib.check(fn(a.ctypes.data, cols, out.ctypes.data))
    return out


def cmvn_stats_to_kaldi(stats_row):
    """One statistics row ``[n | mean | var]`` -> Kaldi's float64 accumulator [2, cols + 1]: ``sum x | count``, then ``sum x^2 | 0``
    (cmvn.ark; WeNet's mean_stat / var_stat / frame_num)."""
    lib = _lib.lib()
    out = _kaldi_convert(stats_row, "cmvn_stats_to_kaldi", lib.ss_cmvn_stats_to_kaldi,
                         lambda k: (k - 1) // 2 if k % 2 == 1 else None, lambda c: 2 * (c + 1))
    return out.reshape(2, -1)


def cmvn_stats_from_kaldi(kaldi):
    """Kaldi's accumulator [2, cols + 1] -> one statistics row ``[n | mean | var]``; a count below 1 gives a fresh (all-zero) row."""
    lib = _lib.lib()
    return _kaldi_convert(kaldi, "cmvn_stats_from_kaldi", lib.ss_cmvn_stats_from_kaldi,
                          lambda k: k // 2 - 1 if k % 2 == 0 else None, lambda c: 2 * c + 1)


def power_to_db_packed(S, offsets, cols=None, ref=1.0, amin=1e-10, top_db=80.0):
    """``power_to_db`` of every clip of a packed block with the clip's own ``top_db`` floor.  Clip b's segment is elements
    cols * offsets[b] : cols * offsets[b + 1]: a [sum T_b, cols] block (cols defaults to its width), or the flat block of
    ``mel_spectrogram_packed`` with cols = num_filters and its row offsets.  See cmvn_packed."""
    lib = _lib.lib()
    if top_db is not None and top_db < 0:
        raise ValueError("top_db must be non-negative")
    td, rf, am = -1.0 if top_db is None else float(top_db), float(ref), float(amin)
    return _post_packed(S, offsets, cols, "power_to_db_packed",
                        lambda p, n, t, r, c, o: lib.ss_power_to_db_packed(p, n, t, r, c, rf, am, td, o),
                        lambda p, n, t, r, c, o, s: lib.ss_power_to_db_packed_device(p, n, t, r, c, rf, am, td, o, s))


# ---- time-axis delta features (Kaldi's add-deltas; ss_add_deltas_*) -----------------------------------------------------------
# derivative_extraction / extract_derivative_feature above are the reference's, along the FEATURE axis; these append the regression
# deltas over neighbouring FRAMES: out row = [x[t] | d1[t] | d2[t]], (order + 1) * cols floats.

def _check_delta_params(order, window, what):
    order, window = int(order), int(window)
    if order not in (1, 2):
        raise ValueError(f"{what}: order must be 1 or 2")
    if window < 1:
        raise ValueError(f"{what}: window must be at least 1")
    if order * window > 32:
        raise ValueError(f"{what}: order * window must be at most 32")
    return order, window


def add_deltas_packed(vec, offsets, order=2, window=2):
    """Kaldi ``add-deltas`` of every clip of a packed block [sum T_b, cols] on its own rows (edge replication at the clip's own first
    and last row), one launch for all clips: -> [sum T_b, (order + 1) * cols], row t = [x[t] | delta | delta-delta].  Order 1 equals
    HTK, ``python_speech_features.delta`` and ``torchaudio.functional.compute_deltas(mode="replicate")``; the second delta is the
    composite filter on the raw rows.  numpy in -> the host-pointer call; a ROCm tensor stays on the device (current stream), and
    ``offsets`` may be the device tensor ``mfcc_packed`` returned or a host array, as for ``cmvn_packed``.  Rows that the table does
    not cover are left uninitialised.  See ``ss_add_deltas_packed`` in ``include/speechsauce_amd.h``."""
    what = "add_deltas_packed"
    order, window = _check_delta_params(order, window, what)
    lib = _lib.lib()
    x, on_device, rows, cols = _packed_block(vec, None, what)
    table, n = _segment_table(offsets, on_device, x.device if on_device else None, rows, what)
    if on_device:
        import torch

        out = torch.empty((rows, (order + 1) * cols), dtype=torch.float32, device=x.device)
        _launch(x.device, lib.ss_add_deltas_packed_device, x, n, table, rows, cols, order, window, out.data_ptr())
        return out
    out = np.empty((rows, (order + 1) * cols), dtype=np.float32)
    _lib.check(lib.ss_add_deltas_packed(x.ctypes.data, n, table.ctypes.data, rows, cols, order, window, out.ctypes.data))
    return out


def add_deltas(feat, order=2, window=2):
    """``add_deltas_packed`` of one matrix [T, cols] -> [T, (order + 1) * cols], or of every matrix of a batch [..., T, cols] on its
    own rows (equal-length clips of one packed block, one launch)."""
    x = _require_f32(feat, tuple(range(2, 9)), "add_deltas")
    shape = tuple(int(v) for v in x.shape)
    T, cols = shape[-2], shape[-1]
    n = int(np.prod(shape[:-2], dtype=np.int64))
    offsets = np.arange(n + 1, dtype=np.int64) * T
    out = add_deltas_packed(x.reshape(n * T, cols), offsets, order, window)
    return out.reshape(shape[:-1] + ((int(order) + 1) * cols,))


class AddDeltasStreamPool(_SidePool):
    """Kaldi ``add-deltas`` over the rows of live streams, with a fixed latency of ``lag = order * window`` rows: deltas need ``lag``
    rows of look-ahead, so output row k of an entry is the feature row of stream time ``rows_seen + k - lag`` (all zeros while that is
    negative: the first ``lag`` rows after a reset are warm-up rows).  ``pool(rows, row_offsets, slots)`` takes the ``(rows,
    row_offsets)`` pair of a ``MfccStreamPool`` / ``CmvnStreamPool`` call and the ``slots`` that call was given and returns
    ``[total_rows, (order + 1) * cols]``: an entry gets exactly as many rows as it brought.  ``flush(slots)`` returns the last ``lag``
    rows of those streams, ``[len(slots) * lag, (order + 1) * cols]``, and makes them fresh.  However a stream is cut into calls, its
    rows plus the flush, the first ``lag`` dropped, are bit for bit ``add_deltas`` of the whole clip.  ``rows_seen`` (int64 per slot,
    on the host) dates every row; it moves only after a call went through.  numpy in -> the host-pointer calls, ROCm tensors in ->
    the device calls on the current stream.  See ``ss_add_deltas_stream_packed`` in ``include/speechsauce_amd.h``."""

    _what, _stem = "AddDeltasStreamPool", "add_deltas"

    def __init__(self, pool_streams, cols, order=2, window=2):
        super().__init__(pool_streams, cols)
        self.order, self.window = _check_delta_params(order, window, self._what)
        self.lag = self.order * self.window
        self.out_cols = (self.order + 1) * self.cols
        L = C.c_size_t()
        _lib.check(_lib.lib().ss_add_deltas_stream_state_len(self.cols, self.order, self.window, C.byref(L)))
        self.state_len = L.value  # 2 * lag * cols + 1

    def _scalars(self):
        return self.cols, self.order, self.window

    def _out_shape(self, n):
        return n, self.out_cols

    def _flush_shape(self, n_active):
        return n_active * self.lag, self.out_cols

    def flush(self, slots):
        """The last ``lag`` rows of the given streams, ``[len(slots) * lag, (order + 1) * cols]`` (entry i: rows i * lag .. (i + 1) *
        lag, stream times rows_seen - lag .. rows_seen - 1, zeros where that is negative); afterwards those streams are fresh.  Before
        the pool's first call there is no state anywhere: the rows are zeros in a numpy array."""
        return self._flush(slots)


# ---- frame splicing and subsampling (Kaldi's splice-feats / subsample-feats, low frame rate; ss_splice_*) ----------------------
# out row k = [x[k * stride - left] | .. | x[k * stride] | .. | x[k * stride + right]], indices clamped to the clip's own rows:
# (left + 1 + right) * cols floats, every one a bit copy; ceil(T / stride) rows.

def _check_splice_params(left, right, stride, what):
    left, right, stride = int(left), int(right), int(stride)
    if not 0 <= left <= 32 or not 0 <= right <= 32:
        raise ValueError(f"{what}: left and right must be in 0 .. 32")
    if not 1 <= stride <= 32:
        raise ValueError(f"{what}: stride must be in 1 .. 32")
    return left, right, stride


def _lfr_params(m, n, what):
    m = int(m)
    if m < 1:
        raise ValueError(f"{what}: m must be at least 1")
    return (m - 1) // 2, m - 1 - (m - 1) // 2, n


def splice_packed(rows, row_offsets, left, right, stride=1):
    """Context splicing and frame subsampling of every clip of a packed block [sum T_b, cols] on its own rows, one launch for all
    clips: -> (out [sum ceil(T_b / stride), (left + 1 + right) * cols], out_offsets).  Output row k of a clip is its rows ``k *
    stride - left .. k * stride + right`` side by side, the index clamped to the clip's first and last row; every float is a bit
    copy.  ``stride = 1`` is Kaldi's ``splice-feats``, ``left = right = 0`` its ``subsample-feats``.  numpy in -> the host-pointer
    call and a numpy ``out_offsets``; a ROCm tensor stays on the device (current stream) and ``out_offsets`` is a device tensor.
    ``row_offsets`` may be the device tensor ``mfcc_packed`` returned (it is read back: the output's size depends on it) or a host
    array.  See ``ss_splice_packed`` in ``include/speechsauce_amd.h``."""
    what = "splice_packed"
    left, right, stride = _check_splice_params(left, right, stride, what)
    lib = _lib.lib()
    x, on_device, total_rows, cols = _packed_block(rows, None, what)
    ro, n = _segment_table(row_offsets, False, None, total_rows, what)  # on the host, validated
    oo = np.empty_like(ro)
    _lib.check(lib.ss_splice_packed_offsets(n, ro.ctypes.data, stride, oo.ctypes.data))
    out_rows, ocols = int(oo[-1]), (left + 1 + right) * cols
    if on_device:
        import torch

        out = torch.empty((out_rows, ocols), dtype=torch.float32, device=x.device)
        _, d_oo = _launch(x.device, lib.ss_splice_packed_device, x, n, ro, total_rows, oo, out_rows, cols, left, right, stride, out.data_ptr())
        return out, d_oo
    out = np.empty((out_rows, ocols), dtype=np.float32)
    _lib.check(lib.ss_splice_packed(x.ctypes.data, n, ro.ctypes.data, total_rows, cols, left, right, stride, out.ctypes.data))
    return out, oo


def splice(x, left, right, stride=1):
    """``splice_packed`` of one matrix [T, cols] -> [ceil(T / stride), (left + 1 + right) * cols], or of every matrix of a batch
    [..., T, cols] on its own rows (equal-length clips of one packed block, one launch)."""
    x = _require_f32(x, tuple(range(2, 9)), "splice")
    shape = tuple(int(v) for v in x.shape)
    T, cols = shape[-2], shape[-1]
    n = int(np.prod(shape[:-2], dtype=np.int64))
    out, _ = splice_packed(x.reshape(n * T, cols), np.arange(n + 1, dtype=np.int64) * T, left, right, stride)
    return out.reshape(shape[:-2] + (-(-T // int(stride)), out.shape[1]))


def lfr_packed(rows, row_offsets, m, n):
    """Low frame rate on packed clips: stack ``m`` frames, skip ``n`` (FunASR's ``apply_lfr(m, n)``) = ``splice_packed`` with ``left =
    (m - 1) // 2, right = m - 1 - left, stride = n``."""
    return splice_packed(rows, row_offsets, *_lfr_params(m, n, "lfr_packed"))


def lfr(x, m, n):
    """Low frame rate of one matrix or a batch: ``splice`` with ``left = (m - 1) // 2, right = m - 1 - left, stride = n``."""
    return splice(x, *_lfr_params(m, n, "lfr"))


# ---- fused splice + affine transform (Kaldi's splice-feats | transform-feats; ss_affine_* / ss_affine_splice_packed*) ---------
# out row k = M @ (the spliced row k) + bias, one serial f32 fmaf chain per element; the spliced block is never written.

class Affine(_Handle):
    """Owns an ``ss_affine`` handle: a matrix ``[out_dim, in_dim]`` (1 <= out_dim <= 256, 1 <= in_dim <= 4096) and an optional bias
    ``[out_dim]``, re-laid into the kernel's operand order at creation and -- after the first device call -- its device copy.  The
    arrays handed in are not kept."""

    _destroy = "ss_affine_destroy"

    def __init__(self, matrix, bias=None):
        m = np.ascontiguousarray(_affine_host(matrix, "Affine: matrix"), dtype=np.float32)
        if m.ndim != 2:
            raise ValueError("Affine: the matrix must be [out_dim, in_dim]")
        b = None
        if bias is not None:
            b = np.ascontiguousarray(_affine_host(bias, "Affine: bias"), dtype=np.float32)
            if b.shape != (m.shape[0],):
                raise ValueError(f"Affine: the bias must have out_dim = {m.shape[0]} entries")
        super().__init__()
        _lib.check(self._owner.ss_affine_create(m.ctypes.data, m.shape[0], m.shape[1], m.shape[1], b.ctypes.data if b is not None else None,
                                                C.byref(self._h)))
        self.out_dim, self.in_dim = int(m.shape[0]), int(m.shape[1])

    @classmethod
    def from_kaldi(cls, mat, in_dim=None):
        """A Kaldi transform matrix as ``transform-feats`` reads it.  ``in_dim`` is the length of the rows it will meet (the spliced
        row): a matrix of ``in_dim`` columns is linear, one of ``in_dim + 1`` columns carries the offset in its LAST column (Kaldi's
        affine convention).  Without ``in_dim`` the matrix is taken as linear."""
        m = np.asarray(_affine_host(mat, "Affine.from_kaldi"), dtype=np.float32)
        if m.ndim != 2:
            raise ValueError("Affine.from_kaldi: the matrix must be 2-D")
        k = m.shape[1] if in_dim is None else int(in_dim)
        if m.shape[1] == k:
            return cls(m)
        if m.shape[1] == k + 1:
            return cls(m[:, :k], m[:, k])
        raise ValueError(f"Affine.from_kaldi: the matrix has {m.shape[1]} columns, rows of {k} take {k} (linear) or {k + 1} (affine)")

    @property
    def chain_len(self) -> int:
        """K4 = 4 * ceil(in_dim / 4): the steps of every output element's fmaf chain."""
        k4 = C.c_size_t()
        _lib.check(self._owner.ss_affine_chain_len(self.in_dim, C.byref(k4)))
        return int(k4.value)


def _affine_host(a, what):
    if _is_torch(a):
        a = a.detach().cpu().numpy()
    a = np.asarray(a)
    if a.dtype != np.float32:
        raise TypeError(f"{what}: expected float32, got {a.dtype}")
    return a


def splice_affine_packed(rows, row_offsets, transform: Affine, left, right, stride=1):
    """``splice_packed`` followed by ``transform`` (an ``Affine`` of ``in_dim = (left + 1 + right) * cols``) in one launch, the
    spliced block never written: -> (out [sum ceil(T_b / stride), out_dim], out_offsets).  Element i of an output row is the serial
    f32 chain ``acc = bias[i]; acc = fmaf(M[i][k], s[k], acc)`` over the spliced row s, k ascending (``ss_affine_splice_packed`` in
    ``include/speechsauce_amd.h``).  numpy in -> the host-pointer call; a ROCm tensor stays on the device (current stream).
    ``row_offsets`` as for ``splice_packed``."""
    what = "splice_affine_packed"
    if not isinstance(transform, Affine):
        raise TypeError(f"{what}: transform must be an Affine")
    left, right, stride = _check_splice_params(left, right, stride, what)
    lib = _lib.lib()
    x, on_device, total_rows, cols = _packed_block(rows, None, what)
    if (left + 1 + right) * cols != transform.in_dim:
        raise ValueError(f"{what}: the transform takes {transform.in_dim} inputs, a spliced row has {(left + 1 + right) * cols}")
    ro, n = _segment_table(row_offsets, False, None, total_rows, what)  # on the host, validated
    oo = np.empty_like(ro)
    _lib.check(lib.ss_splice_packed_offsets(n, ro.ctypes.data, stride, oo.ctypes.data))
    out_rows = int(oo[-1])
    if on_device:
        import torch

        out = torch.empty((out_rows, transform.out_dim), dtype=torch.float32, device=x.device)
        _, d_oo = _launch(x.device, lib.ss_affine_splice_packed_device, transform.handle, x, n, ro, total_rows, oo, out_rows, cols, left, right, stride,
                          out.data_ptr())
        return out, d_oo
    out = np.empty((out_rows, transform.out_dim), dtype=np.float32)
    _lib.check(lib.ss_affine_splice_packed(transform.handle, x.ctypes.data, n, ro.ctypes.data, total_rows, cols, left, right, stride, out.ctypes.data))
    return out, oo


def splice_affine(x, transform: Affine, left, right, stride=1):
    """``splice_affine_packed`` of one matrix [T, cols] -> [ceil(T / stride), out_dim], or of every matrix of a batch [..., T, cols]
    on its own rows (equal-length clips of one packed block, one launch)."""
    x = _require_f32(x, tuple(range(2, 9)), "splice_affine")
    shape = tuple(int(v) for v in x.shape)
    T, cols = shape[-2], shape[-1]
    n = int(np.prod(shape[:-2], dtype=np.int64))
    out, _ = splice_affine_packed(x.reshape(n * T, cols), np.arange(n + 1, dtype=np.int64) * T, transform, left, right, stride)
    return out.reshape(shape[:-2] + (-(-T // int(stride)), out.shape[1]))


def transform_feats_packed(rows, row_offsets, transform: Affine):
    """Kaldi's ``transform-feats`` on packed rows: ``splice_affine_packed`` without context (``left = right = 0, stride = 1``), e.g.
    behind ``SpliceStreamPool`` on a tick's rows.  -> out [total_rows, out_dim]."""
    return splice_affine_packed(rows, row_offsets, transform, 0, 0, 1)[0]


class SpliceStreamPool(_SidePool):
    """``splice`` over the rows of live streams.  A stream is fed whole periods of ``stride`` rows and gets one output row per period,
    ``delay_rows = right // stride`` periods late (all zeros while the output index is negative: the first ``delay_rows`` rows after
    a reset are warm-up rows); it carries ``delay_rows * stride + left`` raw rows.  ``pool(rows, row_offsets, slots)`` takes the
    ``(rows, row_offsets)`` pair of a feature / ``CmvnStreamPool`` / ``AddDeltasStreamPool`` call and the ``slots`` that call was
    given and returns ``[total_rows // stride, (left + 1 + right) * cols]``: entry i's rows are ``row_offsets[i] // stride ..
    row_offsets[i + 1] // stride``.  ``flush(slots)`` returns the last ``delay_rows`` rows of those streams, ``[len(slots) *
    delay_rows, out_cols]``, and makes them fresh.  However a stream is cut into calls, its rows plus the flush, the first
    ``delay_rows`` dropped, are bit for bit ``splice`` of the whole clip; a stream whose length is not a whole number of periods
    repeats its last row up to one before its last call.  ``rows_seen`` (int64 per slot, on the host) moves only after a call went
    through.  numpy in -> the host-pointer calls, ROCm tensors in -> the device calls on the current stream.  See
    ``ss_splice_stream_packed`` in ``include/speechsauce_amd.h``."""

    _what, _stem = "SpliceStreamPool", "splice"

    def __init__(self, pool_streams, cols, left, right, stride=1):
        super().__init__(pool_streams, cols)
        self.left, self.right, self.stride = _check_splice_params(left, right, stride, self._what)
        self.out_cols = (self.left + 1 + self.right) * self.cols
        L, D = C.c_size_t(), C.c_size_t()
        _lib.check(_lib.lib().ss_splice_stream_state_len(self.cols, self.left, self.right, self.stride, C.byref(L), C.byref(D)))
        self.state_len, self.delay_rows = L.value, D.value  # (delay_rows * stride + left) * cols + 1

    @property
    def _period(self):  # an entry brings whole periods of ``stride`` rows (``rows_seen`` still counts rows)
        return self.stride

    def _scalars(self):
        return self.cols, self.left, self.right, self.stride

    def _out_shape(self, n):
        return n // self.stride, self.out_cols

    def _flush_shape(self, n_active):
        return n_active * self.delay_rows, self.out_cols

    def flush(self, slots):
        """The last ``delay_rows`` rows of the given streams, ``[len(slots) * delay_rows, out_cols]`` (entry i: rows i * delay_rows ..
        (i + 1) * delay_rows; zeros where the output index is negative); afterwards those streams are fresh.  Before the pool's first
        call there is no state anywhere: the rows are zeros in a numpy array."""
        return self._flush(slots)


# ---- energy voice-activity decision and voiced-row selection (Kaldi's compute-vad-energy / select-voiced-frames; ss_vad_* /
# ss_select_rows_*) ---------------------------------------------------------------------------------------------------------------
# mask[t] = (voiced rows among t - L .. t + L inside the clip) >= (rows among them inside the clip) * proportion_threshold, a row
# being voiced where its energy is above energy_threshold + energy_mean_scale * (the clip's mean energy).

def _check_vad_params(energy_col, cols, energy_threshold, energy_mean_scale, frames_context, proportion_threshold, what):
    energy_col, L = int(energy_col), int(frames_context)
    thr, scale, prop = float(energy_threshold), float(energy_mean_scale), float(proportion_threshold)
    if cols is not None and not 0 <= energy_col < cols:
        raise ValueError(f"{what}: energy_col must be in 0 .. {cols - 1}")
    if energy_col < 0:
        raise ValueError(f"{what}: energy_col must not be negative")
    if not 0 <= L <= 32:
        raise ValueError(f"{what}: frames_context must be in 0 .. 32")
    if not (np.isfinite(np.float32(thr)) and np.isfinite(np.float32(scale))):
        raise ValueError(f"{what}: energy_threshold and energy_mean_scale must be finite")
    if not 0.0 < float(np.float32(prop)) < 1.0:
        raise ValueError(f"{what}: proportion_threshold must lie strictly between 0 and 1")
    return energy_col, thr, scale, L, prop


def vad_energy_packed(vec, offsets, energy_col=0, energy_threshold=5.0, energy_mean_scale=0.5, frames_context=0, proportion_threshold=0.6):
    """Kaldi ``compute-vad-energy`` of every clip of a packed block [sum T_b, cols] on its own rows, one launch for all clips: ->
    (mask uint8 [sum T_b], counts int64 [n_clips]).  Row t of a clip is voiced where, among its rows ``t - frames_context .. t +
    frames_context``, at least ``proportion_threshold`` of them have an energy (column ``energy_col``) above ``energy_threshold +
    energy_mean_scale * mean energy of the clip``; ``counts`` are the voiced rows per clip.  The defaults are Kaldi's; the x-vector
    recipes use 5.5 / 0.5 / 2 / 0.12.  numpy in -> the host-pointer call; a ROCm tensor stays on the device (current stream), and
    ``offsets`` may be a device tensor or a host array, as for ``cmvn_packed``.  Bytes of rows that the table does not cover are left
    uninitialised.  See ``ss_vad_energy_packed`` in ``include/speechsauce_amd.h``."""
    what = "vad_energy_packed"
    lib = _lib.lib()
    x, on_device, rows, cols = _packed_block(vec, None, what)
    if cols < 1:
        raise ValueError(f"{what}: the block has no columns")
    scalars = _check_vad_params(energy_col, cols, energy_threshold, energy_mean_scale, frames_context, proportion_threshold, what)
    table, n = _segment_table(offsets, on_device, x.device if on_device else None, rows, what)
    if rows == 0:  # no clip has a row: nothing for the device to do
        if on_device:
            import torch

            return torch.empty(0, dtype=torch.uint8, device=x.device), torch.zeros(n, dtype=torch.int64, device=x.device)
        return np.empty(0, dtype=np.uint8), np.zeros(n, dtype=np.int64)
    if on_device:
        import torch

        mask = torch.empty(rows, dtype=torch.uint8, device=x.device)
        counts = torch.empty(n, dtype=torch.int64, device=x.device)
        _launch(x.device, lib.ss_vad_energy_packed_device, x, n, table, rows, cols, *scalars, mask.data_ptr(), counts.data_ptr())
        return mask, counts
    mask, counts = np.empty(rows, dtype=np.uint8), np.empty(n, dtype=np.int64)
    _lib.check(lib.ss_vad_energy_packed(x.ctypes.data, n, table.ctypes.data, rows, cols, *scalars, mask.ctypes.data, counts.ctypes.data))
    return mask, counts


def vad_energy(feat, energy_col=0, energy_threshold=5.0, energy_mean_scale=0.5, frames_context=0, proportion_threshold=0.6):
    """``vad_energy_packed`` of one matrix [T, cols] -> bool [T], or of every matrix of a batch [..., T, cols] on its own rows -> bool
    [..., T] (equal-length clips of one packed block, one launch)."""
    x = _require_f32(feat, tuple(range(2, 9)), "vad_energy")
    shape = tuple(int(v) for v in x.shape)
    T, cols = shape[-2], shape[-1]
    n = int(np.prod(shape[:-2], dtype=np.int64))
    mask, _ = vad_energy_packed(x.reshape(n * T, cols), np.arange(n + 1, dtype=np.int64) * T, energy_col, energy_threshold, energy_mean_scale,
                                frames_context, proportion_threshold)
    if _is_torch(mask):
        return mask.bool().reshape(shape[:-1])
    return mask.astype(bool).reshape(shape[:-1])


def _row_mask(mask, on_device, device, total_rows, what):
    """The byte mask of a selection next to its block: uint8 or bool, one entry per row."""
    if _is_torch(mask):
        import torch

        if mask.dtype not in (torch.uint8, torch.bool):
            raise TypeError(f"{what}: mask must be uint8 or bool, got {mask.dtype}")
        if mask.dim() != 1 or int(mask.numel()) != total_rows:
            raise ValueError(f"{what}: mask must have one entry for each of the block's {total_rows} rows")
        if on_device:
            if mask.is_cuda and mask.device != device:
                raise ValueError(f"{what}: mask and the block live on different devices")
            return mask.to(device).contiguous().view(torch.uint8)
        mask = mask.cpu().numpy()
    m = np.asarray(mask)
    if m.dtype not in (np.uint8, np.bool_):
        raise TypeError(f"{what}: mask must be uint8 or bool, got {m.dtype}")
    if m.ndim != 1 or m.size != total_rows:
        raise ValueError(f"{what}: mask must have one entry for each of the block's {total_rows} rows")
    m = np.ascontiguousarray(m).view(np.uint8)
    if on_device:
        import torch

        return torch.from_numpy(m).to(device)
    return m


def select_rows_packed(vec, row_offsets, mask, trim=True):
    """Kaldi ``select-voiced-frames`` on a packed block [sum T_b, cols]: the rows whose ``mask`` entry is not 0, clip by clip in
    order, and the table of the result -> (out, out_offsets), ``out_offsets[b + 1] - out_offsets[b]`` the kept rows of clip b.  Every
    float is a bit copy.  ``mask`` is any uint8 / bool vector with one entry per row, ``vad_energy_packed``'s or another.  numpy in ->
    the host-pointer call.  A ROCm tensor stays on the device (current stream) and ``out_offsets`` is a device tensor that
    ``cmvn_packed``, ``add_deltas_packed`` ... accept as it is; the result is trimmed to ``out_offsets[-1]`` rows with one read of
    that number, and ``trim=False`` returns the full-capacity block [sum T_b, cols] (rows past ``out_offsets[-1]`` uninitialised)
    without any synchronisation.  See ``ss_select_rows_packed`` in ``include/speechsauce_amd.h``."""
    what = "select_rows_packed"
    lib = _lib.lib()
    x, on_device, total_rows, cols = _packed_block(vec, None, what)
    table, n = _segment_table(row_offsets, on_device, x.device if on_device else None, total_rows, what)
    m = _row_mask(mask, on_device, x.device if on_device else None, total_rows, what)
    if on_device:
        import torch

        out = torch.empty_like(x)
        oo = torch.zeros(n + 1, dtype=torch.int64, device=x.device)
        if n and cols and total_rows:
            _launch(x.device, lib.ss_select_rows_packed_device, x, n, table, total_rows, cols, m, oo.data_ptr(), out.data_ptr())
        if not trim:
            return out, oo
        return out[:int(oo[-1])], oo
    out, oo = np.empty_like(x), np.zeros(n + 1, dtype=np.int64)
    if n and cols and total_rows:
        _lib.check(lib.ss_select_rows_packed(x.ctypes.data, n, table.ctypes.data, total_rows, cols, m.ctypes.data, oo.ctypes.data, out.ctypes.data))
    return (out[:int(oo[-1])] if trim else out), oo


def select_rows(x, mask):
    """``select_rows_packed`` of one matrix [T, cols]: the rows whose ``mask`` entry is not 0 -> [kept, cols]."""
    x = _require_f32(x, (2,), "select_rows")
    out, _ = select_rows_packed(x, np.array([0, int(x.shape[0])], dtype=np.int64), mask)
    return out


class VadEnergyStreamPool(_SidePool):
    """``vad_energy`` over the rows of live streams, with a fixed latency of ``delay_rows = frames_context`` rows: byte k of an entry
    is the decision for stream row ``rows_seen + k - delay_rows`` (0 while that is negative: the first ``delay_rows`` bytes after a
    reset are warm-up).  ``pool(rows, row_offsets, slots)`` takes the ``(rows, row_offsets)`` pair of a feature pool call and the
    ``slots`` that call was given and returns uint8 ``[total_rows]``: an entry gets exactly as many bytes as it brought rows.
    ``flush(slots)`` returns the last ``delay_rows`` decisions of those streams, ``[len(slots) * delay_rows]``, and makes them fresh.
    The threshold is causal: the decision for row t compares with ``energy_threshold + energy_mean_scale *`` the mean energy of the
    rows that have arrived when t is decided.  With ``energy_mean_scale = 0`` a stream's bytes plus the flush, the first
    ``delay_rows`` dropped, are ``vad_energy`` of the whole clip however it was cut.  ``rows_seen`` (int64 per slot, on the host)
    moves only after a call went through.  numpy in -> the host-pointer calls, ROCm tensors in -> the device calls on the current
    stream.  See ``ss_vad_energy_stream_packed`` in ``include/speechsauce_amd.h``."""

    _what, _stem, _dtype = "VadEnergyStreamPool", "vad_energy", "uint8"

    def __init__(self, pool_streams, cols, energy_col=0, energy_threshold=5.0, energy_mean_scale=0.5, frames_context=0, proportion_threshold=0.6):
        super().__init__(pool_streams, cols)
        (self.energy_col, self.energy_threshold, self.energy_mean_scale, self.frames_context,
         self.proportion_threshold) = _check_vad_params(energy_col, self.cols, energy_threshold, energy_mean_scale, frames_context, proportion_threshold,
                                                        self._what)
        L = C.c_size_t()
        _lib.check(_lib.lib().ss_vad_energy_stream_state_len(self.frames_context, C.byref(L)))
        self.state_len, self.delay_rows = L.value, self.frames_context  # 2 * frames_context + 4

    def _flush_scalars(self):  # the decision's: the flush reads no row
        return self.energy_threshold, self.energy_mean_scale, self.frames_context, self.proportion_threshold

    def _scalars(self):
        return self.cols, self.energy_col, *self._flush_scalars()

    def _out_shape(self, n):
        return (n,)

    def _flush_shape(self, n_active):
        return (n_active * self.delay_rows,)

    def flush(self, slots):
        """The last ``delay_rows`` decisions of the given streams, uint8 ``[len(slots) * delay_rows]`` (entry i: bytes i * delay_rows ..
        (i + 1) * delay_rows, stream rows rows_seen - delay_rows .. rows_seen - 1, 0 where that is negative); afterwards those streams
        are fresh.  Before the pool's first call there is no state anywhere: the bytes are zeros in a numpy array."""
        return self._flush(slots)


# ---- padded-batch collation of packed rows (ss_pad_packed*): the rectangular batch a model takes ---------------------------------
# out[b, t, c] ("btc") or out[b, c, t] ("bct") = the clip's row t for t < min(T_b, max_rows), pad_value behind it; float32 is a bit
# copy, float16 / bfloat16 round to nearest even.

_PAD_LAYOUTS = {"btc": 0, "bct": 1}
_PAD_DTYPES = {"float32": 0, "float16": 1, "bfloat16": 2}


def _pad_dtype(dtype, what):
    """-> (SS_PAD_* code, name) of a dtype given as a string, a torch dtype or a numpy dtype"""
    name = dtype if isinstance(dtype, str) else None
    if name is None and type(dtype).__module__.split(".")[0] == "torch":
        name = str(dtype).split(".")[-1]
    if name is None:
        try:
            name = np.dtype(dtype).name
        except TypeError:
            name = repr(dtype)
    if name not in _PAD_DTYPES:
        raise ValueError(f"{what}: dtype must be float32, float16 or bfloat16, got {dtype!r}")
    return _PAD_DTYPES[name], name


def pad_packed(vec, row_offsets, max_rows=None, layout="btc", dtype="float32", pad_value=0.0):
    """The padded batch of a packed block [sum T_b, cols], one launch for all clips: -> (out, lengths).  ``out`` is ``[n_clips,
    max_rows, cols]`` (``layout="btc"``) or ``[n_clips, cols, max_rows]`` (``"bct"``) in ``dtype`` (``"float32"``, ``"float16"``,
    ``"bfloat16"`` or the torch dtypes): clip b's first ``min(T_b, max_rows)`` rows, ``pad_value`` behind them; ``lengths`` (int32)
    holds that row count, -1 for a segment a device table got wrong.  float32 is a bit copy, the 16-bit types round to nearest
    even.  numpy in -> the host-pointer call; float16 comes back as ``np.float16``, bfloat16 as its ``np.uint16`` bit patterns.  A
    ROCm tensor stays on the device (current stream): ``out`` is a tensor of the torch dtype, ``lengths`` an int32 device tensor.
    ``row_offsets`` may be a device tensor, used as it is (``select_rows_packed(..., trim=False)``'s, for example), or a host array.
    ``max_rows=None`` takes the longest clip from a host table; a device table needs an explicit ``max_rows`` (nothing is read
    back).  See ``ss_pad_packed`` in ``include/speechsauce_amd.h``."""
    what = "pad_packed"
    if layout not in _PAD_LAYOUTS:
        raise ValueError(f"{what}: layout must be 'btc' or 'bct', got {layout!r}")
    code, name = _pad_dtype(dtype, what)
    if max_rows is None and _is_torch(row_offsets) and row_offsets.is_cuda:
        raise ValueError(f"{what}: a device row_offsets table needs an explicit max_rows (the table is not read back)")
    if max_rows is not None and int(max_rows) < 1:
        raise ValueError(f"{what}: max_rows must be at least 1")
    lib = _lib.lib()
    x, on_device, total_rows, cols = _packed_block(vec, None, what)
    if cols < 1:
        raise ValueError(f"{what}: the block has no columns")
    table, n = _segment_table(row_offsets, on_device, x.device if on_device else None, total_rows, what)
    if max_rows is None:  # a host table, validated above: the longest clip
        host = np.asarray(row_offsets.numpy() if _is_torch(row_offsets) else row_offsets)
        max_rows = int(np.diff(host).max()) if n else 0
    max_rows = int(max_rows)
    shape = (n, max_rows, cols) if layout == "btc" else (n, cols, max_rows)
    pad_value = float(pad_value)
    if on_device:
        import torch

        out = torch.empty(shape, dtype=getattr(torch, name), device=x.device)
        lengths = torch.zeros(n, dtype=torch.int32, device=x.device)
        if n and max_rows:
            if total_rows == 0:  # every clip is empty: the call still wants a block
                x = torch.zeros((1, cols), dtype=torch.float32, device=x.device)
            _launch(x.device, lib.ss_pad_packed_device, x, n, table, total_rows, cols, max_rows, _PAD_LAYOUTS[layout], code, pad_value, out.data_ptr(),
                    lengths.data_ptr())
        return out, lengths
    out = np.empty(shape, dtype={"float32": np.float32, "float16": np.float16, "bfloat16": np.uint16}[name])
    lengths = np.zeros(n, dtype=np.int32)
    if n and max_rows:
        if total_rows == 0:
            x = np.zeros((1, cols), dtype=np.float32)
        _lib.check(lib.ss_pad_packed(x.ctypes.data, n, table.ctypes.data, total_rows, cols, max_rows, _PAD_LAYOUTS[layout], code, pad_value,
                                     out.ctypes.data, lengths.ctypes.data))
    return out, lengths


def pad(matrices, max_rows=None, layout="btc", dtype="float32", pad_value=0.0):
    """``pad_packed`` of a list of matrices ``[T_i, cols]`` (all numpy arrays or all tensors of one device): -> (out, lengths)."""
    what = "pad"
    mats = list(matrices)
    if not mats:
        raise ValueError(f"{what}: the list is empty")
    for m in mats:
        if len(m.shape) != 2 or int(m.shape[1]) != int(mats[0].shape[1]):
            raise ValueError(f"{what}: every matrix must be [T_i, cols] with the same cols")
    if any(_is_torch(m) for m in mats) != all(_is_torch(m) for m in mats):
        raise TypeError(f"{what}: the matrices must be all numpy arrays or all tensors")
    ro = np.concatenate([[0], np.cumsum([int(m.shape[0]) for m in mats])]).astype(np.int64)
    if _is_torch(mats[0]):
        import torch

        block = torch.cat(mats)
    else:
        block = np.concatenate([np.asarray(m) for m in mats])
    return pad_packed(block, ro, max_rows, layout, dtype, pad_value)


# ---- SpecAugment: time / frequency masking of packed rows, seeded on the device (ss_specaug_* / ss_mask_spans_*) ------------------
# A clip's spans are a pure function of (seed, epoch, clip_base + b, T_b, cols, the scalars): Philox4x32-10, no generator state.

def _specaug_scalars(time_masks, time_width, time_ratio, freq_masks, freq_width, clip_base, what):
    nt, nf, tw, fw, base, ratio = int(time_masks), int(freq_masks), int(time_width), int(freq_width), int(clip_base), float(time_ratio)
    if not (0 <= nt <= 16 and 0 <= nf <= 16):
        raise ValueError(f"{what}: time_masks and freq_masks must lie in 0 .. 16")
    if not (0 <= tw < 1 << 31 and 0 <= fw < 1 << 31):
        raise ValueError(f"{what}: time_width and freq_width must lie in 0 .. 2^31 - 1")
    if not 0.0 <= ratio <= 1.0:
        raise ValueError(f"{what}: time_ratio must lie in [0, 1]")
    if not 0 <= base <= 1 << 32:
        raise ValueError(f"{what}: clip_base must lie in 0 .. 2^32")
    return nt, tw, ratio, nf, fw, base


def _rng_words(rng, what):
    """-> the uint64 pair {seed, epoch} of a host-side rng: a SpecAugment (read back), a pair of ints or an array of two"""
    if isinstance(rng, SpecAugment):
        return np.array([rng.seed, rng.epoch], np.uint64)
    if isinstance(rng, np.ndarray) and rng.dtype == np.uint64 and rng.shape == (2,):
        return np.ascontiguousarray(rng)
    try:
        seed, epoch = (int(v) for v in rng)
    except (TypeError, ValueError):
        raise TypeError(f"{what}: rng must be a SpecAugment, a (seed, epoch) pair or a uint64 array of two") from None
    if not (0 <= seed < 1 << 64 and 0 <= epoch < 1 << 64):
        raise ValueError(f"{what}: seed and epoch must lie in 0 .. 2^64 - 1")
    return np.array([seed, epoch], np.uint64)


def spec_augment_spans(rng, row_offsets, cols, time_masks=2, time_width=100, time_ratio=1.0, freq_masks=2, freq_width=27, clip_base=0,
                       total_rows=None):
    """The spans ``spec_augment_packed`` draws, computed on the host (no device): int32 ``[n_clips, time_masks + freq_masks, 2]`` of
    ``(start, width)`` pairs, time masks first.  ``rng`` is a ``(seed, epoch)`` pair, a uint64 array of two or a ``SpecAugment``
    (read back); ``row_offsets`` a host table, taken as it is: a segment that is reversed, starts below 0 or ends past
    ``total_rows`` (default: the table's last entry) has ``(-1, 0)`` in every span, as on the device."""
    what = "spec_augment_spans"
    nt, tw, ratio, nf, fw, base = _specaug_scalars(time_masks, time_width, time_ratio, freq_masks, freq_width, clip_base, what)
    words = _rng_words(rng, what)
    off = np.asarray(row_offsets.cpu().numpy() if _is_torch(row_offsets) else row_offsets)
    if off.ndim != 1 or off.size < 1 or not np.issubdtype(off.dtype, np.integer):
        raise ValueError(f"{what}: row_offsets must be 1-D integers with n_clips + 1 entries")
    off = np.ascontiguousarray(off, dtype=np.int64)
    if int(cols) < 1:
        raise ValueError(f"{what}: cols must be at least 1")
    total = max(int(off[-1]), 0) if total_rows is None else int(total_rows)
    n = off.size - 1
    spans = np.zeros((n, nt + nf, 2), np.int32)
    if n and nt + nf:
        _lib.check(_lib.lib().ss_specaug_spans(words.ctypes.data, base, n, off.ctypes.data, total, int(cols), nt, tw, ratio, nf, fw, spans.ctypes.data))
    return spans


def _mask_block(rows, row_offsets, out, what):
    """-> (x, on_device, total_rows, cols, table, n, out) of a masking call; ``out`` None is a fresh block, ``out`` on the block's own
    memory is the in-place call"""
    x, on_device, total_rows, cols = _packed_block(rows, None, what)
    if cols < 1:
        raise ValueError(f"{what}: the block has no columns")
    table, n = _segment_table(row_offsets, on_device, x.device if on_device else None, total_rows, what)
    if on_device:
        import torch

        if out is None:
            out = torch.empty_like(x)
        elif not (_is_torch(out) and out.is_cuda and out.device == x.device and out.dtype == torch.float32 and out.is_contiguous() and out.shape == x.shape):
            raise ValueError(f"{what}: out must be a contiguous float32 device tensor of the block's shape")
    elif out is None:
        out = np.empty_like(x)
    elif not (isinstance(out, np.ndarray) and out.dtype == np.float32 and out.flags.c_contiguous and out.flags.writeable and out.shape == x.shape):
        raise ValueError(f"{what}: out must be a writable contiguous float32 array of the block's shape")
    return x, on_device, total_rows, cols, table, n, out


def mask_spans_packed(rows, row_offsets, spans, n_time, n_freq, mask_value=0.0, out=None):
    """Overwrite spans of rows and of columns of every clip of a packed block [sum T_b, cols] with ``mask_value``: ``spans`` is the
    int32 table ``[n_clips, n_time + n_freq, 2]`` of ``(start, width)`` pairs, time spans (rows of the clip) first, then frequency
    spans (columns) -- the table ``spec_augment_packed`` returns, so that one plan can be applied to a second block, or the caller's
    own.  A span that does not lie inside its clip is skipped whole.  ``out=rows`` masks in place (only the masked elements are
    written); a fresh ``out`` holds a bit copy of every unmasked element, and rows that no clip covers are uninitialised.  numpy in
    -> the host-pointer call; a ROCm tensor stays on the device (current stream, nothing is read back)."""
    what = "mask_spans_packed"
    nt, nf = int(n_time), int(n_freq)
    if not (0 <= nt <= 16 and 0 <= nf <= 16):
        raise ValueError(f"{what}: n_time and n_freq must lie in 0 .. 16")
    x, on_device, total_rows, cols, table, n, out = _mask_block(rows, row_offsets, out, what)
    lib, mask_value = _lib.lib(), float(mask_value)
    if on_device:
        import torch

        if _is_torch(spans):
            if spans.dtype != torch.int32:
                raise TypeError(f"{what}: spans must be int32, got {spans.dtype}")
            sp = spans.to(x.device).contiguous()
        else:
            sp = torch.from_numpy(np.ascontiguousarray(spans, dtype=np.int32)).to(x.device)
        if sp.numel() != n * (nt + nf) * 2:
            raise ValueError(f"{what}: spans must hold n_clips * (n_time + n_freq) pairs")
        if n and total_rows:
            _launch(x.device, lib.ss_mask_spans_packed_device, x, n, table, total_rows, cols, sp, nt, nf, mask_value, out.data_ptr())
        return out
    sp = np.ascontiguousarray(spans.cpu().numpy() if _is_torch(spans) else spans)
    if sp.dtype != np.int32:
        raise TypeError(f"{what}: spans must be int32, got {sp.dtype}")
    if sp.size != n * (nt + nf) * 2:
        raise ValueError(f"{what}: spans must hold n_clips * (n_time + n_freq) pairs")
    if n and total_rows:
        _lib.check(lib.ss_mask_spans_packed(x.ctypes.data, n, table.ctypes.data, total_rows, cols, sp.ctypes.data if sp.size else None, nt, nf, mask_value,
                                            out.ctypes.data))
    return out


def spec_augment_packed(rows, row_offsets, rng, time_masks=2, time_width=100, time_ratio=1.0, freq_masks=2, freq_width=27, mask_value=0.0,
                        clip_base=0, out=None):
    """SpecAugment of every clip of a packed block [sum T_b, cols]: -> (out, spans).  ``time_masks`` spans of at most ``min(time_width,
    time_ratio * T_b)`` rows and ``freq_masks`` spans of at most ``freq_width`` columns of every clip are overwritten with
    ``mask_value`` (after CMVN the mean is 0); widths and starts are uniform draws of Philox4x32-10 keyed by ``rng``'s seed and counted
    by its epoch and ``clip_base + b``, so a clip's masks depend on neither its place in the block nor its neighbours, and a shard
    that starts at global clip ``clip_base`` draws what the whole batch would.  The call advances the epoch by one: the next call,
    or the next replay of a captured graph, draws other masks.  ``spans`` is the int32 table ``[n_clips, time_masks + freq_masks, 2]``
    of ``(start, width)`` pairs that was applied.  On the device (ROCm tensors, current stream, nothing read back) ``rng`` is a
    ``SpecAugment`` or its int64 device block of two words; for numpy input it is a ``SpecAugment`` or a writable uint64 array
    ``[seed, epoch]``, updated in place.  ``out=rows`` masks in place; see ``mask_spans_packed``.  One ``rng`` serves one stream of
    calls: concurrent calls on one block race on its epoch."""
    what = "spec_augment_packed"
    nt, tw, ratio, nf, fw, base = _specaug_scalars(time_masks, time_width, time_ratio, freq_masks, freq_width, clip_base, what)
    x, on_device, total_rows, cols, table, n, out = _mask_block(rows, row_offsets, out, what)
    lib, mask_value = _lib.lib(), float(mask_value)
    if on_device:
        import torch

        block = rng._block if isinstance(rng, SpecAugment) else rng
        if not (_is_torch(block) and block.is_cuda and block.device == x.device and block.dtype == torch.int64 and block.numel() == 2 and block.is_contiguous()):
            raise TypeError(f"{what}: on the device rng must be a SpecAugment or a contiguous int64 tensor of two words on the block's device")
        spans = torch.zeros((n, nt + nf, 2), dtype=torch.int32, device=x.device)
        if n:
            xin, xout = (x, out) if total_rows else (torch.zeros((1, cols), device=x.device),) * 2  # no rows: the call still wants a block
            _launch(x.device, lib.ss_specaug_packed_device, xin, n, table, total_rows, cols, block.data_ptr(), base, nt, tw, ratio, nf, fw, mask_value,
                    xout.data_ptr(), _ptr(spans) or None)
        return out, spans
    words = _rng_words(rng, what)
    spans = np.zeros((n, nt + nf, 2), np.int32)
    if n:
        xin, xout = (x, out) if total_rows else (np.zeros((1, cols), np.float32),) * 2
        _lib.check(lib.ss_specaug_packed(xin.ctypes.data, n, table.ctypes.data, total_rows, cols, words.ctypes.data, base, nt, tw, ratio, nf, fw, mask_value,
                                         xout.ctypes.data, spans.ctypes.data if spans.size else None))
        if isinstance(rng, SpecAugment):
            rng.epoch = int(words[1])
        elif isinstance(rng, np.ndarray) and rng is not words:
            rng[1] = words[1]
    return out, spans


class SpecAugment:
    """The generator state of ``spec_augment_packed``: owns the 16-byte device block ``{seed, epoch}`` that the kernels read and
    advance.  ``augment = SpecAugment(seed)``; ``out, spans = augment(rows, row_offsets, time_masks=2, ...)`` -- every call, and
    every replay of a graph that captured one, advances ``epoch`` by one on the device.  ``seed`` and ``epoch`` read the block back
    (a synchronisation: for tests and checkpoints); assigning ``epoch`` restores a checkpoint."""

    def __init__(self, seed, epoch=0, device=None):
        import torch

        seed, epoch = int(seed), int(epoch)
        if not (0 <= seed < 1 << 64 and 0 <= epoch < 1 << 64):
            raise ValueError("SpecAugment: seed and epoch must lie in 0 .. 2^64 - 1")
        self._block = torch.from_numpy(np.array([seed, epoch], np.uint64).view(np.int64)).to(device if device is not None else "cuda")

    def _words(self):
        return self._block.cpu().numpy().view(np.uint64)

    @property
    def seed(self):
        return int(self._words()[0])

    @property
    def epoch(self):
        return int(self._words()[1])

    @epoch.setter
    def epoch(self, value):
        import torch

        value = int(value)
        if not 0 <= value < 1 << 64:
            raise ValueError("SpecAugment: epoch must lie in 0 .. 2^64 - 1")
        self._block[1:].copy_(torch.from_numpy(np.array([value], np.uint64).view(np.int64)))

    def __call__(self, rows, row_offsets, **kwargs):
        return spec_augment_packed(rows, row_offsets, self, **kwargs)


# ---- additive noise at a drawn SNR and gain perturbation of packed clips, seeded on the device (ss_noise_*) --------------------
# A clip's plan row is a function of (seed, epoch, clip_base + b), its own samples, the bank and the scalars; the mix is a function
# of the row.  The generator block is SpecAugment's: one seed may serve both stages (the counter words differ).

#: ``ss_noise_plan_row``: one row per clip of the plan tables below (40 bytes)
NOISE_PLAN_DTYPE = np.dtype([("noise_clip", np.int32), ("start", np.int32), ("snr_db", np.float32), ("gain_db", np.float32),
                             ("speech_gain", np.float32), ("noise_gain", np.float32), ("speech_energy", np.float64), ("noise_energy", np.float64)])


def noise_plan_rows(plan):
    """A plan table as a numpy record array of ``NOISE_PLAN_DTYPE``: a device plan (int64 ``[n_clips, 5]``, the 40-byte rows as
    they lie in memory) is read back (a synchronisation); a host plan is returned as it is."""
    if _is_torch(plan):
        return plan.detach().cpu().contiguous().numpy().reshape(-1).view(NOISE_PLAN_DTYPE)
    return np.ascontiguousarray(plan).reshape(-1).view(NOISE_PLAN_DTYPE)


class _NoiseBank:
    """The noise bank of one call, or of a ``NoiseMix``: packed samples (float32, or int16 with its scale), the offset table and
    the counts; with ``device`` both live there."""

    def __init__(self, bank, bank_lengths, noise_pcm_scale, what, device=None):
        nz, self.scale = _require_signal(bank, (1,), what, noise_pcm_scale)
        self.total = int(nz.shape[0])
        table = _sample_offsets(bank_lengths, self.total, what)
        self.n_noise = table.size - 1
        if device is not None or _is_torch(nz):
            import torch

            device = nz.device if device is None else torch.device(device)
            self.nz = (nz if _is_torch(nz) else torch.from_numpy(np.ascontiguousarray(nz))).to(device).contiguous()
            self.table = torch.from_numpy(table).to(device)
        else:
            self.nz, self.table = np.ascontiguousarray(nz), table
        self.on_device = _is_torch(self.nz)

    def args(self, on_device, scale, what):
        """the bank's part of a call's argument list, for a signal on the device or not, float or PCM (``scale``)"""
        if (scale is None) != (self.scale is None):
            raise ValueError(f"{what}: the signal and the bank must both be float32 or both int16 PCM (pcm_scale and noise_pcm_scale)")
        if on_device != self.on_device:
            raise ValueError(f"{what}: the signal and the bank must both be on the device or both on the host")
        sc = [] if scale is None else [self.scale]
        if on_device:
            return [self.nz if self.total else None, *sc, self.n_noise, self.table, self.total]
        return [self.nz.ctypes.data if self.total else None, *sc, self.n_noise, self.table.ctypes.data, self.total]


def _noise_scalars(prob, snr_db, gain_db, clip_base, what):
    try:
        (snr_lo, snr_hi), (gain_lo, gain_hi) = (tuple(float(np.float32(v)) for v in pair) for pair in (snr_db, gain_db))
    except (TypeError, ValueError):
        raise TypeError(f"{what}: snr_db and gain_db must be (low, high) pairs of numbers") from None
    prob, base = float(prob), int(clip_base)
    if not 0.0 <= prob <= 1.0:
        raise ValueError(f"{what}: prob must lie in [0, 1]")
    for name, lo, hi in (("snr_db", snr_lo, snr_hi), ("gain_db", gain_lo, gain_hi)):
        if not (np.isfinite(lo) and np.isfinite(hi) and lo <= hi):
            raise ValueError(f"{what}: {name} must be a finite (low, high) pair with low <= high")
    if not 0 <= base <= 1 << 32:
        raise ValueError(f"{what}: clip_base must lie in 0 .. 2^32")
    return base, [prob, snr_lo, snr_hi, gain_lo, gain_hi]


def _noise_rng(rng):
    return rng.rng if isinstance(rng, NoiseMix) else rng


def noise_draws(rng, lengths, bank_lengths, prob=1.0, snr_db=(10, 30), gain_db=(0, 0), clip_base=0, *, sample_offsets=None, noise_offsets=None,
                total_samples=None, total_noise=None):
    """The draw fields ``noise_mix_packed`` writes, computed on the host (no device): a record array of ``NOISE_PLAN_DTYPE`` whose
    ``noise_clip``, ``start``, ``snr_db`` and ``gain_db`` are those of the device plan (the gains and energies are 0).  ``rng`` is
    a ``(seed, epoch)`` pair, a uint64 array of two, a ``SpecAugment`` or a ``NoiseMix`` (read back).  ``sample_offsets`` /
    ``noise_offsets`` (with ``lengths`` / ``bank_lengths`` None) are offset tables taken as they stand, with ``total_samples`` /
    ``total_noise`` (default: the table's last entry): a bad speech segment has ``noise_clip == -2``, as on the device."""
    what = "noise_draws"
    base, scalars = _noise_scalars(prob, snr_db, gain_db, clip_base, what)
    words = _rng_words(_noise_rng(rng), what)
    tables = []
    for lens, off, total in ((lengths, sample_offsets, total_samples), (bank_lengths, noise_offsets, total_noise)):
        if (lens is None) == (off is None):
            raise ValueError(f"{what}: give lengths or an offset table, not both")
        off = _sample_offsets(lens, 1 << 62, what) if off is None else np.ascontiguousarray(off.cpu().numpy() if _is_torch(off) else off, dtype=np.int64)
        if off.ndim != 1 or off.size < 1:
            raise ValueError(f"{what}: an offset table has n + 1 entries")
        tables.append((off, max(int(off[-1]), 0) if total is None else int(total)))
    (so, total), (no, ntotal) = tables
    plan = np.zeros(so.size - 1, NOISE_PLAN_DTYPE)
    if plan.size:
        _lib.check(_lib.lib().ss_noise_draws(words.ctypes.data, base, plan.size, so.ctypes.data, total, no.size - 1, no.ctypes.data, ntotal, *scalars,
                                             plan.ctypes.data))
    return plan


def _noise_signal(signal, lengths, pcm_scale, device_tables, what):
    """-> (x, scale, on_device, total_samples, table, n_clips) of a noise call"""
    x, scale = _require_signal(signal, (1,), what, pcm_scale)
    on_device, total = _is_torch(x), int(x.shape[0])
    if device_tables is not None:
        import torch

        t = device_tables[0] if isinstance(device_tables, (tuple, list)) else device_tables
        if lengths is not None or not on_device:
            raise ValueError(f"{what}: device_tables go with lengths=None and a device signal")
        if not (_is_torch(t) and t.is_cuda and t.dtype == torch.int64 and t.dim() == 1 and t.is_contiguous() and t.device == x.device and t.numel() >= 1):
            raise TypeError(f"{what}: device_tables is the sample offsets, a contiguous 1-D int64 tensor of n_clips + 1 entries on the signal's device")
        return x.contiguous(), scale, True, total, t, t.numel() - 1
    table = _sample_offsets(lengths, total, what)
    return (x.contiguous() if on_device else np.ascontiguousarray(x)), scale, on_device, total, table, table.size - 1


def _noise_out(x, scale, on_device, out, what):
    if on_device:
        import torch

        if out is None:
            return torch.empty(x.shape, dtype=torch.float32, device=x.device)
        if not (_is_torch(out) and out.is_cuda and out.device == x.device and out.dtype == torch.float32 and out.is_contiguous() and out.shape == x.shape):
            raise ValueError(f"{what}: out must be a contiguous float32 device tensor of the signal's shape")
        return out
    if out is None:
        return np.empty(x.shape, np.float32)
    if not (isinstance(out, np.ndarray) and out.dtype == np.float32 and out.flags.c_contiguous and out.flags.writeable and out.shape == x.shape):
        raise ValueError(f"{what}: out must be a writable contiguous float32 array of the signal's shape")
    return out


def _noise_block(x, out, total, on_device):
    """the blocks a call hands over: a signal without samples still wants a block"""
    if total:
        return x, out
    if on_device:
        import torch

        return torch.zeros(1, dtype=x.dtype, device=x.device), torch.zeros(1, dtype=torch.float32, device=x.device)
    return np.zeros(1, x.dtype), np.zeros(1, np.float32)


def _noise_device_rng(rng, x, what):
    import torch

    rng = _noise_rng(rng)
    block = rng._block if isinstance(rng, SpecAugment) else rng
    if not (_is_torch(block) and block.is_cuda and block.device == x.device and block.dtype == torch.int64 and block.numel() == 2 and block.is_contiguous()):
        raise TypeError(f"{what}: on the device rng must be a NoiseMix, a SpecAugment or a contiguous int64 tensor of two words on the signal's device")
    return block


def _noise_work(n, total, device, work=None):
    import torch

    need = C.c_size_t()
    _lib.check(_lib.lib().ss_noise_mix_work_bytes(n, total, C.byref(need)))
    if work is None or work.numel() * 8 < need.value or work.device != device:
        work = torch.empty(max(need.value // 8, 1), dtype=torch.float64, device=device)
    return work


def _noise_plan_or_mix(what, mix, signal, lengths, bank, rng, prob, snr_db, gain_db, clip_base, pcm_scale, out, device_tables, work=None):
    base, scalars = _noise_scalars(prob, snr_db, gain_db, clip_base, what)
    x, scale, on_device, total, table, n = _noise_signal(signal, lengths, pcm_scale, device_tables, what)
    bank_args = bank.args(on_device, scale, what)
    if mix:
        out = _noise_out(x, scale, on_device, out, what)
    lib, i16, sc = _lib.lib(), "" if scale is None else "_i16", [] if scale is None else [scale]
    if on_device:
        import torch

        block = _noise_device_rng(rng, x, what)
        plan = torch.zeros((n, 5), dtype=torch.int64, device=x.device)
        if n:
            work = _noise_work(n, total, x.device, work)
            xin, xout = _noise_block(x, out, total, True)
            outs = [xout.data_ptr()] if mix else []
            _launch(x.device, getattr(lib, f"ss_noise_{'mix' if mix else 'plan'}_packed{i16}_device"), xin, *sc, n, table, total, *bank_args, block.data_ptr(),
                    base, *scalars, *outs, plan.data_ptr(), work.data_ptr(), work.numel() * 8)
            work.record_stream(torch.cuda.current_stream(x.device))
        return out, plan, work
    if not mix:
        raise TypeError(f"{what}: the plan alone is a device call; numpy input is served by noise_draws and noise_mix_packed")
    words = _rng_words(_noise_rng(rng), what)
    plan = np.zeros(n, NOISE_PLAN_DTYPE)
    if n:
        xin, xout = _noise_block(x, out, total, False)
        _lib.check(getattr(lib, f"ss_noise_mix_packed{i16}")(xin.ctypes.data, *sc, n, table.ctypes.data, total, *bank_args, words.ctypes.data, base, *scalars,
                                                           xout.ctypes.data, plan.ctypes.data))
        rng = _noise_rng(rng)
        if isinstance(rng, SpecAugment):
            rng.epoch = int(words[1])
        elif isinstance(rng, np.ndarray) and rng is not words:
            rng[1] = words[1]
    return out, plan, None


def noise_plan_packed(signal, lengths, bank, bank_lengths, rng, prob=1.0, snr_db=(10, 30), gain_db=(0, 0), clip_base=0, pcm_scale=None,
                      noise_pcm_scale=None, device_tables=None):
    """The plan of ``noise_mix_packed`` alone, on the device: draws, f64 energies and gains of every clip -> the plan table (int64
    ``[n_clips, 5]``: 40-byte rows, see ``noise_plan_rows``).  The epoch is not advanced and nothing is mixed."""
    what = "noise_plan_packed"
    return _noise_plan_or_mix(what, False, signal, lengths, _NoiseBank(bank, bank_lengths, noise_pcm_scale, what), rng, prob, snr_db, gain_db, clip_base,
                              pcm_scale, None, device_tables)[1]


def _noise_apply(what, signal, lengths, bank, plan, pcm_scale, out, device_tables):
    x, scale, on_device, total, table, n = _noise_signal(signal, lengths, pcm_scale, device_tables, what)
    bank_args = bank.args(on_device, scale, what)
    out = _noise_out(x, scale, on_device, out, what)
    lib, i16, sc = _lib.lib(), "" if scale is None else "_i16", [] if scale is None else [scale]
    if on_device:
        import torch

        if _is_torch(plan):
            if plan.dtype != torch.int64:
                raise TypeError(f"{what}: a device plan is the int64 table [n_clips, 5] the plan and mix calls return")
            rows = plan.to(x.device).contiguous()
        else:
            rows = torch.from_numpy(noise_plan_rows(plan).view(np.int64).copy()).to(x.device)
        if rows.numel() != n * 5:
            raise ValueError(f"{what}: the plan must hold one row per clip")
        if n:
            xin, xout = _noise_block(x, out, total, True)
            _launch(x.device, getattr(lib, f"ss_noise_apply_packed{i16}_device"), xin, *sc, n, table, total, *bank_args, rows, xout.data_ptr())
        return out
    rows = noise_plan_rows(plan)
    if rows.size != n:
        raise ValueError(f"{what}: the plan must hold one row per clip")
    if n:
        xin, xout = _noise_block(x, out, total, False)
        _lib.check(getattr(lib, f"ss_noise_apply_packed{i16}")(xin.ctypes.data, *sc, n, table.ctypes.data, total, *bank_args, rows.ctypes.data, xout.ctypes.data))
    return out


def noise_apply_packed(signal, lengths, bank, bank_lengths, plan, pcm_scale=None, noise_pcm_scale=None, out=None, device_tables=None):
    """The mix of ``noise_mix_packed`` alone, on any plan table -- the one a plan or mix call returned (one plan applied twice gives
    equal outputs) or the caller's own record array of ``NOISE_PLAN_DTYPE`` with fixed ``speech_gain`` / ``noise_gain`` /
    ``noise_clip`` / ``start``: ``out[i] = fma(noise_gain, noise[(start + i) mod N], speech_gain * x[i])``.  A row whose
    ``noise_clip`` or ``start`` is out of range for the bank, or whose ``noise_gain`` is 0, is not mixed; ``noise_clip == -2``
    leaves the clip untouched.  ``out=signal`` (float32) mixes in place."""
    what = "noise_apply_packed"
    return _noise_apply(what, signal, lengths, _NoiseBank(bank, bank_lengths, noise_pcm_scale, what), plan, pcm_scale, out, device_tables)


def noise_mix_packed(signal, lengths, bank, bank_lengths, rng, prob=1.0, snr_db=(10, 30), gain_db=(0, 0), clip_base=0, pcm_scale=None,
                     noise_pcm_scale=None, out=None, device_tables=None):
    """Additive noise and gain perturbation of every clip of a packed 1-D signal, ahead of the front ends: -> (out, plan).  With
    probability ``prob`` a clip gets a segment of a uniformly drawn clip of ``bank`` (packed like the signal, ``bank_lengths``), from
    a uniformly drawn start and repeated as often as the clip needs, at an SNR drawn uniformly from ``snr_db`` (dB, measured on the
    clip's own f64 energies); every clip is scaled by a gain drawn from ``gain_db`` (``(0, 0)``: none).  The draws are Philox4x32-10
    keyed by ``rng``'s seed and counted by its epoch and ``clip_base + b``: a clip's noise depends on neither its place in the block
    nor its neighbours.  The call advances the epoch by one, so the next call, or the next replay of a captured graph, draws other
    noise.  ``plan`` is the table that was applied (``noise_plan_rows``).  ``pcm_scale`` and ``noise_pcm_scale`` (both or neither):
    signal and bank are int16 PCM, a sample is int16 * scale (a power of two); ``out`` is float32, bit for bit the float call on
    the converted arrays.  On the device (ROCm tensors, current stream, nothing read back) ``rng`` is a ``NoiseMix``, a
    ``SpecAugment`` or its int64 block; for numpy input also a writable uint64 array ``[seed, epoch]``, updated in place.
    ``device_tables``: the sample offsets as an int64 device tensor (with ``lengths=None``), used as they stand -- nothing is
    uploaded, so a captured graph can be replayed over changed tables.  ``(out, lengths)`` go on to every packed front end."""
    what = "noise_mix_packed"
    out, plan, _ = _noise_plan_or_mix(what, True, signal, lengths, _NoiseBank(bank, bank_lengths, noise_pcm_scale, what), rng, prob, snr_db, gain_db,
                                      clip_base, pcm_scale, out, device_tables)
    return out, plan


class NoiseMix:
    """``noise_mix_packed`` with its state: owns the generator block (``rng``, a ``SpecAugment``: pass it on to share the seed),
    the device copy of the noise bank and its offsets, and the scratch of the partial sums.  ``mix = NoiseMix(seed, bank,
    bank_lengths)``; ``out, plan = mix(signal, lengths, prob=0.5, snr_db=(10, 30))`` -- every call, and every replay of a graph that
    captured one, advances the epoch on the device."""

    def __init__(self, seed, bank, bank_lengths, noise_pcm_scale=None, epoch=0, device=None):
        self.rng = SpecAugment(seed, epoch, device)
        self.bank = _NoiseBank(bank, bank_lengths, noise_pcm_scale, "NoiseMix", self.rng._block.device)
        self._work = None

    seed = property(lambda self: self.rng.seed)
    epoch = property(lambda self: self.rng.epoch, lambda self, value: setattr(self.rng, "epoch", value))

    def plan(self, signal, lengths, prob=1.0, snr_db=(10, 30), gain_db=(0, 0), clip_base=0, pcm_scale=None, device_tables=None):
        _, plan, self._work = _noise_plan_or_mix("NoiseMix.plan", False, signal, lengths, self.bank, self.rng, prob, snr_db, gain_db, clip_base, pcm_scale,
                                                 None, device_tables, self._work)
        return plan

    def apply(self, signal, lengths, plan, pcm_scale=None, out=None, device_tables=None):
        return _noise_apply("NoiseMix.apply", signal, lengths, self.bank, plan, pcm_scale, out, device_tables)

    def __call__(self, signal, lengths, prob=1.0, snr_db=(10, 30), gain_db=(0, 0), clip_base=0, pcm_scale=None, out=None, device_tables=None):
        out, plan, self._work = _noise_plan_or_mix("NoiseMix", True, signal, lengths, self.bank, self.rng, prob, snr_db, gain_db, clip_base, pcm_scale, out,
                                                   device_tables, self._work)
        return out, plan


# ---- reverberation of packed clips from a bank of room impulse responses, seeded on the device (ss_reverb_*) --------------------
# A clip's plan row is a function of (seed, epoch, clip_base + b), its segment and the bank; the output is a function of the row and
# the clip's own samples.  The generator block is SpecAugment's: one seed may serve SpecAugment, NoiseMix and Reverb (the counter
# words differ).

#: ``ss_reverb_plan_row``: one row per clip of the plan tables below (8 bytes)
REVERB_PLAN_DTYPE = np.dtype([("rir", np.int32), ("shift", np.int32)])
_REVERB_NORMALIZE = {"none": 0, "energy": 1, "peak": 2}


def reverb_plan_rows(plan):
    """A plan table as a numpy record array of ``REVERB_PLAN_DTYPE``: a device plan (int32 ``[n_clips, 2]``, the 8-byte rows as they
    lie in memory) is read back (a synchronisation); a host plan is returned as it is."""
    if _is_torch(plan):
        return plan.detach().cpu().contiguous().numpy().reshape(-1).view(REVERB_PLAN_DTYPE)
    return np.ascontiguousarray(plan).reshape(-1).view(REVERB_PLAN_DTYPE)


class ReverbBank(_Handle):
    """Owns an ``ss_reverb_bank`` handle: impulse responses of 1 .. 16384 taps each, packed in the 1-D float32 ``rirs`` with their
    ``lengths``, normalised (``normalize``: "energy" -- unit energy, torchaudio's and lhotse's rule --, "peak" -- largest magnitude 1
    --, or "none"), their partition spectra formed on the host in f64 and -- after the first device call -- the device copy of those.
    ``align_peak=True`` keeps the direct path where it was (the output is shifted by each response's peak index, Kaldi's
    ``--shift-output=true``); ``False`` is ``fftconvolve(x, h)[:len(x)]``.  The arrays handed in are not kept."""

    _destroy = "ss_reverb_bank_destroy"

    def __init__(self, rirs, lengths, normalize="energy", align_peak=True):
        h = np.ascontiguousarray(_affine_host(rirs, "ReverbBank: rirs"), dtype=np.float32)
        if h.ndim != 1:
            raise ValueError("ReverbBank: rirs must be the responses packed in one 1-D array")
        if normalize not in _REVERB_NORMALIZE:
            raise ValueError('ReverbBank: normalize must be "energy", "peak" or "none"')
        table = _sample_offsets(lengths, int(h.shape[0]), "ReverbBank")
        super().__init__()
        _lib.check(self._owner.ss_reverb_bank_create(h.ctypes.data if h.size else None, table.size - 1, table.ctypes.data, int(h.shape[0]),
                                                     _REVERB_NORMALIZE[normalize], 1 if align_peak else 0, C.byref(self._h)))
        info = [C.c_size_t() for _ in range(4)]
        _lib.check(self._owner.ss_reverb_bank_info(self._h, *(C.byref(v) for v in info)))
        self.n_rir, self.block, self.max_taps, self.n_partitions = (int(v.value) for v in info)
        self.normalize, self.align_peak = normalize, bool(align_peak)

    def __len__(self):
        return self.n_rir

    def rir(self, c):
        """-> (taps, peak): the normalised float32 taps of response ``c`` exactly as the spectra were made from them, and the first
        index of their largest magnitude."""
        n, peak = C.c_size_t(), C.c_size_t()
        _lib.check(self._owner.ss_reverb_bank_rir(self._h, int(c), None, 0, C.byref(n), C.byref(peak)))
        taps = np.empty(n.value, np.float32)
        _lib.check(self._owner.ss_reverb_bank_rir(self._h, int(c), taps.ctypes.data, taps.size, C.byref(n), C.byref(peak)))
        return taps, int(peak.value)

    def shift(self, c):
        """the shift a plan row of response ``c`` carries: its peak index with ``align_peak``, else 0"""
        return self.rir(c)[1] if self.align_peak else 0

    def spectrum(self, c, p):
        """partition ``p`` of response ``c`` as the kernel multiplies by it: complex64 ``[2 * block]``"""
        out = np.empty(4 * self.block, np.float32)
        _lib.check(self._owner.ss_reverb_bank_spectrum(self._h, int(c), int(p), out.ctypes.data))
        return out.view(np.complex64)


def _reverb_rng(rng):
    return rng.rng if isinstance(rng, (Reverb, NoiseMix)) else rng


def _reverb_scalars(prob, clip_base, bank, what):
    if not isinstance(bank, ReverbBank):
        raise TypeError(f"{what}: bank must be a ReverbBank")
    prob, base = float(prob), int(clip_base)
    if not 0.0 <= prob <= 1.0:
        raise ValueError(f"{what}: prob must lie in [0, 1]")
    if not 0 <= base <= 1 << 32:
        raise ValueError(f"{what}: clip_base must lie in 0 .. 2^32")
    return prob, base


def reverb_draws(rng, lengths, bank, prob=1.0, clip_base=0, *, sample_offsets=None, total_samples=None):
    """The plan ``reverb_packed`` writes, computed on the host (no device): a record array of ``REVERB_PLAN_DTYPE``.  ``rng`` is a
    ``(seed, epoch)`` pair, a uint64 array of two, a ``SpecAugment``, a ``NoiseMix`` or a ``Reverb`` (read back).  ``sample_offsets``
    (with ``lengths`` None) is an offset table taken as it stands, with ``total_samples`` (default: the table's last entry): a bad
    speech segment has ``rir == -2``, as on the device."""
    what = "reverb_draws"
    prob, base = _reverb_scalars(prob, clip_base, bank, what)
    words = _rng_words(_reverb_rng(rng), what)
    if (lengths is None) == (sample_offsets is None):
        raise ValueError(f"{what}: give lengths or an offset table, not both")
    if sample_offsets is None:
        so = _sample_offsets(lengths, 1 << 62, what)
    else:
        so = np.ascontiguousarray(sample_offsets.cpu().numpy() if _is_torch(sample_offsets) else sample_offsets, dtype=np.int64)
    if so.ndim != 1 or so.size < 1:
        raise ValueError(f"{what}: an offset table has n + 1 entries")
    total = max(int(so[-1]), 0) if total_samples is None else int(total_samples)
    plan = np.zeros(so.size - 1, REVERB_PLAN_DTYPE)
    if plan.size:
        _lib.check(_lib.lib().ss_reverb_draws(words.ctypes.data, base, plan.size, so.ctypes.data, total, bank.handle, prob, plan.ctypes.data))
    return plan


def _reverb_out(x, scale, on_device, out, what):
    out = _noise_out(x, scale, on_device, out, what)
    if out is x:
        raise ValueError(f"{what}: out must not be the signal: the convolution is not in place")
    return out


def reverb_plan_packed(lengths, bank, rng, prob=1.0, clip_base=0, device_tables=None, total_samples=None):
    """The plan of ``reverb_packed`` alone, on the device: -> the plan table (int32 ``[n_clips, 2]``, see ``reverb_plan_rows``).
    The epoch is not advanced.  ``rng`` is a ``Reverb``, a ``NoiseMix``, a ``SpecAugment`` or its int64 block; the table comes from
    ``lengths``, or from ``device_tables`` (the sample offsets on the device, used as they stand, with ``total_samples`` the size of
    the block they index)."""
    import torch

    what = "reverb_plan_packed"
    prob, base = _reverb_scalars(prob, clip_base, bank, what)
    block = _reverb_rng(rng)
    block = block._block if isinstance(block, SpecAugment) else block
    if not (_is_torch(block) and block.is_cuda and block.dtype == torch.int64 and block.numel() == 2 and block.is_contiguous()):
        raise TypeError(f"{what}: rng must be a Reverb, a NoiseMix, a SpecAugment or a contiguous int64 device tensor of two words")
    if device_tables is not None:
        table = device_tables[0] if isinstance(device_tables, (tuple, list)) else device_tables
        if lengths is not None or total_samples is None:
            raise ValueError(f"{what}: device_tables go with lengths=None and total_samples")
        if not (_is_torch(table) and table.is_cuda and table.dtype == torch.int64 and table.dim() == 1 and table.is_contiguous() and table.numel() >= 1):
            raise TypeError(f"{what}: device_tables is the sample offsets, a contiguous 1-D int64 device tensor of n_clips + 1 entries")
        n, total = table.numel() - 1, int(total_samples)
    else:
        table = _sample_offsets(lengths, 1 << 62, what)
        n, total = table.size - 1, int(table[-1]) if total_samples is None else int(total_samples)
    plan = torch.zeros((n, 2), dtype=torch.int32, device=block.device)
    if n:
        _launch(block.device, _lib.lib().ss_reverb_plan_packed_device, n, table, total, bank.handle, block.data_ptr(), base, prob, plan.data_ptr())
    return plan


def _reverb_device_plan(plan, n, device, what):
    import torch

    if _is_torch(plan):
        if plan.dtype != torch.int32:
            raise TypeError(f"{what}: a device plan is the int32 table [n_clips, 2] the plan and combined calls return")
        rows = plan.to(device).contiguous()
    else:
        rows = torch.from_numpy(reverb_plan_rows(plan).view(np.int32).copy()).to(device)
    if rows.numel() != n * 2:
        raise ValueError(f"{what}: the plan must hold one row per clip")
    return rows


def reverb_apply_packed(signal, lengths, bank, plan, pcm_scale=None, out=None, device_tables=None):
    """The convolution of ``reverb_packed`` alone, on any plan table -- the one a plan or combined call returned (one plan applied
    twice gives equal outputs) or the caller's own record array of ``REVERB_PLAN_DTYPE``: ``out[i] = sum_k h[k] x[i + shift - k]``
    over the clip's own samples.  A row with ``rir == -1``, or whose ``rir`` or ``shift`` is out of range for the bank, is copied bit
    for bit; ``rir == -2`` leaves the clip's samples of ``out`` as they were.  ``out`` must not be the signal."""
    what = "reverb_apply_packed"
    _reverb_scalars(0.0, 0, bank, what)
    x, scale, on_device, total, table, n = _noise_signal(signal, lengths, pcm_scale, device_tables, what)
    out = _reverb_out(x, scale, on_device, out, what)
    lib, i16, sc = _lib.lib(), "" if scale is None else "_i16", [] if scale is None else [scale]
    if on_device:
        rows = _reverb_device_plan(plan, n, x.device, what)
        if n:
            xin, xout = _noise_block(x, out, total, True)
            _launch(x.device, getattr(lib, f"ss_reverb_apply_packed{i16}_device"), xin, *sc, n, table, total, bank.handle, rows, xout.data_ptr())
        return out
    rows = reverb_plan_rows(plan)
    if rows.size != n:
        raise ValueError(f"{what}: the plan must hold one row per clip")
    if n:
        xin, xout = _noise_block(x, out, total, False)
        _lib.check(getattr(lib, f"ss_reverb_apply_packed{i16}")(xin.ctypes.data, *sc, n, table.ctypes.data, total, bank.handle, rows.ctypes.data, xout.ctypes.data))
    return out


def reverb_packed(signal, lengths, bank, rng, prob=1.0, clip_base=0, pcm_scale=None, out=None, device_tables=None):
    """Reverberation of every clip of a packed 1-D signal, ahead of ``noise_mix_packed`` and the front ends: -> (out, plan).  With
    probability ``prob`` a clip is convolved with a uniformly drawn response of ``bank`` (a ``ReverbBank``); its length stays, and no
    clip reads its neighbour.  The draws are Philox4x32-10 keyed by ``rng``'s seed and counted by its epoch and ``clip_base + b``; the
    call advances the epoch by one, so the next call, or the next replay of a captured graph, draws afresh.  ``plan`` is the table
    that was applied (``reverb_plan_rows``).  ``pcm_scale``: the signal is int16 PCM, a sample is int16 * scale (a power of two);
    ``out`` is float32, bit for bit the float call on the converted array.  On the device (ROCm tensors, current stream, nothing read
    back) ``rng`` is a ``Reverb``, a ``NoiseMix``, a ``SpecAugment`` or its int64 block; for numpy input also a writable uint64 array
    ``[seed, epoch]``, updated in place.  ``device_tables``: the sample offsets as an int64 device tensor (with ``lengths=None``),
    used as they stand.  The bank's first device call uploads its spectra: make one call before capturing a graph.
    ``(out, lengths)`` go straight into ``noise_mix_packed`` and every packed front end."""
    what = "reverb_packed"
    prob, base = _reverb_scalars(prob, clip_base, bank, what)
    x, scale, on_device, total, table, n = _noise_signal(signal, lengths, pcm_scale, device_tables, what)
    out = _reverb_out(x, scale, on_device, out, what)
    lib, i16, sc = _lib.lib(), "" if scale is None else "_i16", [] if scale is None else [scale]
    if on_device:
        import torch

        block = _noise_device_rng(_reverb_rng(rng), x, what)
        plan = torch.zeros((n, 2), dtype=torch.int32, device=x.device)
        if n:
            xin, xout = _noise_block(x, out, total, True)
            _launch(x.device, getattr(lib, f"ss_reverb_packed{i16}_device"), xin, *sc, n, table, total, bank.handle, block.data_ptr(), base, prob,
                    xout.data_ptr(), plan.data_ptr())
        return out, plan
    rng = _reverb_rng(rng)
    words = _rng_words(rng, what)
    plan = np.zeros(n, REVERB_PLAN_DTYPE)
    if n:
        xin, xout = _noise_block(x, out, total, False)
        _lib.check(getattr(lib, f"ss_reverb_packed{i16}")(xin.ctypes.data, *sc, n, table.ctypes.data, total, bank.handle, words.ctypes.data, base, prob,
                                                         xout.ctypes.data, plan.ctypes.data))
        if isinstance(rng, SpecAugment):
            rng.epoch = int(words[1])
        elif isinstance(rng, np.ndarray) and rng is not words:
            rng[1] = words[1]
    return out, plan


class Reverb:
    """``reverb_packed`` with its state: the generator block (``rng``, a ``SpecAugment``) and the bank.  ``reverb = Reverb(seed,
    bank)``, or ``Reverb(augment, bank)`` / ``Reverb(noise_mix, bank)`` to share the block of a ``SpecAugment`` or a ``NoiseMix`` (the
    stages' counter words differ, and each call of each stage advances the shared epoch); ``out, plan = reverb(signal, lengths,
    prob=0.5)`` -- every call, and every replay of a graph that captured one, advances the epoch on the device."""

    def __init__(self, seed, bank, epoch=0, device=None):
        if not isinstance(bank, ReverbBank):
            raise TypeError("Reverb: bank must be a ReverbBank")
        shared = seed.rng if isinstance(seed, NoiseMix) else seed
        self.rng = shared if isinstance(shared, SpecAugment) else SpecAugment(seed, epoch, device)
        self.bank = bank

    seed = property(lambda self: self.rng.seed)
    epoch = property(lambda self: self.rng.epoch, lambda self, value: setattr(self.rng, "epoch", value))

    def plan(self, lengths, prob=1.0, clip_base=0, device_tables=None, total_samples=None):
        return reverb_plan_packed(lengths, self.bank, self.rng, prob, clip_base, device_tables, total_samples)

    def apply(self, signal, lengths, plan, pcm_scale=None, out=None, device_tables=None):
        return reverb_apply_packed(signal, lengths, self.bank, plan, pcm_scale, out, device_tables)

    def __call__(self, signal, lengths, prob=1.0, clip_base=0, pcm_scale=None, out=None, device_tables=None):
        return reverb_packed(signal, lengths, self.bank, self.rng, prob, clip_base, pcm_scale, out, device_tables)


# ---- polyphase sinc resampling ahead of the feature calls (ss_resample* in include/speechsauce_amd.h) -------------

class Resampler(_Handle):
    """Owns an ``ss_resampler`` handle: the windowed-sinc filter of ``torchaudio.functional.resample`` (``sinc_interp_hann``) for one
    pair of rates, and -- after the first device call -- its device copy.  ``info`` holds o, n, width, taps, lookback, lookahead,
    latency_periods and tile_outputs."""

    _destroy = "ss_resampler_destroy"

    def __init__(self, orig_rate, new_rate, lowpass_filter_width=6, rolloff=0.99):
        super().__init__()
        _lib.check(self._owner.ss_resampler_create(int(orig_rate), int(new_rate), int(lowpass_filter_width), float(rolloff), C.byref(self._h)))
        self.orig_rate, self.new_rate = int(orig_rate), int(new_rate)
        self.info = SsResampleInfo()
        _lib.check(self._owner.ss_resampler_info(self._h, C.byref(self.info)))

    def out_len(self, n_samples: int) -> int:
        """ceil(n * n_samples / o)"""
        return (int(n_samples) * self.info.n + self.info.o - 1) // self.info.o


@lru_cache(maxsize=32)
def _get_resampler(orig_rate, new_rate, lowpass_filter_width=6, rolloff=0.99, device: int = -1) -> Resampler:
    """Memoised handle factory; ``device`` is part of the key as for ``_get_speech_config``: the handle's table lives in the memory
    of the device of its first device call."""
    return Resampler(orig_rate, new_rate, lowpass_filter_width, rolloff)


_lib._on_switch.append(_get_resampler.cache_clear)  # a handle belongs to the library that created it


def _check_rates(orig_rate, new_rate, what):
    if int(orig_rate) != orig_rate or int(new_rate) != new_rate or int(orig_rate) <= 0 or int(new_rate) <= 0:
        raise ValueError(f"{what}: the rates must be positive integers, got {orig_rate!r} and {new_rate!r}")
    return int(orig_rate), int(new_rate)


def _resample_packed(sig, so, rs: Resampler, scale):
    """packed samples [N], sample offsets so (host int64) -> (out [sum out_len], out offsets (host int64))"""
    lib = _lib.lib()
    i16, sc = ("", []) if scale is None else ("_i16", [scale])
    n = so.size - 1
    oo = np.empty_like(so)
    _lib.check(lib.ss_resample_packed_offsets(rs.orig_rate, rs.new_rate, n, so.ctypes.data, oo.ctypes.data))
    total_in, total_out = int(so[-1]), int(oo[-1])
    if _is_torch(sig):
        import torch

        x = sig.contiguous()
        out = torch.empty((total_out,), dtype=torch.float32, device=x.device)
        if n and total_out:
            _launch(x.device, getattr(lib, f"ss_resample_packed{i16}_device"), rs.handle, x, n, so, *sc, oo, total_in, total_out, out.data_ptr())
        return out, oo
    x = np.ascontiguousarray(sig)
    out = np.empty((total_out,), dtype=np.float32)
    if n and total_out:
        _lib.check(getattr(lib, f"ss_resample_packed{i16}")(rs.handle, x.ctypes.data, n, so.ctypes.data, *sc, oo.ctypes.data, out.ctypes.data))
    return out, oo


def resample(x, orig_rate, new_rate, lowpass_filter_width=6, rolloff=0.99, pcm_scale=None):
    """``torchaudio.functional.resample(x, orig_rate, new_rate)`` with its default ``sinc_interp_hann`` filter, of one clip [L] or of
    every row of a batch [B, L] -> [ceil(n L / o)] or [B, ceil(n L / o)] float32.  numpy in -> the host-pointer call; a ROCm tensor
    stays on the device (current stream, one launch).  ``pcm_scale``: the samples are int16 PCM, sample = int16 * pcm_scale (a power
    of two), converted on load.  Equal rates return ``x`` unchanged, as torchaudio does."""
    what = "resample"
    orig_rate, new_rate = _check_rates(orig_rate, new_rate, what)
    if orig_rate == new_rate:
        return x
    sig, scale = _require_signal(x, (1, 2), what, pcm_scale)
    rs = _get_resampler(orig_rate, new_rate, int(lowpass_filter_width), float(rolloff), _device_key(sig))
    lib = _lib.lib()
    i16, sc = ("", []) if scale is None else ("_i16", [scale])
    one = len(sig.shape) == 1
    batch, L = (1, int(sig.shape[0])) if one else (int(sig.shape[0]), int(sig.shape[1]))
    out_len = rs.out_len(L)
    if _is_torch(sig):
        import torch

        v = sig.reshape(1, L) if one else sig
        if L and v.stride(1) != 1:
            v = v.contiguous()
        ld = int(v.stride(0)) if batch > 1 and L else L
        if ld < L:
            v, ld = v.contiguous(), L
        out = torch.empty((batch, out_len), dtype=torch.float32, device=v.device)
        if batch and out_len:
            _launch(v.device, getattr(lib, f"ss_resample{i16}_device"), rs.handle, v, batch, L, ld, *sc, out.data_ptr(), out_len)
        return out[0] if one else out
    v = np.ascontiguousarray(sig).reshape(batch, L)
    out = np.empty((batch, out_len), dtype=np.float32)
    if batch and out_len:
        _lib.check(getattr(lib, f"ss_resample{i16}")(rs.handle, v.ctypes.data, batch, L, L, *sc, out.ctypes.data, out_len))
    return out[0] if one else out


def resample_packed(signal, lengths, orig_rate, new_rate, lowpass_filter_width=6, rolloff=0.99, pcm_scale=None):
    """``resample`` of clips of different lengths packed end to end in one 1-D signal (float32, or int16 with ``pcm_scale``) ->
    (out [sum out_len_b] float32, out_lengths [n] int64 on the host): clip b's samples are what ``resample`` returns for that clip
    alone, bit for bit -- taps past a clip's end read zeros, never the next clip.  One launch for all clips.  ``(out, out_lengths)``
    is the ``(signal, lengths)`` of ``mfcc_packed`` and the other packed feature calls at ``new_rate``."""
    what = "resample_packed"
    orig_rate, new_rate = _check_rates(orig_rate, new_rate, what)
    sig, scale = _require_signal(signal, (1,), what, pcm_scale)
    so = _sample_offsets(lengths, sig.shape[0], what)
    if orig_rate == new_rate:
        return signal, np.diff(so)
    rs = _get_resampler(orig_rate, new_rate, int(lowpass_filter_width), float(rolloff), _device_key(sig))
    out, oo = _resample_packed(sig, so, rs, scale)
    return out, np.diff(oo)


def resample_list(signals, orig_rate, new_rate, lowpass_filter_width=6, rolloff=0.99, pcm_scale=None):
    """A list of 1-D clips of any lengths -> the list of their resampled clips (views of one block): the clips are packed once and
    served by one ``resample_packed`` call."""
    what = "resample_list"
    sigs = [_require_signal(x, (1,), what, pcm_scale)[0] for x in signals]
    if not sigs:
        return []
    on_device = [_is_torch(x) for x in sigs]
    if any(on_device) and not all(on_device):
        raise ValueError(f"{what}: the clips of one call must all be device tensors or all host arrays")
    if all(on_device):
        import torch

        if any(x.device != sigs[0].device for x in sigs):
            raise ValueError(f"{what}: the clips of one call must live on one device")
        packed = torch.cat(sigs)
    else:
        packed = np.concatenate(sigs)
    out, lens = resample_packed(packed, [int(x.shape[0]) for x in sigs], orig_rate, new_rate, lowpass_filter_width, rolloff, pcm_scale)
    oo = np.concatenate([[0], np.cumsum(lens)]).tolist()
    return [out[oo[b]:oo[b + 1]] for b in range(len(sigs))]


class ResampleStreamPool(_SidePool):
    """``resample`` over the samples of live streams, with a fixed latency of ``latency_periods`` periods: a stream is fed whole
    periods of ``o`` samples (``period_in``; 441 samples = 10 ms for 44.1 kHz -> 16 kHz) and gets ``n`` outputs (``period_out``) per
    period, ``lag = latency_periods * n`` outputs late (zeros while the stream's output time is negative: the first ``lag`` outputs
    after a reset are warm-up).  ``pool.push(samples, sample_offsets, slots)`` takes a packed block, the offsets of its entries and the
    pool rows they belong to, and returns ``[total / o * n]`` outputs: entry i's are ``out[sample_offsets[i] // o * n :
    sample_offsets[i + 1] // o * n]``.  ``flush(slots)`` returns the last ``lag`` outputs of those streams, ``[len(slots), lag]``, and
    makes them fresh.  However a stream is cut into calls, its outputs plus the flush, the first ``lag`` dropped, are bit for bit
    ``resample`` of the whole clip.  float32 samples, or int16 with ``pcm_scale`` (a stream may mix both).  numpy in -> the
    host-pointer calls, ROCm tensors in -> the device calls on the current stream.  The output feeds ``MfccStreamPool`` once the
    caller has buffered it to whole hops.  See ``ss_resample_stream_packed`` in ``include/speechsauce_amd.h``."""

    _what, _stem, _counter = "ResampleStreamPool", "resample", "periods_seen"
    _table, _noun = "sample_offsets", "samples"
    _whole_block = False  # a call counts the samples up to ``sample_offsets[-1]``, and launches nothing where that is 0

    def __init__(self, pool_streams, orig_rate, new_rate, lowpass_filter_width=6, rolloff=0.99):
        super().__init__(pool_streams)
        orig_rate, new_rate = _check_rates(orig_rate, new_rate, self._what)
        self._args = (orig_rate, new_rate, int(lowpass_filter_width), float(rolloff))
        rs = _get_resampler(*self._args)
        self.period_in, self.period_out, self.latency_periods = rs.info.o, rs.info.n, rs.info.latency_periods
        self.lag = self.latency_periods * self.period_out
        L = C.c_size_t()
        _lib.check(_lib.lib().ss_resample_stream_state_len(rs.handle, C.byref(L)))
        self.state_len = L.value

    @property
    def _period(self):
        return self.period_in

    def _count(self, diff):  # ``periods_seen`` counts periods, not samples
        return diff // self.period_in

    def _owner_for(self, x):  # the filter's tables live on one device: every device has its own handle
        return _get_resampler(*self._args, _device_key(x))

    def _out_shape(self, n):
        return (n // self.period_in * self.period_out,)

    def _flush_shape(self, n_active):
        return n_active, self.lag

    def push(self, samples, sample_offsets, slots, pcm_scale=None):
        x, scale = _require_signal(samples, (1,), self._what, pcm_scale)
        if scale is None:
            return self._run(x, sample_offsets, slots)
        return self._run(x, sample_offsets, slots, "_i16", (scale,))  # the PCM entry point takes the scale behind pool_streams

    __call__ = push

    def flush(self, slots):
        """The last ``lag`` outputs of the given streams, ``[len(slots), lag]`` (zeros where the stream's output time is negative);
        afterwards those streams are fresh.  Before the pool's first call there is no state anywhere: the outputs are zeros in a numpy
        array."""
        return self._flush(slots)


# ---- Kaldi-compatible fbank / MFCC front end (ss_kaldi_* in include/speechsauce_amd.h) ---------------------------

class KaldiConfig(_Handle):
    """Owns an ``ss_kaldi_config`` handle: the validated ``ss_kaldi_params``, the kernel's tables on the device that was current at
    creation and a device error word for the packed calls."""

    _destroy = "ss_kaldi_config_destroy"

    def __init__(self, params: SsKaldiParams):
        super().__init__()
        self.params = params
        _lib.check(self._owner.ss_kaldi_config_create(C.byref(params), C.byref(self._h)))

    def num_frames(self, n_samples: int) -> int:
        t = C.c_size_t()
        _lib.check(_lib.lib().ss_kaldi_num_frames(C.byref(self.params), n_samples, C.byref(t)))
        return t.value

    def device_status(self) -> None:
        """Raises SpeechSauceError (SS_ERR_DEVICE) if a packed launch on this handle has skipped an inconsistent clip since the last
        look.  Meaningful after the stream has been synchronised."""
        _lib.check(_lib.lib().ss_kaldi_config_device_status(self._h))


def _kaldi_params(sample_frequency, frame_length, frame_shift, num_mel_bins, num_ceps, low_freq, high_freq, preemphasis_coefficient,
                  cepstral_lifter, window_type, blackman_coeff, remove_dc_offset, use_power, use_energy, raw_energy, energy_floor,
                  input_scale) -> SsKaldiParams:
    if int(sample_frequency) != sample_frequency or int(sample_frequency) <= 0:
        raise ValueError(f"sample_frequency must be a positive integer number of Hz, got {sample_frequency!r}")
    if window_type not in _lib.KALDI_WINDOW:
        raise ValueError(f"window_type must be one of {sorted(_lib.KALDI_WINDOW)}, got {window_type!r}")
    p = SsKaldiParams()
    _lib.check(_lib.lib().ss_kaldi_params_default(C.byref(p), int(sample_frequency)))
    p.frame_length_ms, p.frame_shift_ms = float(frame_length), float(frame_shift)
    p.num_mel_bins, p.num_ceps = int(num_mel_bins), int(num_ceps)
    p.low_freq, p.high_freq = float(low_freq), float(high_freq)
    p.preemph_coef, p.cepstral_lifter = float(preemphasis_coefficient), float(cepstral_lifter)
    p.window_type, p.blackman_coeff = _lib.KALDI_WINDOW[window_type], float(blackman_coeff)
    p.remove_dc_offset, p.use_power, p.use_energy, p.raw_energy = int(bool(remove_dc_offset)), int(bool(use_power)), int(bool(use_energy)), int(bool(raw_energy))
    p.energy_floor, p.input_scale = float(energy_floor), float(input_scale)
    return p


@lru_cache(maxsize=32)
def _get_kaldi_config(key: tuple, device: int = -1) -> KaldiConfig:
    """Memoised handle factory, keyed like ``_get_resampler``: the parameters and the device the tables live on."""
    return KaldiConfig(_kaldi_params(*key))


_lib._on_switch.append(_get_kaldi_config.cache_clear)  # a handle belongs to the library that created it

# what torchaudio.compliance.kaldi takes and this front end does not serve; the value that changes nothing is accepted
_KALDI_NEUTRAL = {"dither": 0.0, "snip_edges": True, "htk_compat": False, "subtract_mean": False, "vtln_warp": 1.0}


def _kaldi_reject(what, unsupported):
    for k, v in unsupported.items():
        if k == "channel":
            raise ValueError(f"{what}: channel is not offered: pass the channel's samples (a 2-D input is a batch of clips)")
        if k in _KALDI_NEUTRAL or k.startswith("vtln_"):
            if k in _KALDI_NEUTRAL and v == _KALDI_NEUTRAL[k]:
                continue
            raise ValueError(f"{what}: {k}={v!r} is not offered by this front end (dither, snip_edges=False, htk_compat, subtract_mean "
                             "and VTLN are out of scope: see ss_kaldi_* in include/speechsauce_amd.h)")
        raise TypeError(f"{what}() got an unexpected keyword argument {k!r}")


def _kaldi_cfg(what, sig, mfcc, sample_frequency, frame_length, frame_shift, num_mel_bins, num_ceps, low_freq, high_freq,
               preemphasis_coefficient, cepstral_lifter, window_type, blackman_coeff, remove_dc_offset, use_power, use_energy, raw_energy,
               energy_floor, input_scale, unsupported) -> KaldiConfig:
    _kaldi_reject(what, unsupported)
    # the fbank calls put the energy column in place themselves: their handles are made with use_energy = 0 and no cepstra
    key = (sample_frequency, float(frame_length), float(frame_shift), int(num_mel_bins), int(num_ceps) if mfcc else 0, float(low_freq),
           float(high_freq), float(preemphasis_coefficient), float(cepstral_lifter) if mfcc else 0.0, window_type, float(blackman_coeff),
           bool(remove_dc_offset), bool(use_power), bool(use_energy) if mfcc else False, bool(raw_energy), float(energy_floor), float(input_scale))
    return _get_kaldi_config(key, _device_key(sig))


def _kaldi_dense(sig, cfg: KaldiConfig, mfcc: bool, with_energy: bool, scale=None):
    """sig [L] or [B, L] -> [T, cols] or [B, T, cols]; fbank with_energy: the log energy as column 0 (torchaudio's layout).
    scale: the signal is int16 PCM, sample = int16 * scale (the ``ss_kpcm_*`` entry points)"""
    lib = _lib.lib()
    fam, sc = ("ss_kaldi", []) if scale is None else ("ss_kpcm", [scale])
    one = len(sig.shape) == 1
    batch, L = (1, int(sig.shape[0])) if one else (int(sig.shape[0]), int(sig.shape[1]))
    T = cfg.num_frames(L)
    cols = cfg.params.num_ceps if mfcc else cfg.params.num_mel_bins
    if _is_torch(sig):
        import torch

        v = sig.reshape(1, L) if one else sig
        if v.stride(1) != 1:
            v = v.contiguous()
        ld = int(v.stride(0)) if batch > 1 else L
        if ld < L:
            v, ld = v.contiguous(), L
        out = torch.empty((batch, T, cols), dtype=torch.float32, device=v.device)
        en = torch.empty((batch, T), dtype=torch.float32, device=v.device) if with_energy else None
        if batch and mfcc:
            _launch(v.device, getattr(lib, f"{fam}_mfcc_device"), cfg.handle, v, batch, L, ld, *sc, out.data_ptr())
        elif batch:
            _launch(v.device, getattr(lib, f"{fam}_fbank_device"), cfg.handle, v, batch, L, ld, *sc, out.data_ptr(),
                    en.data_ptr() if with_energy else None)
        if with_energy:
            out = torch.cat([en.unsqueeze(-1), out], dim=-1)
        return out[0] if one else out
    v = np.ascontiguousarray(sig).reshape(batch, L)
    out = np.empty((batch, T, cols), dtype=np.float32)
    en = np.empty((batch, T), dtype=np.float32) if with_energy else None
    if batch:
        if mfcc:
            _lib.check(getattr(lib, f"{fam}_mfcc")(cfg.handle, v.ctypes.data, batch, L, L, *sc, out.ctypes.data))
        else:
            _lib.check(getattr(lib, f"{fam}_fbank")(cfg.handle, v.ctypes.data, batch, L, L, *sc, out.ctypes.data,
                                                    en.ctypes.data if with_energy else None))
    if with_energy:
        out = np.concatenate([en[..., None], out], axis=-1)
    return out[0] if one else out


def _kaldi_packed(sig, so, cfg: KaldiConfig, mfcc: bool, with_energy: bool, scale=None):
    """packed samples [N], sample offsets so (host int64, used as they stand) -> (rows [sum T_b, cols], frame offsets (host int64));
    scale: as for ``_kaldi_dense``"""
    lib = _lib.lib()
    fam, sc = ("ss_kaldi", []) if scale is None else ("ss_kpcm", [scale])
    n = so.size - 1
    fo = np.empty_like(so)
    _lib.check(lib.ss_kaldi_packed_frame_offsets(C.byref(cfg.params), n, so.ctypes.data, fo.ctypes.data))
    rows = int(fo[-1])
    cols = cfg.params.num_ceps if mfcc else cfg.params.num_mel_bins
    if _is_torch(sig):
        import torch

        x = sig.contiguous()
        out = torch.empty((rows, cols), dtype=torch.float32, device=x.device)
        en = torch.empty((rows,), dtype=torch.float32, device=x.device) if with_energy else None
        if n and rows and mfcc:
            _launch(x.device, getattr(lib, f"{fam}_mfcc_packed_device"), cfg.handle, x, n, so, *sc, fo, rows, out.data_ptr())
        elif n and rows:
            _launch(x.device, getattr(lib, f"{fam}_fbank_packed_device"), cfg.handle, x, n, so, *sc, fo, rows, out.data_ptr(),
                    en.data_ptr() if with_energy else None)
        if with_energy:
            out = torch.cat([en.unsqueeze(-1), out], dim=-1)
        return out, fo
    x = np.ascontiguousarray(sig)
    out = np.empty((rows, cols), dtype=np.float32)
    en = np.empty((rows,), dtype=np.float32) if with_energy else None
    if n and rows:
        if mfcc:
            _lib.check(getattr(lib, f"{fam}_mfcc_packed")(cfg.handle, x.ctypes.data, n, so.ctypes.data, *sc, out.ctypes.data))
        else:
            _lib.check(getattr(lib, f"{fam}_fbank_packed")(cfg.handle, x.ctypes.data, n, so.ctypes.data, *sc, out.ctypes.data,
                                                           en.ctypes.data if with_energy else None))
    if with_energy:
        out = np.concatenate([en[:, None], out], axis=-1)
    return out, fo


def kaldi_fbank(waveform, sample_frequency=16000.0, frame_length=25.0, frame_shift=10.0, num_mel_bins=23, low_freq=20.0, high_freq=0.0,
                preemphasis_coefficient=0.97, window_type="povey", blackman_coeff=0.42, remove_dc_offset=True, use_power=True,
                use_energy=False, raw_energy=True, energy_floor=1.0, input_scale=1.0, *, pcm_scale=None, **unsupported):
    """``torchaudio.compliance.kaldi.fbank`` (Kaldi's compute-fbank-feats) of one clip [L] -> [T, num_mel_bins] or of every row of a
    batch [B, L] -> [B, T, num_mel_bins], float32; the names and defaults are torchaudio's.  ``use_energy=True`` puts the log energy
    in column 0 ([.., num_mel_bins + 1]), as torchaudio does.  numpy in -> the host-pointer call; a ROCm tensor stays on the device
    (current stream, one launch).  ``input_scale``: every sample is multiplied by it first (32768 for normalised floats that stand
    for 16-bit PCM).  ``pcm_scale``: the waveform is int16 PCM and a sample is int16 * pcm_scale, a power of two (1.0: Kaldi's own
    integer-valued samples; 2**-15: torchaudio's normalised ones) -- the kernel converts on load, bit for bit the float call on the
    converted samples, and ``input_scale`` still applies afterwards.  Served for frames that pad to 512 points (256 < samples per frame <= 512); dither, snip_edges=False, htk_compat,
    subtract_mean, vtln_* and channel raise."""
    what = "kaldi_fbank"
    sig, scale = _require_signal(waveform, (1, 2), what, pcm_scale)
    cfg = _kaldi_cfg(what, sig, False, sample_frequency, frame_length, frame_shift, num_mel_bins, 0, low_freq, high_freq, preemphasis_coefficient,
                     0.0, window_type, blackman_coeff, remove_dc_offset, use_power, False, raw_energy, energy_floor, input_scale, unsupported)
    return _kaldi_dense(sig, cfg, False, bool(use_energy), scale)


def kaldi_mfcc(waveform, sample_frequency=16000.0, frame_length=25.0, frame_shift=10.0, num_mel_bins=23, low_freq=20.0, high_freq=0.0,
               preemphasis_coefficient=0.97, window_type="povey", blackman_coeff=0.42, remove_dc_offset=True, use_energy=False,
               raw_energy=True, energy_floor=1.0, input_scale=1.0, num_ceps=13, cepstral_lifter=22.0, *, pcm_scale=None, **unsupported):
    """``torchaudio.compliance.kaldi.mfcc`` (Kaldi's compute-mfcc-feats) of one clip [L] -> [T, num_ceps] or of a batch [B, L] ->
    [B, T, num_ceps]: the orthonormal DCT of ``kaldi_fbank``'s power-spectrum log-mel row with the cepstral lifter; ``use_energy=True``
    replaces coefficient 0 by the log energy.  See ``kaldi_fbank`` for the inputs and for what is not served."""
    what = "kaldi_mfcc"
    sig, scale = _require_signal(waveform, (1, 2), what, pcm_scale)
    cfg = _kaldi_cfg(what, sig, True, sample_frequency, frame_length, frame_shift, num_mel_bins, num_ceps, low_freq, high_freq,
                     preemphasis_coefficient, cepstral_lifter, window_type, blackman_coeff, remove_dc_offset, True, use_energy, raw_energy,
                     energy_floor, input_scale, unsupported)
    return _kaldi_dense(sig, cfg, True, False, scale)


def kaldi_fbank_packed(signal, lengths, sample_frequency=16000.0, frame_length=25.0, frame_shift=10.0, num_mel_bins=23, low_freq=20.0,
                       high_freq=0.0, preemphasis_coefficient=0.97, window_type="povey", blackman_coeff=0.42, remove_dc_offset=True,
                       use_power=True, use_energy=False, raw_energy=True, energy_floor=1.0, input_scale=1.0, *, pcm_scale=None,
                       **unsupported):
    """``kaldi_fbank`` of clips of different lengths packed end to end in one 1-D float32 signal -> (rows [sum T_b, cols],
    frame_offsets [n + 1] int64 on the host): clip b's rows are frame_offsets[b] : frame_offsets[b + 1], bit for bit what
    ``kaldi_fbank`` returns for that clip alone.  One launch for all clips.  ``(out, out_lengths)`` of ``resample_packed`` are valid
    ``(signal, lengths)`` as they stand.  ``pcm_scale``: the signal is int16 PCM (see ``kaldi_fbank``)."""
    what = "kaldi_fbank_packed"
    sig, scale = _require_signal(signal, (1,), what, pcm_scale)
    so = _sample_offsets(lengths, sig.shape[0], what)
    cfg = _kaldi_cfg(what, sig, False, sample_frequency, frame_length, frame_shift, num_mel_bins, 0, low_freq, high_freq, preemphasis_coefficient,
                     0.0, window_type, blackman_coeff, remove_dc_offset, use_power, False, raw_energy, energy_floor, input_scale, unsupported)
    return _kaldi_packed(sig, so, cfg, False, bool(use_energy), scale)


def kaldi_mfcc_packed(signal, lengths, sample_frequency=16000.0, frame_length=25.0, frame_shift=10.0, num_mel_bins=23, low_freq=20.0,
                      high_freq=0.0, preemphasis_coefficient=0.97, window_type="povey", blackman_coeff=0.42, remove_dc_offset=True,
                      use_energy=False, raw_energy=True, energy_floor=1.0, input_scale=1.0, num_ceps=13, cepstral_lifter=22.0, *,
                      pcm_scale=None, **unsupported):
    """``kaldi_mfcc`` of packed clips (see ``kaldi_fbank_packed``) -> (rows [sum T_b, num_ceps], frame_offsets [n + 1])."""
    what = "kaldi_mfcc_packed"
    sig, scale = _require_signal(signal, (1,), what, pcm_scale)
    so = _sample_offsets(lengths, sig.shape[0], what)
    cfg = _kaldi_cfg(what, sig, True, sample_frequency, frame_length, frame_shift, num_mel_bins, num_ceps, low_freq, high_freq,
                     preemphasis_coefficient, cepstral_lifter, window_type, blackman_coeff, remove_dc_offset, True, use_energy, raw_energy,
                     energy_floor, input_scale, unsupported)
    return _kaldi_packed(sig, so, cfg, True, False, scale)


# ---- the Kaldi front end over a pool of stream states (ss_kstream_*) ----------------------------------------------------------

class _FrontStreamPoolBase(_StreamPoolMixin):
    """What the pools of the handle-based front ends (``Kaldi*StreamPool``, ``NemoLogMelStreamPool``) share: they own their pool block
    and sizes themselves (no dense streaming base behind the mixin), zero rows in place, and take chunk lengths or sample offsets."""

    def reset(self, slots=None):
        """Zero the state of every stream of the pool, or of the given slots (fresh streams: their next ``delay_rows`` rows are
        warm-up rows again)."""
        if self._state is None:
            return
        if slots is None:
            self._state[...] = 0
        else:
            idx = list(np.atleast_1d(np.asarray(slots, dtype=np.int64)))
            if idx:
                self._state[idx] = 0

    def _lengths(self, lengths_or_offsets, n_slots):
        if lengths_or_offsets is None:
            return None
        v = np.asarray(lengths_or_offsets.cpu() if _is_torch(lengths_or_offsets) else lengths_or_offsets)
        if v.ndim != 1 or not (np.issubdtype(v.dtype, np.integer) or v.size == 0):
            raise TypeError(f"{self._what}: lengths_or_offsets must be a 1-D sequence of integers")
        v = v.astype(np.int64)
        if v.size == n_slots + 1:  # sample offsets
            if v[0] != 0:
                raise ValueError(f"{self._what}: sample offsets must start at 0")
            return np.diff(v)
        return v


class _KaldiStreamPoolBase(_FrontStreamPoolBase):
    """A pool of ``pool_streams`` live audio streams through ``kaldi_fbank`` / ``kaldi_mfcc``: the constructor takes torchaudio's
    keyword names (see ``kaldi_fbank``) plus ``pool_streams``; every stream carries its last ``state_len = delay_rows * hop`` samples,
    ``delay_rows = ceil(frame / hop) - 1``.  ``pool(chunks, lengths_or_offsets, slots, pcm_scale=None)``: ``chunks`` is one packed
    1-D float32 buffer (int16 with ``pcm_scale``, a power of two: sample = ``int16 * pcm_scale``) with the chunk lengths -- or the
    ``len(slots) + 1`` sample offsets -- of the entries, every chunk a whole number of hops (zero included), or a list of 1-D
    chunks with ``lengths_or_offsets=None``; ``slots`` names each chunk's pool row (distinct).  Returns ``(rows, row_offsets)``,
    the pair the ``CmvnStreamPool`` / ``AddDeltasStreamPool`` calls take with the same ``slots``.

    A stream's rows over all calls, however it was cut, are bit for bit ``kaldi_fbank`` / ``kaldi_mfcc`` of ``zeros(state_len) ++
    stream``: the first ``delay_rows`` rows after a reset are warm-up rows over the zero prefix, the rows after them are the offline
    call's on the stream itself.  numpy in -> the host-pointer call, ROCm tensors in -> the device call on the current stream.
    See ``ss_kstream_*`` in ``include/speechsauce_amd.h``."""

    _mfcc = False

    def __init__(self, pool_streams, kaldi_args, unsupported):
        what = self._what
        _kaldi_reject(what, unsupported)
        if int(pool_streams) < 1:
            raise ValueError(f"{what}: pool_streams must be at least 1")
        self.pool_streams = int(pool_streams)
        self._kaldi_args = kaldi_args
        self._params = _kaldi_params(*self._key())
        lib = _lib.lib()
        _lib.check(lib.ss_kaldi_params_validate(C.byref(self._params)))
        S, D, fl, sh, pad = (C.c_size_t() for _ in range(5))
        _lib.check(lib.ss_kaldi_sizes(C.byref(self._params), C.byref(fl), C.byref(sh), C.byref(pad)))
        _lib.check(lib.ss_kstream_state_len(C.byref(self._params), C.byref(S), C.byref(D)))
        self.state_len, self.delay_rows, self.hop = S.value, D.value, sh.value
        self._state = None
        self._where = None

    def _key(self):
        (sample_frequency, frame_length, frame_shift, num_mel_bins, num_ceps, low_freq, high_freq, preemphasis_coefficient, cepstral_lifter,
         window_type, blackman_coeff, remove_dc_offset, use_power, use_energy, raw_energy, energy_floor, input_scale) = self._kaldi_args
        mfcc = self._mfcc
        return (sample_frequency, float(frame_length), float(frame_shift), int(num_mel_bins), int(num_ceps) if mfcc else 0, float(low_freq),
                float(high_freq), float(preemphasis_coefficient), float(cepstral_lifter) if mfcc else 0.0, window_type, float(blackman_coeff),
                bool(remove_dc_offset), bool(use_power), bool(use_energy) if mfcc else False, bool(raw_energy), float(energy_floor),
                float(input_scale))

    def _config_for(self, packed):
        return _get_kaldi_config(self._key(), _device_key(packed))

    def _run(self, chunks, lengths_or_offsets, slots, pcm_scale, cols, with_energy):
        slot_list = [int(v) for v in slots]
        (packed, so, ro, sl, config), i16, scale = self._prepare_pcm(chunks, slot_list, self._lengths(lengths_or_offsets, len(slot_list)), pcm_scale)
        R = int(ro[-1])
        kind = "mfcc" if self._mfcc else "fbank"
        if _is_torch(packed):
            import torch

            outs = [torch.empty((R, cols), dtype=torch.float32, device=packed.device)]
            if not self._mfcc:
                outs.append(torch.empty((R,), dtype=torch.float32, device=packed.device))
        else:
            outs = [np.empty((R, cols), dtype=np.float32)]
            if not self._mfcc:
                outs.append(np.empty((R,), dtype=np.float32))
        self._call_pool(packed, so, ro, sl, config, outs, f"ss_kstream_{kind}_packed{i16}_device", f"ss_kstream_{kind}_packed{i16}", scale)
        if with_energy:
            return outs[0], outs[1], ro
        return outs[0], ro


class KaldiFbankStreamPool(_KaldiStreamPoolBase):
    """Ragged streaming ``kaldi_fbank``: ``pool(chunks, lengths_or_offsets, slots)`` -> ``(rows [total_rows, num_mel_bins],
    row_offsets)``; ``pool(..., with_energy=True)`` -> ``(rows, log_energy [total_rows], row_offsets)``."""

    _what = "KaldiFbankStreamPool"

    def __init__(self, pool_streams, sample_frequency=16000.0, frame_length=25.0, frame_shift=10.0, num_mel_bins=23, low_freq=20.0,
                 high_freq=0.0, preemphasis_coefficient=0.97, window_type="povey", blackman_coeff=0.42, remove_dc_offset=True,
                 use_power=True, raw_energy=True, energy_floor=1.0, input_scale=1.0, **unsupported):
        super().__init__(pool_streams, (sample_frequency, frame_length, frame_shift, num_mel_bins, 0, low_freq, high_freq,
                                        preemphasis_coefficient, 0.0, window_type, blackman_coeff, remove_dc_offset, use_power, False,
                                        raw_energy, energy_floor, input_scale), unsupported)
        self.cols = int(num_mel_bins)

    def __call__(self, chunks, lengths_or_offsets, slots, pcm_scale=None, with_energy=False):
        return self._run(chunks, lengths_or_offsets, slots, pcm_scale, self.cols, bool(with_energy))


class KaldiMfccStreamPool(_KaldiStreamPoolBase):
    """Ragged streaming ``kaldi_mfcc``: ``pool(chunks, lengths_or_offsets, slots)`` -> ``(rows [total_rows, num_ceps],
    row_offsets)``."""

    _what = "KaldiMfccStreamPool"
    _mfcc = True

    def __init__(self, pool_streams, sample_frequency=16000.0, frame_length=25.0, frame_shift=10.0, num_mel_bins=23, low_freq=20.0,
                 high_freq=0.0, preemphasis_coefficient=0.97, window_type="povey", blackman_coeff=0.42, remove_dc_offset=True,
                 use_energy=False, raw_energy=True, energy_floor=1.0, input_scale=1.0, num_ceps=13, cepstral_lifter=22.0, **unsupported):
        super().__init__(pool_streams, (sample_frequency, frame_length, frame_shift, num_mel_bins, num_ceps, low_freq, high_freq,
                                        preemphasis_coefficient, cepstral_lifter, window_type, blackman_coeff, remove_dc_offset, True,
                                        use_energy, raw_energy, energy_floor, input_scale), unsupported)
        self.cols = int(num_ceps)

    def __call__(self, chunks, lengths_or_offsets, slots, pcm_scale=None):
        return self._run(chunks, lengths_or_offsets, slots, pcm_scale, self.cols, False)


def _kaldi_list(what, signals, packed_fn, pcm_scale, kw):
    sigs = [_require_signal(x, (1,), what, pcm_scale)[0] for x in signals]
    if not sigs:
        return []
    on_device = [_is_torch(x) for x in sigs]
    if any(on_device) and not all(on_device):
        raise ValueError(f"{what}: the clips of one call must all be device tensors or all host arrays")
    if all(on_device):
        import torch

        if any(x.device != sigs[0].device for x in sigs):
            raise ValueError(f"{what}: the clips of one call must live on one device")
        packed = torch.cat(sigs)
    else:
        packed = np.concatenate(sigs)
    out, fo = packed_fn(packed, [int(x.shape[0]) for x in sigs], pcm_scale=pcm_scale, **kw)
    fo = fo.tolist()
    return [out[fo[b]:fo[b + 1]] for b in range(len(sigs))]


def kaldi_fbank_list(signals, *, pcm_scale=None, **kw):
    """A list of 1-D float32 clips of any lengths (int16 PCM with ``pcm_scale``) -> the list of their ``kaldi_fbank`` rows (views of one
    block): the clips are packed once and served by one ``kaldi_fbank_packed`` call, whose keyword arguments this takes."""
    return _kaldi_list("kaldi_fbank_list", signals, kaldi_fbank_packed, pcm_scale, kw)


def kaldi_mfcc_list(signals, *, pcm_scale=None, **kw):
    """``kaldi_fbank_list`` for ``kaldi_mfcc_packed``."""
    return _kaldi_list("kaldi_mfcc_list", signals, kaldi_mfcc_packed, pcm_scale, kw)


# ---- Whisper log-mel front end (ss_whisper_* in include/speechsauce_amd.h) ------------------------------------------

class WhisperConfig(_Handle):
    """Owns an ``ss_whisper_config`` handle: the tables and the per-clip keys on the device that was current at creation, a device
    error word for the packed calls, and the f32 scratch block that the 16-bit output types take (grown on demand, never inside a
    captured region: call once eagerly with the largest shape before capturing)."""

    _destroy = "ss_whisper_config_destroy"

    def __init__(self, n_mels: int):
        super().__init__()
        self.params = SsWhisperParams()
        _lib.check(self._owner.ss_whisper_params_default(C.byref(self.params), int(n_mels)))
        _lib.check(self._owner.ss_whisper_config_create(C.byref(self.params), C.byref(self._h)))
        self._work = None

    def work_bytes(self, batch: int, n_frames: int, code: int) -> int:
        n = C.c_size_t()
        _lib.check(_lib.lib().ss_whisper_work_bytes(C.byref(self.params), batch, n_frames, code, C.byref(n)))
        return n.value

    def work(self, batch: int, n_frames: int, code: int, device):
        """the cached scratch block as a device pointer (None for float32)"""
        need = self.work_bytes(batch, n_frames, code)
        if need == 0:
            return None
        import torch

        if self._work is None or self._work.numel() * 4 < need or self._work.device != device:
            self._work = torch.empty(((need + 3) // 4,), dtype=torch.float32, device=device)
        return self._work.data_ptr()

    def device_status(self) -> None:
        """Raises SpeechSauceError (SS_ERR_DEVICE) if a packed launch on this handle has met a bad table entry since the last look.
        Meaningful after the stream has been synchronised."""
        _lib.check(_lib.lib().ss_whisper_config_device_status(self._h))


@lru_cache(maxsize=8)
def _get_whisper_config(n_mels: int, device: int = -1) -> WhisperConfig:
    return WhisperConfig(n_mels)


_lib._on_switch.append(_get_whisper_config.cache_clear)


def whisper_num_frames(n_samples: int) -> int:
    """``n_samples // 160``: the frames Whisper keeps of a clip (no device needed)."""
    t = C.c_size_t()
    _lib.check(_lib.lib().ss_whisper_num_frames(int(n_samples), C.byref(t)))
    return t.value


def _whisper_frames(n_frames, longest: int, what: str) -> int:
    n = whisper_num_frames(longest) if n_frames is None else int(n_frames)
    if n < 2:
        raise ValueError(f"{what}: n_frames must be at least 2, got {n} (a clip of fewer than 320 samples needs an explicit n_frames)")
    return n


def _whisper_out(shape, name, device):
    """(the output block, its address); numpy has no bfloat16: a host bfloat16 result is a uint16 array of the bit patterns"""
    if device is not None:
        import torch

        out = torch.empty(shape, dtype=getattr(torch, name), device=device)
        return out, out.data_ptr()
    out = np.empty(shape, dtype={"float32": np.float32, "float16": np.float16, "bfloat16": np.uint16}[name])
    return out, out.ctypes.data


def whisper_log_mel(x, n_mels=80, n_frames=None, dtype="float32", *, pcm_scale=None):
    """The Whisper log-mel block (``whisper.audio.log_mel_spectrogram``, ``transformers.WhisperFeatureExtractor``) of one 16 kHz clip
    [L] -> [n_mels, n_frames] or of every row of a batch [B, L] -> [B, n_mels, n_frames].  ``n_frames=None`` keeps ``L // 160``
    frames; ``3000`` is the 30 s window (the clip is padded with zeros or trimmed).  ``dtype``: float32, float16 or bfloat16 (a host
    bfloat16 result is a uint16 array of bit patterns).  ``pcm_scale``: x is int16 PCM and a sample is int16 * pcm_scale, a power of
    two (2**-15: Whisper's own convention) -- the kernel converts on load, bit for bit the float call on the converted samples."""
    what = "whisper_log_mel"
    sig, scale = _require_signal(x, (1, 2), what, pcm_scale)
    i16, sc, zeros = ("", [], np.float32) if scale is None else ("_i16", [scale], np.int16)
    code, name = _pad_dtype(dtype, what)
    one = len(sig.shape) == 1
    batch, L = (1, int(sig.shape[0])) if one else (int(sig.shape[0]), int(sig.shape[1]))
    T = _whisper_frames(n_frames, L, what)
    cfg = _get_whisper_config(int(n_mels), _device_key(sig))
    M = cfg.params.n_mels
    lib = _lib.lib()
    if _is_torch(sig):
        import torch

        v = sig.reshape(1, L) if one else sig
        if L and v.stride(1) != 1:
            v = v.contiguous()
        ld = int(v.stride(0)) if batch > 1 and L else L
        if ld < L:
            v, ld = v.contiguous(), L
        out, optr = _whisper_out((batch, M, T), name, v.device)
        if batch:
            keep = v if L else torch.zeros(4, dtype=v.dtype, device=v.device)  # an empty clip reads nothing: any address will do
            _launch(v.device, getattr(lib, f"ss_whisper_log_mel{i16}_device"), cfg.handle, keep, batch, L, ld, *sc, T, code,
                    cfg.work(batch, T, code, v.device), optr)
        return out[0] if one else out
    v = np.ascontiguousarray(sig).reshape(batch, L)
    if L == 0:
        v = np.zeros((batch, 4), zeros)
    out, optr = _whisper_out((batch, M, T), name, None)
    if batch:
        _lib.check(getattr(lib, f"ss_whisper_log_mel{i16}")(cfg.handle, v.ctypes.data, batch, L, v.shape[1], *sc, T, code, optr))
    return out[0] if one else out


def whisper_log_mel_packed(signal, lengths, n_mels=80, n_frames=None, dtype="float32", *, pcm_scale=None):
    """Clips of different lengths end to end in ``signal`` [N] -> ``(out [n_clips, n_mels, n_frames], lengths int32 [n_clips])``: every
    clip padded or trimmed to the same ``n_frames`` (None: the longest clip's ``len // 160``), ``lengths[b] = min(len_b // 160,
    n_frames)`` the frames that come from the clip's own samples.  One call of three launches whatever the lengths.  ``pcm_scale``:
    the signal is int16 PCM (see ``whisper_log_mel``)."""
    what = "whisper_log_mel_packed"
    sig, scale = _require_signal(signal, (1,), what, pcm_scale)
    i16, sc, zeros = ("", [], np.float32) if scale is None else ("_i16", [scale], np.int16)
    code, name = _pad_dtype(dtype, what)
    so = _sample_offsets(lengths, int(sig.shape[0]), what)
    n = so.size - 1
    T = _whisper_frames(n_frames, int(np.diff(so).max()) if n else 320, what)
    cfg = _get_whisper_config(int(n_mels), _device_key(sig))
    M = cfg.params.n_mels
    lib = _lib.lib()
    if _is_torch(sig):
        import torch

        x = sig.contiguous()
        out, optr = _whisper_out((n, M, T), name, x.device)
        lens = torch.empty((n,), dtype=torch.int32, device=x.device)
        if n:
            keep = x if x.numel() else torch.zeros(4, dtype=x.dtype, device=x.device)
            _launch(x.device, getattr(lib, f"ss_whisper_log_mel_packed{i16}_device"), cfg.handle, keep, n, so, *sc, T, code,
                    cfg.work(n, T, code, x.device), optr, lens.data_ptr())
        return out, lens
    x = np.ascontiguousarray(sig)
    if x.size == 0:
        x = np.zeros(4, zeros)
    out, optr = _whisper_out((n, M, T), name, None)
    lens = np.empty((n,), dtype=np.int32)
    if n:
        _lib.check(getattr(lib, f"ss_whisper_log_mel_packed{i16}")(cfg.handle, x.ctypes.data, n, so.ctypes.data, *sc, T, code, optr,
                                                                   lens.ctypes.data))
    return out, lens


def whisper_log_mel_list(signals, n_mels=80, n_frames=None, dtype="float32", *, pcm_scale=None):
    """A list of 1-D float32 clips of any lengths (int16 PCM with ``pcm_scale``) -> ``(out [n_clips, n_mels, n_frames], lengths)``: the
    clips are packed once and served by one ``whisper_log_mel_packed`` call."""
    what = "whisper_log_mel_list"
    sigs = [_require_signal(x, (1,), what, pcm_scale)[0] for x in signals]
    if not sigs:
        raise ValueError(f"{what}: no clips")
    on_device = [_is_torch(x) for x in sigs]
    if any(on_device) and not all(on_device):
        raise ValueError(f"{what}: the clips of one call must all be device tensors or all host arrays")
    if all(on_device):
        import torch

        if any(x.device != sigs[0].device for x in sigs):
            raise ValueError(f"{what}: the clips of one call must live on one device")
        packed = torch.cat(sigs)
    else:
        packed = np.concatenate(sigs)
    return whisper_log_mel_packed(packed, [int(x.shape[0]) for x in sigs], n_mels=n_mels, n_frames=n_frames, dtype=dtype, pcm_scale=pcm_scale)


# ---- NeMo / Parakeet log-mel front end (ss_nemo_* in include/speechsauce_amd.h) ---------------------------------------

class NemoConfig(_Handle):
    """Owns an ``ss_nemo_config`` handle: the validated ``ss_nemo_params``, the kernel's tables on the device that was current at
    creation and a device error word for the packed calls."""

    _destroy = "ss_nemo_config_destroy"

    def __init__(self, params: SsNemoParams):
        super().__init__()
        self.params = params
        _lib.check(self._owner.ss_nemo_config_create(C.byref(params), C.byref(self._h)))

    def device_status(self) -> None:
        """Raises SpeechSauceError (SS_ERR_DEVICE) if a packed launch on this handle has skipped an inconsistent clip since the last
        look.  Meaningful after the stream has been synchronised."""
        _lib.check(_lib.lib().ss_nemo_config_device_status(self._h))


def _nemo_params(n_mels, normalize, win_length, preemph, log_guard, norm_eps) -> SsNemoParams:
    if normalize not in _lib.NEMO_NORMALIZE:
        raise ValueError(f"normalize must be 'per_feature' or None ('all_features' is not offered), got {normalize!r}")
    p = SsNemoParams()
    _lib.check(_lib.lib().ss_nemo_params_default(C.byref(p), int(n_mels)))
    p.win_length, p.normalize = int(win_length), _lib.NEMO_NORMALIZE[normalize]
    p.preemph, p.log_guard, p.norm_eps = float(preemph), float(log_guard), float(norm_eps)
    return p


@lru_cache(maxsize=16)
def _get_nemo_config(key: tuple, device: int = -1) -> NemoConfig:
    """Memoised handle factory, keyed like ``_get_kaldi_config``: the parameters and the device the tables live on."""
    return NemoConfig(_nemo_params(*key))


_lib._on_switch.append(_get_nemo_config.cache_clear)


def _nemo_cfg(sig, n_mels, normalize, win_length, preemph, log_guard, norm_eps) -> NemoConfig:
    key = (int(n_mels), normalize, int(win_length), float(preemph), float(log_guard), float(norm_eps))
    return _get_nemo_config(key, _device_key(sig))


def nemo_num_frames(n_samples: int) -> int:
    """``n_samples // 160``: the rows the NeMo front end keeps of a clip (the extractor's ``features_lengths``; no device needed)."""
    p, t = SsNemoParams(), C.c_size_t()
    _lib.check(_lib.lib().ss_nemo_params_default(C.byref(p), 80))
    _lib.check(_lib.lib().ss_nemo_num_frames(C.byref(p), int(n_samples), C.byref(t)))
    return t.value


def nemo_log_mel(x, n_mels=80, normalize="per_feature", win_length=400, preemph=0.97, log_guard=2.0 ** -24, norm_eps=1e-5):
    """The NeMo / Parakeet log-mel rows (NeMo's ``AudioToMelSpectrogramPreprocessor``, ``transformers.ParakeetFeatureExtractor``) of
    one 16 kHz float32 clip [L] -> [L // 160, n_mels] or of every row of a batch [B, L] -> [B, L // 160, n_mels]: whole-clip
    pre-emphasis, a ``win_length`` symmetric Hann window centred in 512-point frames at a 160-sample hop with zero padding, the power
    spectrum, ``n_mels`` (up to 128) Slaney mels, ``ln(. + log_guard)`` and -- ``normalize="per_feature"`` -- each band's mean and
    standard deviation (ddof = 1) over the clip's own rows taken out; ``normalize=None`` returns the log-mel rows.  numpy in -> the
    host-pointer call; a ROCm tensor stays on the device (current stream: one launch, two with the normalisation)."""
    what = "nemo_log_mel"
    sig = _require_f32(x, (1, 2), what)
    cfg = _nemo_cfg(sig, n_mels, normalize, win_length, preemph, log_guard, norm_eps)
    lib = _lib.lib()
    one = len(sig.shape) == 1
    batch, L = (1, int(sig.shape[0])) if one else (int(sig.shape[0]), int(sig.shape[1]))
    T, M = nemo_num_frames(L), cfg.params.n_mels
    if _is_torch(sig):
        import torch

        v = sig.reshape(1, L) if one else sig
        if L and v.stride(1) != 1:
            v = v.contiguous()
        ld = int(v.stride(0)) if batch > 1 and L else L
        if ld < L:
            v, ld = v.contiguous(), L
        out = torch.empty((batch, T, M), dtype=torch.float32, device=v.device)
        if batch and T:
            _launch(v.device, lib.ss_nemo_log_mel_device, cfg.handle, v, batch, L, ld, out.data_ptr())
        return out[0] if one else out
    v = np.ascontiguousarray(sig).reshape(batch, L)
    out = np.empty((batch, T, M), dtype=np.float32)
    if batch and T:
        _lib.check(lib.ss_nemo_log_mel(cfg.handle, v.ctypes.data, batch, L, L, out.ctypes.data))
    return out[0] if one else out


def nemo_log_mel_packed(signal, lengths, n_mels=80, normalize="per_feature", win_length=400, preemph=0.97, log_guard=2.0 ** -24,
                        norm_eps=1e-5, *, device_tables=None):
    """``nemo_log_mel`` of clips of different lengths packed end to end in one 1-D float32 signal -> (rows [sum T_b, n_mels],
    frame_offsets [n + 1] int64 on the host): clip b's rows are frame_offsets[b] : frame_offsets[b + 1], bit for bit what
    ``nemo_log_mel`` returns for that clip alone; a clip of fewer than 160 samples has none.  One call for all clips.  ``(out,
    out_lengths)`` of ``resample_packed`` are valid ``(signal, lengths)`` as they stand, and ``(rows, frame_offsets)`` go on to
    ``spec_augment_packed`` / ``pad_packed``.  ``device_tables=(sample_offsets, frame_offsets, total_frames)`` (with
    ``lengths=None``; int64 device tensors of n + 1 entries): the tables are used as they stand and nothing is read back or
    uploaded, so the call can be captured in a graph and replayed over changed tables -- the kernels skip a clip whose entries are
    inconsistent and ``NemoConfig.device_status()`` reports it; ``frame_offsets`` is then returned as it was given."""
    what = "nemo_log_mel_packed"
    sig = _require_f32(signal, (1,), what)
    if device_tables is not None and (lengths is not None or not (_is_torch(sig) and sig.is_cuda)):
        raise ValueError(f"{what}: device_tables go with lengths=None and a device signal")
    so = None if device_tables is not None else _sample_offsets(lengths, int(sig.shape[0]), what)
    cfg = _nemo_cfg(sig, n_mels, normalize, win_length, preemph, log_guard, norm_eps)
    lib, M = _lib.lib(), cfg.params.n_mels
    if device_tables is not None:
        import torch

        dso, dfo, rows = device_tables
        for t in (dso, dfo):
            if not (_is_torch(t) and t.is_cuda and t.dtype == torch.int64 and t.dim() == 1 and t.is_contiguous() and t.device == sig.device):
                raise TypeError(f"{what}: device_tables must be contiguous 1-D int64 tensors on the signal's device")
        if dso.numel() != dfo.numel() or dso.numel() < 1:
            raise ValueError(f"{what}: device_tables must both hold n_clips + 1 entries")
        n, rows = dso.numel() - 1, int(rows)
        x = sig.contiguous()
        out = torch.empty((rows, M), dtype=torch.float32, device=x.device)
        if n and rows:
            _launch(x.device, lib.ss_nemo_log_mel_packed_device, cfg.handle, x, n, dso, dfo, rows, out.data_ptr())
        return out, dfo
    n = so.size - 1
    fo = np.empty_like(so)
    _lib.check(lib.ss_nemo_packed_frame_offsets(C.byref(cfg.params), n, so.ctypes.data, fo.ctypes.data))
    rows = int(fo[-1])
    if _is_torch(sig):
        import torch

        x = sig.contiguous()
        out = torch.empty((rows, M), dtype=torch.float32, device=x.device)
        if n and rows:
            _launch(x.device, lib.ss_nemo_log_mel_packed_device, cfg.handle, x, n, so, fo, rows, out.data_ptr())
        return out, fo
    x = np.ascontiguousarray(sig)
    out = np.empty((rows, M), dtype=np.float32)
    if n and rows:
        _lib.check(lib.ss_nemo_log_mel_packed(cfg.handle, x.ctypes.data, n, so.ctypes.data, out.ctypes.data))
    return out, fo


def nemo_log_mel_list(signals, n_mels=80, normalize="per_feature", win_length=400, preemph=0.97, log_guard=2.0 ** -24, norm_eps=1e-5, *,
                      padded=False, layout="btc", dtype="float32", pad_value=0.0):
    """A list of 1-D float32 clips of any lengths -> the list of their ``nemo_log_mel`` rows (views of one block): the clips are
    packed once and served by one ``nemo_log_mel_packed`` call.  ``padded=True`` chains ``pad_packed`` and returns the model input
    ``(out, lengths)`` instead: ``[n, T_max, n_mels]`` (``layout="btc"``, the ``transformers`` models) or ``[n, n_mels, T_max]``
    (``"bct"``, NeMo's own) in ``dtype``."""
    what = "nemo_log_mel_list"
    sigs = [_require_f32(x, (1,), what) for x in signals]
    if not sigs:
        raise ValueError(f"{what}: no clips")
    on_device = [_is_torch(x) for x in sigs]
    if any(on_device) and not all(on_device):
        raise ValueError(f"{what}: the clips of one call must all be device tensors or all host arrays")
    if all(on_device):
        import torch

        if any(x.device != sigs[0].device for x in sigs):
            raise ValueError(f"{what}: the clips of one call must live on one device")
        packed = torch.cat(sigs)
    else:
        packed = np.concatenate(sigs)
    rows, fo = nemo_log_mel_packed(packed, [int(x.shape[0]) for x in sigs], n_mels, normalize, win_length, preemph, log_guard, norm_eps)
    if padded:
        return pad_packed(rows, fo, None, layout, dtype, pad_value)
    fo = fo.tolist()
    return [rows[fo[b]:fo[b + 1]] for b in range(len(sigs))]


class NemoLogMelStreamPool(_FrontStreamPoolBase):
    """A pool of ``pool_streams`` live audio streams through ``nemo_log_mel(..., normalize=None)``: the log-mel input of cache-aware
    FastConformer and the real-time Parakeet models, hop by hop.  Every stream carries its last ``state_len = delay_rows * 160 +
    win_length // 2 + 1`` samples, ``delay_rows = ceil(win_length / 320) - 1`` (1 for the default 400-sample window).
    ``pool(chunks, lengths_or_offsets, slots, pcm_scale=None)`` takes what ``KaldiFbankStreamPool`` takes -- one packed 1-D float32
    buffer (int16 with ``pcm_scale``, a power of two) with the chunk lengths or the ``len(slots) + 1`` sample offsets, every chunk a
    whole number of 160-sample hops (zero included), or a list of 1-D chunks with ``lengths_or_offsets=None`` -- and returns ``(rows
    [total_rows, n_mels], row_offsets)``, the pair ``CmvnStreamPool`` / ``SpliceStreamPool`` take with the same ``slots``.
    ``flush(slots)`` ends the named streams: ``[len(slots) * delay_rows, n_mels]``, stream ``i``'s last ``delay_rows`` rows at
    ``[i * delay_rows, (i + 1) * delay_rows)`` -- the frames that overhang the stream's end -- and the slots are fresh afterwards.

    The first ``delay_rows`` rows of a stream after a reset are warm-up rows (the rows of ``zeros(delay_rows * 160) ++ stream``);
    the rows after them, followed by the flush rows, are bit for bit ``nemo_log_mel(stream, normalize=None)``, however the stream
    was cut into calls.  A trailing partial hop is the caller's to hold back.  Per-feature normalisation needs a whole clip: chain
    ``CmvnStreamPool`` instead.  numpy in -> the host-pointer call, ROCm tensors in -> the device call on the current stream.  See
    ``ss_nstream_*`` in ``include/speechsauce_amd.h``."""

    _what = "NemoLogMelStreamPool"

    def __init__(self, pool_streams, n_mels=80, win_length=400, preemph=0.97, log_guard=2.0 ** -24):
        if int(pool_streams) < 1:
            raise ValueError(f"{self._what}: pool_streams must be at least 1")
        self.pool_streams = int(pool_streams)
        self._key = (int(n_mels), None, int(win_length), float(preemph), float(log_guard), 1e-5)
        self._params = _nemo_params(*self._key)
        lib = _lib.lib()
        _lib.check(lib.ss_nemo_params_validate(C.byref(self._params)))
        S, L = C.c_size_t(), C.c_size_t()
        _lib.check(lib.ss_nstream_state_len(C.byref(self._params), C.byref(S), C.byref(L)))
        self.state_len, self.delay_rows, self.hop, self.cols = S.value, L.value, int(self._params.hop_length), int(n_mels)
        self._state = None
        self._where = None

    def _config_for(self, packed):
        return _get_nemo_config(self._key, _device_key(packed))

    def __call__(self, chunks, lengths_or_offsets, slots, pcm_scale=None):
        slot_list = [int(v) for v in slots]
        (packed, so, ro, sl, config), i16, scale = self._prepare_pcm(chunks, slot_list, self._lengths(lengths_or_offsets, len(slot_list)), pcm_scale)
        R = int(ro[-1])
        if _is_torch(packed):
            import torch

            out = torch.empty((R, self.cols), dtype=torch.float32, device=packed.device)
        else:
            out = np.empty((R, self.cols), dtype=np.float32)
        self._call_pool(packed, so, ro, sl, config, [out], f"ss_nstream_log_mel_packed{i16}_device", f"ss_nstream_log_mel_packed{i16}", scale)
        return out, ro

    def flush(self, slots):
        """The last ``delay_rows`` rows of every named stream -> ``[len(slots) * delay_rows, n_mels]``; the slots are fresh
        afterwards.  Before the first ``pool`` call every stream is fresh: the rows are those of silence, on the host."""
        sl = np.asarray(_pool_slots(slots, self.pool_streams, self._what), dtype=np.int32)
        n, lib = sl.size, _lib.lib()
        if self._state is None:  # nothing was pushed yet: the flush of fresh streams, served by a host pool of zeros
            self._state = np.zeros((self.pool_streams, self.state_len), dtype=np.float32)
            self._where = ("host",)
        if _is_torch(self._state):
            import torch

            out = torch.empty((n * self.delay_rows, self.cols), dtype=torch.float32, device=self._state.device)
            if n:
                _launch(self._state.device, lib.ss_nstream_flush_device, self._config_for(self._state).handle, n, sl, self.pool_streams,
                        self._state.data_ptr(), out.data_ptr())
        else:
            out = np.empty((n * self.delay_rows, self.cols), dtype=np.float32)
            if n:
                _lib.check(lib.ss_nstream_flush(self._config_for(self._state).handle, n, sl.ctypes.data, self.pool_streams,
                                                self._state.ctypes.data, out.ctypes.data))
        return out
