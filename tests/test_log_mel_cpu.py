"""The log-mel calls (ss_log_mel_spectrogram*), the part that needs no device: the eight entry points exist in the product library
beside an unchanged ABI number, their argument checks come before anything touches a device, and the Python front's wrappers apply
power_to_db's argument rules and mel_spectrogram_packed's offsets."""
import ctypes as C

import numpy as np
import pytest

ENTRY_POINTS = [
    "ss_log_mel_spectrogram",
    "ss_log_mel_spectrogram_device",
    "ss_log_mel_spectrogram_i16",
    "ss_log_mel_spectrogram_i16_device",
    "ss_log_mel_spectrogram_packed",
    "ss_log_mel_spectrogram_packed_device",
    "ss_log_mel_spectrogram_packed_i16",
    "ss_log_mel_spectrogram_packed_i16_device",
]
SS_ERR_ARG = 3


def test_the_eight_entry_points_resolve_and_the_abi_number_stays(sslib):
    from speechsauce_amd import _lib

    raw = C.CDLL(_lib.LIB_PATH)  # the product library's own symbol table, not the prototypes of the Python front
    for name in ENTRY_POINTS:
        assert hasattr(raw, name), name
        assert name in _lib.PROTOTYPES, name
    assert sslib.ss_abi_version() == 7


def test_header_says_how_the_floor_differs_from_power_to_db(sslib):
    import os

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = " ".join(open(os.path.join(root, "include", "speechsauce_amd.h")).read().split())
    assert "PER CLIP" in text and "ONE maximum over the whole block" in text
    import speechsauce_amd as ss

    assert "one maximum over the whole block" in " ".join(ss.log_mel_spectrogram.__doc__.split())


def test_null_config_and_null_buffers_are_argument_errors(sslib):
    x = np.zeros(4096, dtype=np.float32)
    xi = np.zeros(4096, dtype=np.int16)
    out = np.zeros(128 * 8, dtype=np.float32)
    so = np.array([0, 4096], dtype=np.int64)
    db = (1.0, 1e-10, 80.0)
    s = 2.0 ** -15
    # a null config, whatever else is passed
    assert sslib.ss_log_mel_spectrogram(None, x.ctypes.data, 1, 4096, *db, out.ctypes.data) == SS_ERR_ARG
    assert sslib.ss_log_mel_spectrogram_device(None, x.ctypes.data, 1, 4096, 4096, *db, out.ctypes.data, None) == SS_ERR_ARG
    assert sslib.ss_log_mel_spectrogram_i16(None, xi.ctypes.data, 1, 4096, s, *db, out.ctypes.data) == SS_ERR_ARG
    assert sslib.ss_log_mel_spectrogram_i16_device(None, xi.ctypes.data, 1, 4096, 4096, s, *db, out.ctypes.data, None) == SS_ERR_ARG
    assert sslib.ss_log_mel_spectrogram_packed(None, x.ctypes.data, 1, so.ctypes.data, *db, out.ctypes.data) == SS_ERR_ARG
    assert sslib.ss_log_mel_spectrogram_packed_device(None, x.ctypes.data, 1, so.ctypes.data, so.ctypes.data, 8, *db, out.ctypes.data,
                                                      None) == SS_ERR_ARG
    assert sslib.ss_log_mel_spectrogram_packed_i16(None, xi.ctypes.data, 1, so.ctypes.data, s, *db, out.ctypes.data) == SS_ERR_ARG
    assert sslib.ss_log_mel_spectrogram_packed_i16_device(None, xi.ctypes.data, 1, so.ctypes.data, s, so.ctypes.data, 8, *db,
                                                          out.ctypes.data, None) == SS_ERR_ARG
    # null buffers and a null config
    assert sslib.ss_log_mel_spectrogram(None, None, 1, 4096, *db, None) == SS_ERR_ARG
    assert sslib.ss_log_mel_spectrogram_packed(None, None, 1, None, *db, None) == SS_ERR_ARG
    # amin <= 0 and a NaN ref are argument errors before anything else is looked at
    for bad in ((1.0, 0.0, 80.0), (1.0, -1.0, 80.0), (float("nan"), 1e-10, 80.0)):
        assert sslib.ss_log_mel_spectrogram_device(None, None, 0, 0, 0, *bad, None, None) == SS_ERR_ARG
        assert sslib.ss_log_mel_spectrogram_packed_device(None, None, 0, None, None, 0, *bad, None, None) == SS_ERR_ARG
    assert b"amin" in sslib.ss_last_error_string() or b"ref" in sslib.ss_last_error_string()


def test_python_wrappers_raise_before_touching_a_device(sslib):
    import speechsauce_amd as ss

    x = np.zeros(16000, dtype=np.float32)
    for fn, args in ((ss.log_mel_spectrogram, (x, 16000)), (ss.log_mel_spectrogram_packed, (x, [8000, 8000], 16000)),
                     (ss.log_mel_spectrogram_list, ([x[:8000], x[8000:]], 16000))):
        with pytest.raises(ValueError):
            fn(*args, top_db=-1.0)
        with pytest.raises(ValueError):
            fn(*args, amin=0.0)
        with pytest.raises(ValueError):
            fn(*args, ref=float("nan"))
        with pytest.raises(TypeError):
            fn(*args, pcm_scale=2.0 ** -15)  # pcm_scale with a float signal
    with pytest.raises(TypeError):
        ss.log_mel_spectrogram(x.astype(np.float64), 16000)
    with pytest.raises(TypeError):
        ss.log_mel_spectrogram_packed(x.astype(np.float64), [8000, 8000], 16000)
    with pytest.raises(TypeError):
        ss.log_mel_spectrogram(x.astype(np.int16), 16000)  # int16 without pcm_scale
    with pytest.raises(ValueError):
        ss.log_mel_spectrogram_packed(x, [16000, 1], 16000)  # more samples than the buffer holds
    assert ss.log_mel_spectrogram_list([], 16000) == []
    for name in ("log_mel_spectrogram", "log_mel_spectrogram_packed", "log_mel_spectrogram_list"):
        assert name in ss.__all__


def test_packed_form_uses_the_mel_calls_row_offsets(sslib):
    """log_mel_spectrogram_packed hands the ABI, and returns, the row offsets of mel_spectrogram_packed's offset helper, and its call
    is the mel call's with ref, amin, top_db in front of the output pointer.  Checked without a device: the front runs on a stand-in
    library that records the packed calls and passes the offset helper through."""
    import speechsauce_amd as ss
    from speechsauce_amd import _lib

    cfg = ss.SpeechConfig.__new__(ss.SpeechConfig)  # (no handle: the offsets need only the parameters)
    cfg.params = _lib.make_params(fft_points=2048, frame_length=0.032, frame_stride=0.032, num_filters=128, high_frequency=8000.0)
    cfg._h = None
    lens = [700, 2048, 5000, 16000, 16500]
    so = ss._sample_offsets(lens, sum(lens), "t")
    want = ss._row_offsets(cfg, so)
    assert np.diff(want).tolist() == [2, 4, 10, 32, 33]
    calls = []

    class Recorder:
        ss_packed_row_offsets = sslib.ss_packed_row_offsets

        def __getattr__(self, name):
            return lambda *a: calls.append((name, a)) or 0

    x = np.zeros(sum(lens), dtype=np.float32)
    with _lib.use_library(Recorder()):
        out_m, ro_m = ss._internal_stft_packed(x, so, cfg, False)
        out_l, ro_l = ss._internal_stft_packed(x, so, cfg, False, None, [1.0, 1e-10, 80.0])
    assert np.array_equal(ro_m, want) and np.array_equal(ro_l, want)
    assert out_m.shape == out_l.shape == (128 * int(want[-1]),)
    assert [c[0] for c in calls] == ["ss_mel_spectrogram_packed", "ss_log_mel_spectrogram_packed"]
    mel_args, log_args = calls[0][1], calls[1][1]
    assert log_args[:4] == mel_args[:4] and log_args[4:7] == (1.0, 1e-10, 80.0) and len(log_args) == len(mel_args) + 3
