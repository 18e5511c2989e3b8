"""Host side of the resampler (ss_resample_* in include/speechsauce_amd.h): no device anywhere in this file.

The specification is restated here in numpy f64 -- `ref_filter` and `ref_resample` are the header's formula, not a call into the
library -- and the library's host-only helpers, argument rules and table checks are held to it.  tests/test_resample.py imports
the restatement for the GPU side."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "speechsauce_amd.h")

SS_OK, SS_ERR_ARG, SS_ERR_HIP, SS_ERR_UNSUPPORTED = 0, 3, 4, 5


# ---- the specification, restated ----
def ref_filter(orig_rate, new_rate, lpw=6, rolloff=0.99):
    """-> o, n, width, h [n x (2 width + o)] f64 (exact zeros outside |t| < lpw), inside [n x (2 width + o)] bool"""
    g = math.gcd(orig_rate, new_rate)
    o, n = orig_rate // g, new_rate // g
    base = min(o, n) * rolloff
    width = math.ceil(lpw * o / base)
    k = np.arange(2 * width + o)
    i = np.arange(n)
    t = (-i[:, None] / n + (k[None, :] - width) / o) * base
    inside = np.abs(t) < lpw
    with np.errstate(invalid="ignore", divide="ignore"):
        sinc = np.where(t == 0, 1.0, np.sin(np.pi * t) / (np.pi * t))
    h = np.where(inside, sinc * np.cos(np.pi * t / (2 * lpw)) ** 2 * (base / o), 0.0)
    return o, n, width, h, inside


def ref_sizes(orig_rate, new_rate, lpw=6, rolloff=0.99):
    o, n, width, h, inside = ref_filter(orig_rate, new_rate, lpw, rolloff)
    first = inside.argmax(axis=1)
    count = inside.sum(axis=1)
    assert all(inside[i, first[i]:first[i] + count[i]].all() for i in range(n))  # one contiguous run per phase
    lookback = int((width - first).max())
    lookahead = int((first + count - 1 - width).max())
    return dict(o=o, n=n, width=width, taps=int(count.max()), lookback=lookback, lookahead=lookahead, D=-(-(lookahead + 1) // o),
                first=first.astype(np.int32), count=count.astype(np.int32))


def ref_out_len(o, n, L):
    return -(-n * L // o)


def ref_resample(x, orig_rate, new_rate, lpw=6, rolloff=0.99):
    """out[j n + i] = sum_k h[i][k] x[j o + k - width], x outside the clip = 0, ceil(n L / o) outputs; all f64"""
    o, n, width, h, _ = ref_filter(orig_rate, new_rate, lpw, rolloff)
    x = np.asarray(x, np.float64)
    L = x.shape[0]
    periods = -(-L // o) if L else 0
    xp = np.concatenate([np.zeros(width), x, np.zeros(periods * o - L + width + o)])
    win = np.lib.stride_tricks.sliding_window_view(xp, 2 * width + o)[::o][:periods]  # [periods x K]
    out = win @ h.T  # [periods x n]
    return out.reshape(-1)[:ref_out_len(o, n, L)]


# the issue's table: conversion -> o, n, width, taps, lookahead, D
TABLE = {
    (48000, 16000): (3, 1, 19, 37, 18, 7),
    (44100, 16000): (441, 160, 17, 34, 454, 2),
    (8000, 16000): (1, 2, 7, 13, 6, 7),
    (16000, 8000): (2, 1, 13, 25, 12, 7),
    (44100, 48000): (147, 160, 7, 13, 152, 2),
    (11025, 16000): (441, 640, 7, 13, None, None),
    (44100, 8000): (441, 80, 34, 67, None, None),
    (7, 5): (7, 5, 9, 17, 14, 3),
}


def _info(sslib, orig, new, lpw=6, rolloff=0.99):
    from speechsauce_amd._lib import SsResampleInfo

    info = SsResampleInfo()
    rc = sslib.ss_resample_sizes(orig, new, lpw, rolloff, C.byref(info))
    return rc, info


def test_restatement_reproduces_the_table():
    for (orig, new), (o, n, width, taps, lookahead, D) in TABLE.items():
        s = ref_sizes(orig, new)
        assert (s["o"], s["n"], s["width"], s["taps"]) == (o, n, width, taps), (orig, new)
        if lookahead is not None:
            assert (s["lookahead"], s["D"]) == (lookahead, D), (orig, new)
    # table sizes the issue names: the compact table of 44.1k -> 16k is 21.3 KB, of 11.025k -> 16k 32.5 KB
    assert 160 * 34 * 4 == 21760 and 640 * 13 * 4 == 33280


@pytest.mark.parametrize("rates", sorted(TABLE))
def test_sizes_match_the_table_and_the_restatement(sslib, rates):
    orig, new = rates
    o, n, width, taps, lookahead, D = TABLE[rates]
    rc, info = _info(sslib, orig, new)
    assert rc == SS_OK, sslib.ss_last_error_string()
    assert (info.o, info.n, info.width, info.taps) == (o, n, width, taps)
    if lookahead is not None:
        assert (info.lookahead, info.latency_periods) == (lookahead, D)
    s = ref_sizes(orig, new)
    assert (info.lookback, info.lookahead, info.latency_periods) == (s["lookback"], s["lookahead"], s["D"])
    assert info.tile_outputs >= n and info.tile_outputs % n == 0


@pytest.mark.parametrize("rates", sorted(TABLE) + [(16000, 44100), (3, 2)])
def test_taps_equal_the_restatement_rounded_to_f32(sslib, rates):
    orig, new = rates
    s = ref_sizes(orig, new)
    o, n, width, h64, inside = ref_filter(orig, new)
    taps = s["taps"]
    h = np.full((n, taps), np.nan, np.float32)
    first = np.full(n, -1, np.int32)
    count = np.full(n, -1, np.int32)
    assert sslib.ss_resample_taps(orig, new, 6, 0.99, h.ctypes.data, first.ctypes.data, count.ctypes.data) == SS_OK
    np.testing.assert_array_equal(first, s["first"])
    np.testing.assert_array_equal(count, s["count"])
    for i in range(n):
        want = h64[i, first[i]:first[i] + count[i]].astype(np.float32)
        ulp = np.spacing(np.abs(want).max())  # 1 ulp of f32 at the row's largest tap: libm sin / cos differences
        assert np.abs(h[i, :count[i]].astype(np.float64) - want.astype(np.float64)).max() <= ulp, (rates, i)
        assert (h[i, count[i]:] == 0.0).all() and not np.signbit(h[i, count[i]:]).any()  # the padding: exactly +0.0
    # the f64 table is exactly 0.0 outside the runs (torchaudio's own holds ~1e-50 there)
    assert (h64[~inside] == 0.0).all()
    # first / count may be NULL
    h2 = np.empty_like(h)
    assert sslib.ss_resample_taps(orig, new, 6, 0.99, h2.ctypes.data, None, None) == SS_OK
    np.testing.assert_array_equal(h2.view(np.int32), h.view(np.int32))


def test_other_widths_and_rolloffs(sslib):
    for lpw, rolloff in ((1, 0.99), (16, 0.9475937167399596), (6, 1.0), (3, 0.5)):
        rc, info = _info(sslib, 48000, 32000, lpw, rolloff)
        assert rc == SS_OK
        # rolloff crosses the ABI as a float and is read back as its seven-digit decimal
        r7 = float("%.7g" % np.float32(rolloff))
        s = ref_sizes(48000, 32000, lpw, r7)
        assert (info.o, info.n, info.width, info.taps, info.lookback, info.lookahead, info.latency_periods) == \
            (s["o"], s["n"], s["width"], s["taps"], s["lookback"], s["lookahead"], s["D"]), (lpw, rolloff)
    assert float("%.7g" % np.float32(0.99)) == 0.99


@pytest.mark.parametrize("rates", [(48000, 16000), (44100, 16000), (8000, 16000), (7, 5)])
def test_len_and_packed_offsets(sslib, rates):
    orig, new = rates
    o, n = TABLE[rates][:2]
    lens = [0, 1, o - 1, o, o + 1, 5 * o + 2]
    for L in lens:
        got = C.c_size_t(12345)
        assert sslib.ss_resample_len(orig, new, L, C.byref(got)) == SS_OK
        assert got.value == ref_out_len(o, n, L) == math.ceil(n * L / o), (rates, L)
    so = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    oo = np.full_like(so, -1)
    assert sslib.ss_resample_packed_offsets(orig, new, len(lens), so.ctypes.data, oo.ctypes.data) == SS_OK
    np.testing.assert_array_equal(np.diff(oo), [ref_out_len(o, n, L) for L in lens])
    assert oo[0] == 0
    bad = so.copy()
    bad[3] = bad[2] - 1
    assert sslib.ss_resample_packed_offsets(orig, new, len(lens), bad.ctypes.data, oo.ctypes.data) == SS_ERR_ARG
    assert b"clip 2" in sslib.ss_last_error_string()
    bad = so.copy()
    bad[0] = 1
    assert sslib.ss_resample_packed_offsets(orig, new, len(lens), bad.ctypes.data, oo.ctypes.data) == SS_ERR_ARG


def test_argument_and_support_rules(sslib):
    from speechsauce_amd._lib import SsResampleInfo

    info = SsResampleInfo()
    h = C.c_void_p()

    def both(orig, new, lpw, rolloff):
        a = sslib.ss_resample_sizes(orig, new, lpw, rolloff, C.byref(info))
        b = sslib.ss_resampler_create(orig, new, lpw, rolloff, C.byref(h))
        assert a == b and (b != SS_OK) == (not h.value)
        if h.value:
            sslib.ss_resampler_destroy(h)
        return a

    for args in ((0, 16000, 6, 0.99), (16000, 0, 6, 0.99),      # a rate of 0
                 (16000, 16000, 6, 0.99),                         # equal rates
                 (48000, 16000, 0, 0.99), (48000, 16000, 65, 0.99),   # lpw outside 1 .. 64
                 (48000, 16000, 6, 0.0), (48000, 16000, 6, -0.5), (48000, 16000, 6, 1.0001), (48000, 16000, 6, float("nan")),
                 (1025, 1, 6, 0.99), (1, 1025, 6, 0.99), (2050, 4, 6, 0.99)):   # o or n above 1024
        assert both(*args) == SS_ERR_ARG, args
        assert sslib.ss_last_error_string() != b""
    assert both(48000, 16000, 1, 1.0) == SS_OK and both(48000, 16000, 64, 0.99) != SS_ERR_ARG
    assert both(2048, 4, 6, 0.99) == SS_ERR_UNSUPPORTED      # o = 512 is legal; 512 / 1: far more than 256 taps
    # taps > 256: 48 / 1 has a run of about 2 * 6 * 48 / 0.99 taps
    assert ref_sizes(48000, 1000)["taps"] > 256
    assert both(48000, 1000, 6, 0.99) == SS_ERR_UNSUPPORTED and b"taps" in sslib.ss_last_error_string()
    assert both(48000, 16000, 6, 1e-6) == SS_ERR_UNSUPPORTED   # (decided without forming the table)
    # the compact table: 1023 -> 1024 needs 1024 x 13 floats = 53248 bytes > 40960; 11.025k -> 16k (33280 bytes) is supported
    s = ref_sizes(1023, 1024)
    assert s["taps"] <= 256 and s["n"] * s["taps"] * 4 > 40960
    assert both(1023, 1024, 6, 0.99) == SS_ERR_UNSUPPORTED and b"table" in sslib.ss_last_error_string()
    for rates in TABLE:
        assert both(*rates, 6, 0.99) == SS_OK, rates
    # null outputs
    assert sslib.ss_resample_sizes(48000, 16000, 6, 0.99, None) == SS_ERR_ARG
    assert sslib.ss_resampler_create(48000, 16000, 6, 0.99, None) == SS_ERR_ARG
    assert sslib.ss_resample_len(48000, 16000, 5, None) == SS_ERR_ARG
    assert sslib.ss_resample_len(0, 16000, 5, C.byref(C.c_size_t())) == SS_ERR_ARG
    sslib.ss_resampler_destroy(None)  # a no-op


@pytest.fixture()
def handle(sslib):
    h = C.c_void_p()
    assert sslib.ss_resampler_create(44100, 16000, 6, 0.99, C.byref(h)) == SS_OK
    yield h
    sslib.ss_resampler_destroy(h)


def test_handle_reports_its_sizes_without_a_device(sslib, handle):
    from speechsauce_amd._lib import SsResampleInfo

    info = SsResampleInfo()
    assert sslib.ss_resampler_info(handle, C.byref(info)) == SS_OK
    assert (info.o, info.n, info.taps, info.latency_periods) == (441, 160, 34, 2)
    n = C.c_size_t()
    assert sslib.ss_resample_stream_state_len(handle, C.byref(n)) == SS_OK
    assert n.value == info.latency_periods * info.o + info.lookback + 1
    assert sslib.ss_resample_stream_state_len(None, C.byref(n)) == SS_ERR_ARG


def test_calls_decided_before_the_device(sslib, handle):
    """n_clips == 0 / batch == 0 / n_active == 0 are SS_OK without a device; argument and table errors come back before any device
    is touched (this file runs without one) and the host forms name the first bad clip or entry."""
    x = np.zeros(4410, np.float32)
    pcm = np.zeros(4410, np.int16)
    out = np.full(1700, 7.0, np.float32)
    so = np.array([0, 441, 441, 4410], np.int64)
    oo = np.array([0, 160, 160, 1600], np.int64)
    p = lambda a: a.ctypes.data  # noqa: E731
    # nothing to do
    assert sslib.ss_resample(handle, p(x), 0, 4410, 4410, p(out), 1600) == SS_OK
    assert sslib.ss_resample_device(handle, p(x), 0, 4410, 4410, p(out), 1600, None) == SS_OK
    assert sslib.ss_resample_packed(handle, p(x), 0, p(so), p(oo), p(out)) == SS_OK
    assert sslib.ss_resample_packed_device(handle, p(x), 0, p(so), p(oo), 4410, 1600, p(out), None) == SS_OK
    assert sslib.ss_resample_packed_i16(handle, p(pcm), 0, p(so), 2.0 ** -15, p(oo), p(out)) == SS_OK
    pool = np.zeros((4, 2 * 441 + 17 + 1), np.float32)
    slots = np.array([0, 1, 2], np.int32)
    assert sslib.ss_resample_stream_packed(handle, p(x), 0, p(so), p(slots), 4, p(pool), p(out)) == SS_OK
    assert sslib.ss_resample_stream_packed_device(handle, p(x), 0, p(so), 4410, p(slots), 4, p(pool), p(out), None) == SS_OK
    assert sslib.ss_resample_stream_flush(handle, 0, p(slots), 4, p(pool), p(out)) == SS_OK
    assert sslib.ss_resample_stream_flush_device(handle, 0, p(slots), 4, p(pool), p(out), None) == SS_OK
    assert (out == 7.0).all() and not pool.any()
    # dense argument rules
    assert sslib.ss_resample(None, p(x), 1, 4410, 4410, p(out), 1600) == SS_ERR_ARG
    assert sslib.ss_resample(handle, None, 1, 4410, 4410, p(out), 1600) == SS_ERR_ARG
    assert sslib.ss_resample(handle, p(x), 1, 4410, 4409, p(out), 1600) == SS_ERR_ARG        # ld < n_samples
    assert sslib.ss_resample(handle, p(x), 1, 4410, 4410, p(out), 1599) == SS_ERR_ARG        # ld_out < out_len
    assert sslib.ss_resample(handle, p(x), 1, 4410, 4410, p(x), 1600) == SS_ERR_ARG          # in place
    assert sslib.ss_resample(handle, p(x), 1, 2 ** 31, 2 ** 31, p(out), 2 ** 31) == SS_ERR_ARG
    for scale in (0.0, 3.0, -1.0, float("nan"), 2.0 ** 65):
        assert sslib.ss_resample_i16(handle, p(pcm), 1, 4410, 4410, scale, p(out), 1600) == SS_ERR_ARG
        assert b"power of two" in sslib.ss_last_error_string()
        assert sslib.ss_resample_packed_i16(handle, p(pcm), 3, p(so), scale, p(oo), p(out)) == SS_ERR_ARG
        assert sslib.ss_resample_stream_packed_i16(handle, p(pcm), 3, p(so), p(slots), 4, scale, p(pool), p(out)) == SS_ERR_ARG
    # packed host form: the tables are checked first and the first bad clip is named
    for bad_so, bad_oo, word in ((np.array([0, 441, 440, 4410]), oo, b"clip 1"),            # reversed
                                 (np.array([1, 441, 441, 4410]), oo, b"sample_offsets[0]"),
                                 (so, np.array([0, 160, 160, 1601]), b"clip 2"),              # an output span of the wrong length
                                 (so, np.array([0, 161, 161, 1601]), b"clip 0"),
                                 (so, np.array([2, 162, 162, 1602]), b"out_offsets[0]")):
        bad_so, bad_oo = np.ascontiguousarray(bad_so, np.int64), np.ascontiguousarray(bad_oo, np.int64)
        assert sslib.ss_resample_packed(handle, p(x), 3, p(bad_so), p(bad_oo), p(out)) == SS_ERR_ARG
        assert word in sslib.ss_last_error_string(), sslib.ss_last_error_string()
        assert sslib.ss_resample_packed_i16(handle, p(pcm), 3, p(bad_so), 1.0, p(bad_oo), p(out)) == SS_ERR_ARG
    assert sslib.ss_resample_packed(handle, p(x), 3, None, p(oo), p(out)) == SS_ERR_ARG
    empty = np.zeros(4, np.int64)
    assert sslib.ss_resample_packed(handle, p(x), 3, p(empty), p(empty), p(out)) == SS_OK     # empty clips only: nothing moves
    # pool host forms: entries of whole periods, slots inside the pool and named once
    for bad_so, bad_slots, word in ((np.array([0, 441, 440, 882]), slots, b"entry 1"),
                                    (np.array([0, 441, 882, 1324]), slots, b"entry 2"),        # 442 samples: not whole periods
                                    (np.array([1, 442, 883, 1324]), slots, b"sample_offsets[0]"),
                                    (np.array([0, 441, 882, 1323]), np.array([0, 4, 2], np.int32), b"entry 1"),
                                    (np.array([0, 441, 882, 1323]), np.array([0, 2, 2], np.int32), b"named twice")):
        bad_so = np.ascontiguousarray(bad_so, np.int64)
        assert sslib.ss_resample_stream_packed(handle, p(x), 3, p(bad_so), p(bad_slots), 4, p(pool), p(out)) == SS_ERR_ARG
        assert word in sslib.ss_last_error_string(), sslib.ss_last_error_string()
    assert sslib.ss_resample_stream_flush(handle, 2, p(np.array([1, 1], np.int32)), 4, p(pool), p(out)) == SS_ERR_ARG
    assert sslib.ss_resample_stream_flush(handle, 2, p(np.array([1, 9], np.int32)), 4, p(pool), p(out)) == SS_ERR_ARG
    assert sslib.ss_resample_stream_packed(handle, p(x), 3, p(so), p(slots), 0, p(pool), p(out)) == SS_ERR_ARG   # a pool without rows
    assert sslib.ss_resample_stream_packed(handle, p(x), 3, p(empty), p(slots), 4, p(pool), p(out)) == SS_OK      # empty entries only
    assert sslib.ss_resample_stream_packed(handle, p(x), 3, p(np.array([0, 441, 882, 1323], np.int64)), p(slots), 4, p(x), p(out)) == SS_ERR_ARG  # pool == x
    assert (out == 7.0).all() and not pool.any()


def _has_gpu():
    try:
        import torch

        return torch.cuda.is_available()
    except Exception:
        return False


@pytest.mark.skipif(_has_gpu(), reason="checks the no-device failure mode")
def test_valid_calls_fail_loudly_without_a_device(sslib, handle):
    import speechsauce_amd as ss

    x = np.zeros(4410, np.float32)
    out = np.zeros(1600, np.float32)
    assert sslib.ss_resample(handle, x.ctypes.data, 1, 4410, 4410, out.ctypes.data, 1600) == SS_ERR_HIP
    assert b"no CPU fallback" in sslib.ss_last_error_string()
    with pytest.raises(ss.SpeechSauceError) as e:
        ss.resample(x, 44100, 16000)
    assert e.value.status == SS_ERR_HIP


def test_python_front_rules():
    import speechsauce_amd as ss

    x = np.arange(10, dtype=np.float32)
    assert ss.resample(x, 16000, 16000) is x                       # equal rates: the input, unchanged (torchaudio does the same)
    out, lens = ss.resample_packed(x, [4, 6], 8000, 8000)
    assert out is x and lens.tolist() == [4, 6]
    assert ss.resample_list([], 48000, 16000) == []
    with pytest.raises(TypeError):
        ss.resample(x.astype(np.float64), 48000, 16000)
    with pytest.raises(TypeError):
        ss.resample(x, 48000, 16000, pcm_scale=2.0 ** -15)          # with pcm_scale the signal must be int16
    with pytest.raises(ValueError):
        ss.resample(x.astype(np.int16), 48000, 16000, pcm_scale=3.0)
    with pytest.raises(ValueError):
        ss.resample(np.zeros((2, 2, 8), np.float32), 48000, 16000)
    with pytest.raises(ValueError):
        ss.resample(x, 48000.5, 16000)
    with pytest.raises(ss.SpeechSauceError) as e:
        ss.resample(x, 48000, 1000)
    assert e.value.status == SS_ERR_UNSUPPORTED
    pool = ss.ResampleStreamPool(8, 44100, 16000)
    assert (pool.period_in, pool.period_out, pool.latency_periods, pool.lag) == (441, 160, 2, 320)
    assert pool.state is None and pool.flush([1, 2]).shape == (2, 320) and not pool.flush([3]).any()
    with pytest.raises(ValueError):
        pool.push(np.zeros(442, np.float32), [0, 442], [0])          # not whole periods
    with pytest.raises(ValueError):
        pool.push(np.zeros(441, np.float32), [0, 441], [8])
    assert {"resample", "resample_packed", "resample_list", "ResampleStreamPool"} <= set(ss.__all__)
    assert ss._get_resampler(48000, 16000) is ss._get_resampler(48000, 16000)   # the handle is memoised


def test_prototypes_follow_the_header(sslib):
    from speechsauce_amd import _lib

    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    decl = dict(re.findall(r"^\s*(?:int|void)\s+(ss_resampl\w+)\s*\(([^;]*?)\)\s*;", text, flags=re.S | re.M))
    assert len(decl) == 22
    for name, args in decl.items():
        assert name in _lib.PROTOTYPES and hasattr(sslib, name), name
        res, argtypes = _lib.PROTOTYPES[name]
        assert len(argtypes) == len([a for a in args.split(",") if a.strip()]), name
        assert res is (None if name == "ss_resampler_destroy" else C.c_int)
        kinds = ["float" if re.match(r"float\s+\w+$", a.strip()) else "other" for a in args.split(",")]
        assert [i for i, k in enumerate(kinds) if k == "float"] == [i for i, t in enumerate(argtypes) if t is C.c_float], name
    assert sslib.ss_abi_version() == 7
    assert re.search(r"#define SS_ABI_VERSION 7\b", open(HEADER).read())


def test_convention_tones_through_the_restatement():
    """Pins the convention without torchaudio, on the restatement itself: 48 kHz -> 16 kHz has one phase, so away from the clip's ends
    a tone of frequency f comes out as the same tone at the new rate times G(f) = sum_k h[k] exp(2 pi i f (k - width) / 48000).
    A 1 kHz tone (well inside the passband) therefore misses the ideal 1 kHz tone at 16 kHz by at most |G - 1|, and a 12 kHz tone
    (above the new Nyquist of 8 kHz) comes out no larger than |G|: both bounds are read off the restatement's own frequency response
    here, and the stop-band gain lies below the pass-band gain."""
    orig, new = 48000, 16000
    o, n, width, h, _ = ref_filter(orig, new)
    assert (o, n) == (3, 1)
    k = np.arange(h.shape[1]) - width

    def gain(f):
        return np.sum(h[0] * np.exp(2j * np.pi * f * k / orig))

    L = 4800
    s = np.arange(L)
    j = np.arange(ref_out_len(o, n, L))
    inner = (j * o - width >= 0) & (j * o + width + o <= L)          # every tap inside the clip
    assert inner.sum() > 1000

    def slack(f):  # f64 rounding: the sums themselves, and the tones' arguments (up to 2 pi f L / orig, each rounded) on both sides
        return (64 + 4 * np.pi * f * L / orig) * np.finfo(np.float64).eps * max(1.0, np.abs(h[0]).sum())

    f_pass, f_stop = 1000.0, 12000.0
    y = ref_resample(np.cos(2 * np.pi * f_pass * s / orig), orig, new)
    assert np.abs(y[inner] - np.cos(2 * np.pi * f_pass * j[inner] / new)).max() <= abs(gain(f_pass) - 1) + slack(f_pass)
    z = ref_resample(np.cos(2 * np.pi * f_stop * s / orig), orig, new)
    assert np.abs(z[inner]).max() <= abs(gain(f_stop)) + slack(f_stop)
    assert abs(gain(f_stop)) < abs(gain(f_pass)) and abs(gain(f_pass) - 1) < abs(gain(f_stop) - 1)
    # and the unattenuated stop-band tone would have aliased to 4 kHz at full size: the filter is what removes it
    assert np.abs(z[inner]).max() < np.abs(y[inner]).max()
