"""Time-axis delta features (Kaldi's add-deltas): ss_add_deltas_packed (host pointers) and its *_device form on packed clips,
ss_add_deltas_stream_state_len / ss_add_deltas_stream_packed* / ss_add_deltas_stream_flush* over a pool of stream states, and the
Python front's add_deltas, add_deltas_packed and AddDeltasStreamPool.

The reference crate differences along the feature axis only, so the yardstick is `restate` below: a numpy restatement of the
definition in include/speechsauce_amd.h, written in the definition's order -- per order o an f64 accumulator that starts at +0.0
and takes double(k[j]) * double(x[clamp(t + j)]) for j ascending, zero taps skipped, then float(acc * (1.0 / D_o)).  Every product
is exact in f64 (|k| <= 2992 < 2^12 times a 24-bit significand), so the additions are the only roundings and they happen in the same
order in the kernel: the GPU tests compare BIT FOR BIT.  `StreamModel` restates the pool calls (2L rows of history, latency L) on
the same arithmetic.
"""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

from common import RTOL, rel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"ss_add_deltas_packed_device": 9, "ss_add_deltas_packed": 8, "ss_add_deltas_stream_state_len": 4,
         "ss_add_deltas_stream_packed_device": 12, "ss_add_deltas_stream_packed": 10, "ss_add_deltas_stream_flush_device": 9,
         "ss_add_deltas_stream_flush": 8}
COLS = (1, 13, 33, 80)                                # 33 crosses a 32-column tile
OW = ((1, 2), (2, 2), (2, 1), (1, 9), (2, 16))        # (order, window): lags 2, 4, 2, 9, 32
LONG = 5000                                           # rows: crosses row tiles and the shared-clip split
STREAM_ROWS = 128                                     # an entry that sees more rows than this (history + new) leaves the LDS path


# ---------------------------------------------------------------- the restatement ----------------------------------------------

def taps(order, window):
    """-> (k [2 * order * window + 1] int64, D): k(o) = k(o-1) * [-window .. window], D = (2 sum n^2)^order."""
    base = np.arange(-window, window + 1, dtype=np.int64)
    k = np.array([1], dtype=np.int64)
    for _ in range(order):
        k = np.convolve(k, base)
    return k, (2 * sum(n * n for n in range(1, window + 1))) ** order


def _delta_f64(buf, centres, last, o, window):
    """acc * inv of d_o, before the rounding to float32, of the rows `centres` (indices into buf [N, C] float32, all >= 0), the row
    index clamped to 0 .. last."""
    k, D = taps(o, window)
    half = o * window
    inv = 1.0 / float(D)
    b64 = buf.astype(np.float64)
    centres = np.asarray(centres, dtype=np.int64)
    acc = np.zeros((len(centres), buf.shape[1]), dtype=np.float64)  # +0.0
    with np.errstate(invalid="ignore", over="ignore"):
        for j in range(-half, half + 1):
            if k[j + half] == 0:
                continue
            acc = acc + float(k[j + half]) * b64[np.clip(centres + j, 0, last)]
        return acc * inv


def _delta_at(buf, centres, last, o, window):
    with np.errstate(invalid="ignore", over="ignore"):
        return _delta_f64(buf, centres, last, o, window).astype(np.float32)


def restate(x, order, window):
    """The definition on ONE clip: x [T, C] float32 -> [T, (order + 1) * C] float32."""
    x = np.asarray(x, dtype=np.float32)
    T = x.shape[0]
    if T == 0:
        return np.zeros((0, (order + 1) * x.shape[1]), np.float32)
    t = np.arange(T)
    return np.concatenate([x] + [_delta_at(x, t, T - 1, o, window) for o in range(1, order + 1)], axis=1)


class StreamModel:
    """The pool calls on one stream: the last 2L raw rows are kept, output row k of a push is the row of stream time seen + k - L."""

    def __init__(self, cols, order, window):
        self.cols, self.order, self.window, self.L = cols, order, window, order * window
        self.hist = np.zeros((0, cols), np.float32)

    def _rows(self, buf, centres, last):
        out = np.zeros((len(centres), (self.order + 1) * self.cols), np.float32)
        centres = np.asarray(centres, dtype=np.int64)
        ok = centres >= 0
        if ok.any():
            c = centres[ok]
            out[ok] = np.concatenate([buf[c]] + [_delta_at(buf, c, last, o, self.window) for o in range(1, self.order + 1)], axis=1)
        return out

    def push(self, new):
        count = len(self.hist)
        if len(new) == 0:
            return np.zeros((0, (self.order + 1) * self.cols), np.float32)
        buf = np.concatenate([self.hist, new])
        # with count < 2L buf[0] is stream row 0 (the left clamp is the definition's); with count == 2L no tap reaches below buf[0]
        out = self._rows(buf, count + np.arange(len(new)) - self.L, len(buf) - 1)
        self.hist = buf[max(len(buf) - 2 * self.L, 0):]
        return out

    def flush(self):
        count = len(self.hist)
        buf = self.hist if count else np.zeros((1, self.cols), np.float32)
        out = self._rows(buf, count + np.arange(self.L) - self.L if count else np.full(self.L, -1), max(count - 1, 0))
        self.hist = np.zeros((0, self.cols), np.float32)
        return out


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


@functools.lru_cache(maxsize=None)
def _clip(cols, T, seed=0):
    """Seeded rows [T, cols], float32; never modified."""
    x = (np.random.default_rng(1000 * cols + seed).standard_normal((T, cols)) * 3 + 1).astype(np.float32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def _want(cols, T, order, window, seed=0):
    w = restate(_clip(cols, T, seed), order, window)
    w.setflags(write=False)
    return w


# ---------------------------------------------------------------- CPU ---------------------------------------------------------

def test_symbols_are_declared_exported_and_prototyped(sslib):
    from speechsauce_amd import _lib

    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "speechsauce_amd.h")).read(), flags=re.S)
    for name, arity in NAMES.items():
        assert re.search(r"^int %s\(" % name, header, flags=re.M), name
        assert name in _lib.PROTOTYPES, name
        fn = getattr(sslib, name)
        assert fn.restype is C.c_int and len(fn.argtypes) == len(_lib.PROTOTYPES[name][1]) == arity, name
    assert sslib.ss_abi_version() == 7  # entry points only: the version stays
    shim = open(os.path.join(ROOT, "mfcc-rust_amd", "rust-shim", "src", "lib.rs")).read()
    for fn in ("try_add_deltas_packed", "try_add_deltas_stream_state_len", "try_add_deltas_stream_packed", "try_add_deltas_stream_flush"):
        assert "pub fn %s(" % fn in shim, fn
    assert "inline std::vector<float> add_deltas_packed(" in open(os.path.join(ROOT, "include", "speechsauce_amd.hpp")).read()


def _state_len(sslib, cols, order, window):
    L = C.c_size_t(12345)
    return sslib.ss_add_deltas_stream_state_len(cols, order, window, C.byref(L)), L.value


def test_state_len_formula_and_rejections(sslib):
    for cols in COLS:
        for order, window in OW:
            assert _state_len(sslib, cols, order, window) == (0, 2 * order * window * cols + 1)
    assert _state_len(sslib, 13, 1, 32) == (0, 64 * 13 + 1) and _state_len(sslib, 13, 2, 16) == (0, 64 * 13 + 1)  # L = 32: the largest
    for bad in ((0, 2, 2), (13, 2, 0), (13, 0, 2), (13, 3, 2), (13, 1, 33), (13, 2, 17), (13, 2, 1 << 40)):
        assert _state_len(sslib, *bad) == (3, 12345), bad  # SS_ERR_ARG, the output untouched
    assert _state_len(sslib, 1 << 25, 2, 16)[0] == 3                                   # 2^31 + 1 floats
    assert _state_len(sslib, (1 << 25) - 1, 2, 16) == (0, 64 * ((1 << 25) - 1) + 1)    # just below
    assert _state_len(sslib, 1 << 31, 1, 1)[0] == 3
    assert sslib.ss_add_deltas_stream_state_len(13, 2, 2, None) == 3


def test_argument_errors_are_decided_before_the_device_is_touched(sslib):
    """Every call here is rejected (or has nothing to do) on the host: none of the pointers is ever handed to the device, so host
    arrays stand in for device buffers.  On a host without a device a call that got past its checks would return SS_ERR_HIP."""
    cols, order, window, rows, P = 13, 2, 2, 6, 4
    L = order * window
    len_ = 2 * L * cols + 1
    vec = np.ones((rows, cols), np.float32)
    out = np.full((max(rows, 2 * L), 3 * cols), -5.0, np.float32)  # also large enough for a flush of two entries
    pool = np.full((P, len_), -7.0, np.float32)
    off = np.array([0, 2, 6], np.int64)
    sl = np.array([1, 3], np.int32)
    v, o, p, r, s = vec.ctypes.data, out.ctypes.data, pool.ctypes.data, off.ctypes.data, sl.ctypes.data

    def packed_dev(vec=v, n=2, off=r, total=rows, cols=cols, order=order, window=window, out=o):
        return sslib.ss_add_deltas_packed_device(vec, n, off, total, cols, order, window, out, None)

    def packed_host(vec=v, n=2, off=r, total=rows, cols=cols, order=order, window=window, out=o):
        return sslib.ss_add_deltas_packed(vec, n, off, total, cols, order, window, out)

    def stream_dev(vec=v, n=2, ro=r, total=rows, sl=s, P=P, cols=cols, order=order, window=window, pool=p, out=o):
        return sslib.ss_add_deltas_stream_packed_device(vec, n, ro, total, sl, P, cols, order, window, pool, out, None)

    def stream_host(vec=v, n=2, ro=r, sl=s, P=P, cols=cols, order=order, window=window, pool=p, out=o):
        return sslib.ss_add_deltas_stream_packed(vec, n, ro, sl, P, cols, order, window, pool, out)

    def flush_dev(n=2, sl=s, P=P, cols=cols, order=order, window=window, pool=p, out=o):
        return sslib.ss_add_deltas_stream_flush_device(n, sl, P, cols, order, window, pool, out, None)

    def flush_host(n=2, sl=s, P=P, cols=cols, order=order, window=window, pool=p, out=o):
        return sslib.ss_add_deltas_stream_flush(n, sl, P, cols, order, window, pool, out)

    # an empty call is SS_OK with nothing launched, also without a device and whatever else is passed
    for call in (packed_dev, packed_host, stream_dev, stream_host, flush_dev, flush_host):
        assert call(n=0) == 0, call.__name__
    assert sslib.ss_add_deltas_packed_device(None, 0, None, 0, 0, 0, 0, None, None) == 0
    assert sslib.ss_add_deltas_packed(None, 0, None, 0, 0, 0, 0, None) == 0
    assert sslib.ss_add_deltas_stream_packed_device(None, 0, None, 0, None, 0, 0, 0, 0, None, None, None) == 0
    assert sslib.ss_add_deltas_stream_packed(None, 0, None, None, 0, 0, 0, 0, None, None) == 0
    assert sslib.ss_add_deltas_stream_flush_device(0, None, 0, 0, 0, 0, None, None, None) == 0
    assert sslib.ss_add_deltas_stream_flush(0, None, 0, 0, 0, 0, None, None) == 0
    # the scalars every call shares
    for call in (packed_dev, packed_host, stream_dev, stream_host, flush_dev, flush_host):
        what = call.__name__
        assert call(cols=0) == 3, what
        assert call(order=0) == 3 and call(order=3) == 3, what
        assert b"order" in sslib.ss_last_error_string()
        assert call(window=0) == 3 and call(order=1, window=33) == 3 and call(order=2, window=17) == 3, what
        assert call(n=1 << 31) == 3 and call(cols=1 << 31) == 3, what
        assert call(out=None) == 3, what
    for call in (packed_dev, packed_host):
        for name in ("vec", "off", "out"):
            assert call(**{name: None}) == 3, (call.__name__, name)
        assert call(total=1 << 31) == 3
        assert call(out=v) == 3 and b"in place" in sslib.ss_last_error_string()  # out must not overlap vec
        assert call(out=v + 4 * (rows * cols - 1)) == 3                         # ... not even in its last float
        assert call(out=v - 4 * (3 * rows * cols - 1)) == 3                     # out is (order + 1) times as long as vec
    for call in (stream_dev, stream_host):
        for name in ("vec", "ro", "sl", "pool", "out"):
            assert call(**{name: None}) == 3, (call.__name__, name)
        assert call(P=0) == 3 and call(P=1 << 31) == 3
        assert call(cols=1 << 25, order=2, window=16) == 3  # the state length reaches 2^31
        assert call(out=v) == 3 and call(out=v + 4 * cols) == 3
        assert call(pool=v) == 3 and call(pool=o) == 3 and call(pool=o + 4 * (3 * rows * cols - 1)) == 3  # the pool overlapping vec / out
    assert stream_dev(total=1 << 31) == 3
    for call in (flush_dev, flush_host):
        for name in ("sl", "pool", "out"):
            assert call(**{name: None}) == 3, (call.__name__, name)
        assert call(P=0) == 3 and call(P=1 << 31) == 3
        assert call(pool=o) == 3 and call(pool=o + 4 * (2 * L * 3 * cols - 1)) == 3  # the pool overlapping the 2 * L rows of out
    # the host forms' table errors name the first bad clip / entry
    for bad, where in (([1, 2, 6], b"clip 0"), ([0, 4, 3], b"clip 1"), ([0, 2, 7], b"clip 1")):
        b = np.array(bad, np.int64)
        assert packed_host(off=b.ctypes.data) == 3 and where in sslib.ss_last_error_string(), bad
    for bad, where in (([1, 2, 6], b"entry 0"), ([0, 4, 3], b"entry 1")):
        b = np.array(bad, np.int64)
        assert stream_host(ro=b.ctypes.data) == 3 and where in sslib.ss_last_error_string(), bad
    for call in (stream_host, flush_host):
        for bad, where in (([1, 4], b"entry 1"), ([-1, 3], b"entry 0"), ([3, 3], b"entry 1")):
            b = np.array(bad, np.int32)
            assert call(sl=b.ctypes.data) == 3 and where in sslib.ss_last_error_string(), (call.__name__, bad)
            assert (b"outside the pool" if bad[0] != bad[1] else b"named twice") in sslib.ss_last_error_string()
    # clips / entries without rows only: nothing to do, no device needed
    z = np.zeros(3, np.int64)
    assert packed_host(off=z.ctypes.data) == 0 and stream_host(ro=z.ctypes.data) == 0
    assert packed_dev(total=0) == 0 and stream_dev(total=0) == 0
    assert (out == -5.0).all() and (pool == -7.0).all() and (vec == 1.0).all()  # nothing was written by any of it


def _has_gpu():
    try:
        import torch

        return torch.cuda.is_available()
    except Exception:
        return False


@pytest.mark.skipif(_has_gpu(), reason="checks the no-device failure mode")
def test_python_front_fails_loudly_without_a_device(sslib):
    import speechsauce_amd as ss
    from speechsauce_amd import SpeechSauceError

    x = np.zeros((5, 13), np.float32)
    for call in (lambda: ss.add_deltas(x), lambda: ss.add_deltas_packed(x, [0, 2, 5])):
        with pytest.raises(SpeechSauceError) as e:
            call()
        assert e.value.status == 4  # SS_ERR_HIP: there is no CPU path
    m = ss.AddDeltasStreamPool(4, 13)
    with pytest.raises(SpeechSauceError) as e:
        m(x[:3], [0, 2, 3], [2, 0])
    assert e.value.status == 4
    assert m.state is None and not m.rows_seen.any()  # rows_seen moves only after a call went through


def test_python_argument_rules(sslib):
    import speechsauce_amd as ss

    for name in ("add_deltas", "add_deltas_packed", "AddDeltasStreamPool"):
        assert name in ss.__all__ and hasattr(ss, name)
    z = lambda r, c=13, dt=np.float32: np.zeros((r, c), dt)  # noqa: E731
    for bad in (dict(order=0), dict(order=3), dict(window=0), dict(order=2, window=17), dict(order=1, window=33)):
        with pytest.raises(ValueError):
            ss.add_deltas(z(4), **bad)
        with pytest.raises(ValueError):
            ss.add_deltas_packed(z(4), [0, 4], **bad)
        with pytest.raises(ValueError):
            ss.AddDeltasStreamPool(4, 13, **bad)
    with pytest.raises(TypeError):
        ss.add_deltas(z(4, dt=np.float64))
    with pytest.raises(ValueError):
        ss.add_deltas(np.zeros(13, np.float32))  # not a matrix
    with pytest.raises(TypeError):
        ss.add_deltas_packed(z(4, dt=np.float64), [0, 4])
    for bad_off in ([1, 4], [0, 3, 2], [0, 5]):
        with pytest.raises(ValueError):
            ss.add_deltas_packed(z(4), bad_off)
    with pytest.raises(TypeError):
        ss.add_deltas_packed(z(4), np.array([0.0, 4.0]))
    # no clip has a row: nothing for the device to do
    got = ss.add_deltas_packed(z(0), [0, 0, 0])
    assert got.shape == (0, 39) and got.dtype == np.float32
    assert ss.add_deltas(z(0), order=1).shape == (0, 26)

    m = ss.AddDeltasStreamPool(4, 13)
    assert (m.pool_streams, m.cols, m.order, m.window, m.lag, m.state_len) == (4, 13, 2, 2, 4, 8 * 13 + 1)
    assert m.state is None and m.rows_seen.dtype == np.int64 and m.rows_seen.shape == (4,) and not m.rows_seen.any()
    assert ss.AddDeltasStreamPool(2, 40, order=1, window=9).lag == 9
    with pytest.raises(TypeError):
        m(z(3, dt=np.float64), [0, 3], [0])  # wrong dtype
    with pytest.raises(ValueError):
        m(np.zeros(39, np.float32), [0, 3], [0])  # not 2-D
    with pytest.raises(ValueError):
        m(z(3, 12), [0, 3], [0])  # wrong number of columns
    with pytest.raises(ValueError):
        m(z(3), [0, 2, 3], [0])  # table length
    with pytest.raises(ValueError):
        m(z(3), [0, 3], [4])  # a slot outside the pool
    with pytest.raises(ValueError):
        m(z(3), [0, 3], [-1])
    with pytest.raises(ValueError):
        m(z(3), [0, 2, 3], [1, 1])  # a slot named twice
    with pytest.raises(ValueError):
        m(z(3), [1, 3], [0])  # ro[0] != 0
    with pytest.raises(ValueError):
        m(z(3), [0, 2, 1], [0, 1])  # a decreasing pair
    with pytest.raises(ValueError):
        m(z(3), [0, 4], [0])  # past the block
    with pytest.raises(TypeError):
        m(z(3), np.array([0.0, 3.0]), [0])  # a float table
    with pytest.raises(ValueError):
        m.flush([4])
    with pytest.raises(ValueError):
        m.flush([1, 1])
    with pytest.raises(ValueError):
        m.reset(slots=[7])
    assert m.state is None and not m.rows_seen.any()  # nothing was created or counted by the rejected calls
    m.reset()
    m.reset(slots=[1])  # no state yet: nothing to do
    f = m.flush([2, 0])  # before the first call there is no state anywhere: L rows of zeros each, no device needed
    assert f.shape == (2 * 4, 39) and not f.any() and m.state is None
    got = m(z(0), [0, 0, 0], [2, 3])  # entries without rows: no device needed
    assert got.shape == (0, 39) and not m.rows_seen.any()
    for bad in (dict(pool_streams=0, cols=13), dict(pool_streams=4, cols=0)):
        with pytest.raises(ValueError):
            ss.AddDeltasStreamPool(**bad)
    with pytest.raises(ss.SpeechSauceError) as e:
        ss.AddDeltasStreamPool(1, 1 << 25, order=2, window=16)
    assert e.value.status == 3


def test_the_restatement_itself():
    k, D = taps(1, 2)
    assert k.tolist() == [-2, -1, 0, 1, 2] and D == 10
    k, D = taps(2, 2)
    assert k.tolist() == [4, 4, 1, -4, -10, -4, 1, 4, 4] and D == 100
    k, D = taps(2, 16)
    assert np.abs(k).max() == 2992 and D == 8952064 and len(k) == 65
    for order, window in OW:
        k, D = taps(order, window)
        assert k.sum() == 0 and len(k) == 2 * order * window + 1 and np.abs(k).max() < 1 << 12  # the products are exact in f64
    T = 30
    t = np.arange(T, dtype=np.float32)
    # a ramp t * s: delta = s in the interior, 0.5 * s at row 0 for window 2 ((1 * s + 2 * 2 s) / 10), delta-delta = 0 in the interior
    s = np.array([1.0, -2.5], np.float32)
    o = restate(t[:, None] * s[None, :], 2, 2)
    assert o.shape == (T, 6)
    assert np.array_equal(o[:, :2], t[:, None] * s[None, :])  # the static block is a copy
    assert np.allclose(o[2:-2, 2:4], s, rtol=0, atol=1e-6) and np.allclose(o[0, 2:4], 0.5 * s, rtol=0, atol=1e-6)
    assert np.array_equal(o[4:-4, 4:6], np.zeros((T - 8, 2), np.float32))
    # t^2: delta-delta = 2 in the interior
    o = restate((t * t)[:, None], 2, 2)
    assert np.allclose(o[4:-4, 2], 2.0, rtol=0, atol=1e-5)
    for cols in (3, 13):
        for order, window in OW:
            L = order * window
            # a constant column: +0.0, the sign bit clear
            c = np.tile(_clip(cols, 1, seed=5), (2 * L + 5, 1))
            o = restate(c, order, window)
            assert not _u32(o[:, cols:]).any()
            # T = 1: all-zero deltas
            o = restate(_clip(cols, 1, seed=6), order, window)
            assert o.shape == (1, (order + 1) * cols) and not _u32(o[:, cols:]).any()
            # an independent second writing: np.pad(..., "edge") plus slices -- order 1 the textbook sum n (x[t+n] - x[t-n]) / D, order
            # 2 the convolved taps on the padded raw rows -- agrees to 1e-12 in f64 (before the rounding to float32)
            T = 2 * L + 7
            x = _clip(cols, T, seed=7)
            x64 = x.astype(np.float64)
            xp = np.pad(x64, ((window, window), (0, 0)), mode="edge")
            want1 = sum(n * (xp[window + n:window + n + T] - xp[window - n:window - n + T]) for n in range(1, window + 1)) / taps(1, window)[1]
            assert np.abs(_delta_f64(x, np.arange(T), T - 1, 1, window) - want1).max() <= 1e-12
            if order == 2:
                k, D = taps(2, window)
                xp = np.pad(x64, ((L, L), (0, 0)), mode="edge")
                want2 = sum(int(k[j]) * xp[j:j + T] for j in range(2 * L + 1)) / D
                assert np.abs(_delta_f64(x, np.arange(T), T - 1, 2, window) - want2).max() <= 1e-12
            got = restate(x, order, window)
            assert np.array_equal(got[:, :cols], x) and got.shape == (T, (order + 1) * cols)
            assert np.array_equal(got[:, cols:2 * cols], _delta_f64(x, np.arange(T), T - 1, 1, window).astype(np.float32))
    # the composite second delta differs from the first delta of the first delta only near the ends
    x = _clip(4, 30, seed=9)
    d1 = restate(x, 1, 2)[:, 4:]
    it = restate(d1, 1, 2)[:, 4:]
    comp = restate(x, 2, 2)[:, 8:]
    differs = np.flatnonzero(np.abs(it - comp).max(axis=1) > 1e-5)
    assert differs.tolist() == [0, 1, 28, 29]


@pytest.mark.parametrize("order,window", [(2, 2), (1, 2), (2, 1), (2, 3), (1, 9)])
def test_the_stream_model_equals_the_one_shot_model(order, window):
    """Random cuts of 0-5 rows, empty entries included, then flush: all rows, the first L dropped, are the one-shot rows bit for bit."""
    rng = np.random.default_rng(17)
    L = order * window
    for cols in (3, 5, 13, 40):
        for T in sorted({0, 1, 2, L - 1, L, L + 1, 2 * L, 2 * L + 1, 37}):
            x = (rng.standard_normal((T, cols)) * 10).astype(np.float32)
            want = restate(x, order, window)
            for _ in range(3):
                st, outs, pos = StreamModel(cols, order, window), [], 0
                while pos < T:
                    r = int(rng.integers(0, 6))
                    outs.append(st.push(x[pos:pos + r]))
                    assert outs[-1].shape[0] == min(r, T - pos)
                    pos += r
                outs += [st.push(x[:0]), st.flush()]
                got = np.concatenate(outs)
                assert got.shape[0] == T + L
                assert not _u32(got[:L]).any()  # warm-up rows: +0.0
                assert np.array_equal(_u32(got[L:]), _u32(want)), (cols, T)
                assert len(st.hist) == 0


# ---------------------------------------------------------------- GPU ---------------------------------------------------------

def _bits(t):
    import torch

    return t.contiguous().view(torch.int32)


def _packed_call(torch, lib, x, d_off, n_clips, total_rows, cols, order, window, out):
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    return lib.ss_add_deltas_packed_device(x.data_ptr(), n_clips, d_off.data_ptr(), total_rows, cols, order, window, out.data_ptr(), st)


def _packed(torch, lib, clips, cols, order, window):
    """ss_add_deltas_packed_device on a list of host clips [T_b, cols]; returns (out [sum T_b, ocols] on the host, offsets)."""
    off = np.zeros(len(clips) + 1, np.int64)
    np.cumsum([c.shape[0] for c in clips], out=off[1:])
    R = int(off[-1])
    x = torch.from_numpy(np.concatenate(list(clips) + [np.zeros((1, cols), np.float32)])).cuda()
    out = torch.full((R + 1, (order + 1) * cols), float("nan"), device="cuda")
    rc = _packed_call(torch, lib, x, torch.from_numpy(off).cuda(), len(clips), R, cols, order, window, out)
    assert rc == 0, lib.ss_last_error_string()
    torch.cuda.synchronize()
    assert torch.isnan(out[R:]).all()
    return out[:R].cpu().numpy(), off


@pytest.mark.gpu
@pytest.mark.parametrize("order,window", OW)
@pytest.mark.parametrize("cols", COLS)
def test_packed_parity_is_bit_for_bit(ss, sslib, cols, order, window):
    import torch

    L = order * window
    lens = [0, 1, 2, L - 1, L, L + 1, 2 * L, 2 * L + 1, LONG]
    clips = [_clip(cols, T, seed=i) for i, T in enumerate(lens)]
    got, off = _packed(torch, sslib, clips, cols, order, window)
    for i, T in enumerate(lens):
        want = _want(cols, T, order, window, seed=i)
        g = got[off[i]:off[i + 1]]
        assert g.shape == want.shape
        bad = np.flatnonzero((_u32(g) != _u32(want)).any(axis=1))
        assert bad.size == 0, (T, bad[:8], g[bad[:1]], want[bad[:1]])
    # add_deltas of one matrix is the one-clip packed call, and the host form and the Python front move the same bits
    xl = torch.from_numpy(clips[-1].copy()).cuda()
    one = ss.add_deltas(xl, order, window)
    assert one.shape == (LONG, (order + 1) * cols) and np.array_equal(_u32(one.cpu().numpy()), _u32(got[off[-2]:]))
    short = np.concatenate(clips[:-1])
    got_np = ss.add_deltas_packed(short, off[:-1], order, window)
    assert isinstance(got_np, np.ndarray) and np.array_equal(_u32(got_np), _u32(got[:off[-2]]))
    got_t = ss.add_deltas_packed(torch.from_numpy(short).cuda(), torch.from_numpy(off[:-1]).cuda(), order, window)
    assert torch.is_tensor(got_t) and np.array_equal(_u32(got_t.cpu().numpy()), _u32(got[:off[-2]]))
    batch = ss.add_deltas(np.stack([clips[6], clips[6][::-1]]), order, window)  # [2, 2L, cols]: every matrix on its own rows
    assert np.array_equal(_u32(batch[0]), _u32(got[off[6]:off[7]])) and np.array_equal(_u32(batch[1]), _u32(restate(clips[6][::-1], order, window)))


@pytest.mark.gpu
@pytest.mark.parametrize("cols,order,window", [(13, 2, 2), (33, 1, 9), (80, 2, 16), (1, 2, 1)])
def test_a_clip_does_not_depend_on_its_place_in_the_block(sslib, cols, order, window):
    import torch

    mine = _clip(cols, 150, seed=40)  # three row tiles
    a, b, c = _clip(cols, 7, seed=41), _clip(cols, 300, seed=42), _clip(cols, 1, seed=43)
    want = _want(cols, 150, order, window, seed=40)
    for clips, i in (([mine, a, b], 0), ([a, b, mine], 2), ([a, mine, b], 1), ([b, c, mine[:0], mine, a], 3), ([mine], 0)):
        got, off = _packed(torch, sslib, clips, cols, order, window)
        assert np.array_equal(_u32(got[off[i]:off[i + 1]]), _u32(want)), i


@pytest.mark.gpu
def test_bad_segment_tables_are_contained(sslib):
    """A contract check, run once: a reversed segment, a negative start and an end past total_rows are skipped, nothing outside the
    blocks is touched, rows of no valid segment keep their fill and the valid clips are still exact."""
    import torch

    cols, order, window, GUARD, FILL = 33, 2, 2, 70, -777.0
    ocols = 3 * cols
    total_rows = 40
    off = np.array([0, 3, -4, 5, 4, 9, 12, 45, 38, 40], np.int64)
    # c0 0..3 good | c1 3..-4 reversed | c2 -4..5 starts below 0 | c3 5..4 reversed | c4 4..9 good | c5 9..12 good |
    # c6 12..45 ends past total_rows | c7 45..38 reversed | c8 38..40 good
    good = [(0, 3), (4, 9), (9, 12), (38, 40)]
    x_g = torch.full((total_rows + 2 * GUARD, cols), FILL, device="cuda")
    src = _clip(cols, total_rows, seed=50)
    x_g[GUARD:GUARD + total_rows] = torch.from_numpy(src.copy()).cuda()
    x_before = x_g.clone()
    out_g = torch.full((total_rows + 2 * GUARD, ocols), FILL, device="cuda")
    tab_g = torch.full((len(off) + 16,), -(1 << 40), dtype=torch.int64, device="cuda")  # guard words that would be wild offsets
    tab_g[8:8 + len(off)] = torch.from_numpy(off).cuda()
    tab_before = tab_g.clone()
    rc = _packed_call(torch, sslib, x_g[GUARD:GUARD + total_rows], tab_g[8:8 + len(off)], len(off) - 1, total_rows, cols, order, window,
                      out_g[GUARD:GUARD + total_rows])
    assert rc == 0, sslib.ss_last_error_string()  # the table is device data: the call itself cannot know
    torch.cuda.synchronize()
    out = out_g[GUARD:GUARD + total_rows].cpu().numpy()
    written = np.zeros(total_rows, bool)
    for lo, hi in good:
        assert np.array_equal(_u32(out[lo:hi]), _u32(restate(src[lo:hi], order, window))), (lo, hi)  # valid clips are still exact
        written[lo:hi] = True
    assert (out[~written] == FILL).all() and (~written).sum() == 27  # rows of no valid segment keep their fill
    assert (out_g[:GUARD] == FILL).all() and (out_g[GUARD + total_rows:] == FILL).all()
    assert torch.equal(_bits(x_g), _bits(x_before)) and torch.equal(tab_g, tab_before)


@pytest.mark.gpu
@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
@pytest.mark.parametrize("cols,order,window", [(13, 2, 2), (33, 1, 9), (80, 2, 16)])
def test_a_nan_or_inf_reaches_exactly_the_outputs_whose_taps_cover_it(sslib, cols, order, window, bad):
    import torch

    L = order * window
    T, t0, c0 = 3 * L + 40, L + 17, cols - 2
    clips = [_clip(cols, 9, seed=60), _clip(cols, T, seed=61).copy(), _clip(cols, 2 * L + 3, seed=62)]
    clean, off = _packed(torch, sslib, clips, cols, order, window)
    clips[1][t0, c0] = bad
    got, _ = _packed(torch, sslib, clips, cols, order, window)
    hit = np.zeros(got.shape, bool)
    lo = int(off[1])
    hit[lo + t0, c0] = True  # the static copy
    for o in range(1, order + 1):
        k, _ = taps(o, window)
        half = o * window
        for j in range(-half, half + 1):
            if k[j + half] != 0 and 0 <= t0 - j < T:  # output row t0 - j reads row t0 under tap j (no clamped index is t0: it is interior)
                hit[lo + t0 - j, o * cols + c0] = True
    assert not hit[lo + t0, cols + c0]  # the first delta of the row itself: its centre tap is zero and skipped
    assert np.isfinite(got[lo + t0, cols + c0])
    assert np.array_equal(~np.isfinite(got), hit)
    assert np.array_equal(_u32(got)[~hit], _u32(clean)[~hit])  # nothing else changes a bit
    want = restate(clips[1], order, window)
    assert np.array_equal(~np.isfinite(want), hit[lo:lo + T])


def _stream_raw(torch, lib, x, n_active, d_ro, total_rows, d_sl, pool_streams, cols, order, window, pool, out, stream=None):
    st = C.c_void_p(stream if stream is not None else torch.cuda.current_stream().cuda_stream)
    return lib.ss_add_deltas_stream_packed_device(x.data_ptr(), n_active, d_ro.data_ptr(), total_rows, d_sl.data_ptr(), pool_streams, cols,
                                                  order, window, pool.data_ptr(), out.data_ptr(), st)


def _stream_call(torch, lib, chunks, slots, pool, cols, order, window):
    """One pool call on a list of [R_i, cols] device blocks; returns (out [total_rows, ocols], ro)."""
    ro = np.zeros(len(chunks) + 1, np.int64)
    np.cumsum([int(c.shape[0]) for c in chunks], out=ro[1:])
    R = int(ro[-1])
    x = torch.cat(list(chunks)) if R else torch.zeros((1, cols), device="cuda")
    out = torch.full((max(R, 1), (order + 1) * cols), float("nan"), device="cuda")
    rc = _stream_raw(torch, lib, x, len(chunks), torch.from_numpy(ro).cuda(), R, torch.tensor(list(slots), dtype=torch.int32, device="cuda"),
                     pool.shape[0], cols, order, window, pool, out)
    assert rc == 0, lib.ss_last_error_string()
    return out[:R], ro


def _flush_call(torch, lib, slots, pool, cols, order, window):
    L = order * window
    out = torch.full((len(slots) * L, (order + 1) * cols), float("nan"), device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = lib.ss_add_deltas_stream_flush_device(len(slots), torch.tensor(list(slots), dtype=torch.int32, device="cuda").data_ptr(), pool.shape[0], cols,
                                               order, window, pool.data_ptr(), out.data_ptr(), st)
    assert rc == 0, lib.ss_last_error_string()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("order,window", OW)
@pytest.mark.parametrize("cols", COLS)
def test_stream_rows_plus_flush_are_the_packed_call_however_the_stream_is_cut(sslib, cols, order, window):
    """Three streams cut differently over many calls (0-5 rows per entry, absent entries, and one catch-up entry long enough to leave
    the LDS path) and a fourth shorter than L, then flush: per stream the rows after the first L are ss_add_deltas_packed_device on
    the whole clip bit for bit, and the first L are +0.0."""
    import torch

    L = order * window
    CATCH = STREAM_ROWS + 12  # with any history this entry sees more than STREAM_ROWS rows
    rng = np.random.default_rng(100 * cols + 10 * order + window)
    lens = [2 * L + 20 + CATCH, 3 * L + 9 + CATCH, 2 * L + 31 + CATCH, max(L - 1, 1) if L > 1 else 1]
    if L > 1:
        assert lens[3] < L
    B, P = len(lens), 9
    slots = [5, 0, 7, 2]
    clips = [_clip(cols, T, seed=70 + b) for b, T in enumerate(lens)]
    dev = [torch.from_numpy(c.copy()).cuda() for c in clips]
    whole, off = _packed(torch, sslib, clips, cols, order, window)
    pool = torch.zeros((P, 2 * L * cols + 1), device="cuda")
    at, got, n_calls = [0] * B, [[] for _ in range(B)], 0
    catch_at = [3, 1, 6, None]  # the call in which stream b brings its catch-up entry
    while any(at[b] < lens[b] for b in range(B)) or n_calls < 8:
        entries, chunks = [], []
        for b in rng.permutation(B):
            left = lens[b] - at[b]
            if catch_at[b] == n_calls:
                r = min(CATCH, left)
            elif rng.random() < 0.2:
                continue  # absent from this call
            else:
                r = min(int(rng.integers(0, 6)), left)
            entries.append(b)
            chunks.append(dev[b][at[b]:at[b] + r])
            at[b] += r
        if entries:
            out, ro = _stream_call(torch, sslib, chunks, [slots[b] for b in entries], pool, cols, order, window)
            for i, b in enumerate(entries):
                got[b].append(out[ro[i]:ro[i + 1]].clone())
        n_calls += 1
    assert n_calls >= 8
    counts = pool[slots, -1].cpu().numpy()
    assert counts.tolist() == [float(min(T, 2 * L)) for T in lens]
    tail = _flush_call(torch, sslib, slots, pool, cols, order, window)
    torch.cuda.synchronize()
    assert not pool.any()  # flushed streams are fresh, the other pool rows were never touched
    for b in range(B):
        rows = torch.cat(got[b] + [tail[b * L:(b + 1) * L]]).cpu().numpy()
        assert rows.shape == (lens[b] + L, (order + 1) * cols)
        assert not _u32(rows[:L]).any(), b  # warm-up rows: +0.0
        want = whole[off[b]:off[b + 1]]
        bad = np.flatnonzero((_u32(rows[L:]) != _u32(want)).any(axis=1))
        assert bad.size == 0, (b, bad[:8])
        assert np.array_equal(_u32(want), _u32(_want(cols, lens[b], order, window, seed=70 + b)))


@pytest.mark.gpu
@pytest.mark.parametrize("cols,order,window", [(13, 2, 2), (33, 1, 9), (80, 2, 16)])
def test_an_entry_does_not_depend_on_its_place_slot_or_neighbours(sslib, cols, order, window):
    import torch

    L = order * window
    len_ = 2 * L * cols + 1
    s = [torch.from_numpy(_clip(cols, 3 * L + 60, seed=80 + b).copy()).cuda() for b in range(5)]
    P = 12
    base = torch.zeros((P, len_), device="cuda")
    _stream_call(torch, sslib, [s[b][:2 * L + 3] for b in range(4)], [7, 0, 1, 2], base, cols, order, window)  # full histories
    base[9] = base[7]  # the same stream state in another slot
    a0 = 2 * L + 3
    mine = s[0][a0:a0 + 5]
    other = [s[b][a0:a0 + r] for b, r in ((1, 1), (2, 37), (3, 2), (4, 9))]
    empty = mine[:0]
    layouts = {"first": ([mine] + other, [7, 0, 1, 2, 3]),
               "last": (other + [mine], [0, 1, 2, 3, 7]),
               "other_slot": (other[:2] + [mine] + other[2:], [0, 1, 9, 2, 3]),
               "between_empties": (other[:2] + [empty, mine, empty] + other[2:], [0, 1, 10, 7, 11, 2, 3]),
               "alone": ([mine], [7])}
    rows, states, tails = {}, {}, {}
    for key, (chunks, slots) in layouts.items():
        pool = base.clone()
        out, ro = _stream_call(torch, sslib, chunks, slots, pool, cols, order, window)
        slot = 9 if key == "other_slot" else 7
        i = slots.index(slot)
        rows[key] = out[ro[i]:ro[i + 1]].clone()
        states[key] = pool[slot].clone()
        if key == "between_empties":  # R_i == 0: the pool row is left bit for bit
            assert torch.equal(_bits(pool[10]), _bits(base[10])) and torch.equal(_bits(pool[11]), _bits(base[11]))
        fl_slots = [s_ for s_ in slots if s_ not in (10, 11)]
        tail = _flush_call(torch, sslib, fl_slots[::-1], pool, cols, order, window)  # and the flush, in another order
        j = fl_slots[::-1].index(slot)
        tails[key] = tail[j * L:(j + 1) * L].clone()
    torch.cuda.synchronize()
    want = _want(cols, 3 * L + 60, order, window, seed=80)
    assert np.array_equal(_u32(rows["alone"].cpu().numpy()), _u32(want[a0 - L:a0 + 5 - L]))
    whole = restate(_clip(cols, 3 * L + 60, seed=80)[:a0 + 5], order, window)
    assert np.array_equal(_u32(tails["alone"].cpu().numpy()), _u32(whole[a0 + 5 - L:]))
    for key in layouts:
        assert torch.equal(_bits(rows[key]), _bits(rows["alone"])), key
        assert torch.equal(_bits(states[key]), _bits(states["alone"])), key
        assert torch.equal(_bits(tails[key]), _bits(tails["alone"])), key


@pytest.mark.gpu
def test_pool_memory_the_call_does_not_own_is_left_as_it_was(sslib):
    import torch

    cols, order, window, P, FILL = 33, 2, 2, 9, -777.0
    L = order * window
    len_ = 2 * L * cols + 1
    s = [torch.from_numpy(_clip(cols, 60, seed=90 + b).copy()).cuda() for b in range(6)]
    pool = torch.full((P, len_), FILL, device="cuda")
    named, empties = [4, 1, 7], [2, 6]
    pool[named] = 0.0
    before = pool.clone()
    chunks = [s[0][:3], s[1][:0], s[2][:40], s[3][:0], s[4][:1]]
    slots = [4, 2, 1, 6, 7]
    ro = np.zeros(6, np.int64)
    np.cumsum([c.shape[0] for c in chunks], out=ro[1:])
    R, EXTRA = int(ro[-1]), 5
    x = torch.cat(chunks + [s[5][:EXTRA]])
    out = torch.full((R + EXTRA, 3 * cols), FILL, device="cuda")
    rc = _stream_raw(torch, sslib, x, 5, torch.from_numpy(ro).cuda(), R + EXTRA, torch.tensor(slots, dtype=torch.int32, device="cuda"), P, cols,
                     order, window, pool, out)
    assert rc == 0, sslib.ss_last_error_string()
    torch.cuda.synchronize()
    assert (out[R:] == FILL).all()  # rows past ro[n_active]
    assert not (out[:R] == FILL).any()
    for r in range(P):
        if r in named:
            assert not torch.equal(pool[r], before[r]), r
        else:  # never named, or named by an entry without rows
            assert torch.equal(_bits(pool[r]), _bits(before[r])), r
    for b, i in ((0, 0), (2, 2), (4, 4)):
        n = int(chunks[i].shape[0])
        m = StreamModel(cols, order, window)
        assert np.array_equal(_u32(out[ro[i]:ro[i + 1]].cpu().numpy()), _u32(m.push(_clip(cols, 60, seed=90 + b)[:n]))), b
        keep = min(n, 2 * L)
        row = pool[slots[i]].cpu().numpy()
        hist = row[:-1].reshape(2 * L, cols)
        assert row[-1] == keep and np.array_equal(hist[2 * L - keep:], m.hist) and not hist[:2 * L - keep].any()


@pytest.mark.gpu
def test_bad_device_tables_and_count_words_are_contained(sslib):
    """A contract check, run once.  The entry decoder bounds every access before it happens: a bad entry is skipped, a bad count
    word is read as a fresh stream, nothing outside the buffers is touched and the good entries of the same call are still exact."""
    import torch

    cols, order, window, P, GUARD, FILL = 13, 2, 2, 8, 4, -777.0
    L = order * window
    H = 2 * L
    len_, ocols = H * cols + 1, 3 * cols
    s = [torch.from_numpy(_clip(cols, 260, seed=110 + b).copy()).cuda() for b in range(P)]

    def single(chunk, state_row):
        """The expected rows and pool row of one entry: the same call on that entry alone."""
        p = state_row[None, :].clone()
        o, _ = _stream_call(torch, sslib, [chunk], [0], p, cols, order, window)
        return o.clone(), p[0].clone()

    # ---- bad tables: entry i owns ro[i] .. ro[i+1] ----
    ro = np.array([0, 3, 5, 4, 6, 9, -2, 11, 13, 16], np.int64)
    total_rows = 14
    slots = [1, P, 2, 3, -1, 4, 6, 5, 7]
    #        e0 good | e1 slot = pool_streams | e2 decreasing | e3 good | e4 slot = -1 | e5 decreasing, below 0 | e6 starts below 0 |
    #        e7 good | e8 ends past total_rows
    good = {0: (0, 3), 3: (4, 6), 7: (11, 13)}
    x_g = torch.full((total_rows + 2 * GUARD, cols), FILL, device="cuda")
    x = x_g[GUARD:GUARD + total_rows]
    x.copy_(s[6][100:100 + total_rows])
    x_before = x_g.clone()
    out_g = torch.full((total_rows + 2 * GUARD, ocols), FILL, device="cuda")
    out = out_g[GUARD:GUARD + total_rows]
    pool_g = torch.full((P + 2 * GUARD, len_), FILL, device="cuda")
    pool = pool_g[GUARD:GUARD + P]
    _stream_call(torch, sslib, [s[b][:40] for b in range(P)], list(range(P)), pool.zero_(), cols, order, window)  # valid states everywhere
    before = pool.clone()
    want = {i: single(x[a:b], before[slots[i]]) for i, (a, b) in good.items()}
    rc = _stream_raw(torch, sslib, x, len(slots), torch.from_numpy(ro).cuda(), total_rows, torch.tensor(slots, dtype=torch.int32, device="cuda"),
                     P, cols, order, window, pool, out)
    assert rc == 0, sslib.ss_last_error_string()  # the tables are device data: the call itself cannot know
    torch.cuda.synchronize()
    written = np.zeros(total_rows, bool)
    for i, (a, b) in good.items():
        assert torch.equal(_bits(out[a:b]), _bits(want[i][0])), i
        assert torch.equal(_bits(pool[slots[i]]), _bits(want[i][1])), i
        written[a:b] = True
    assert (out[torch.from_numpy(~written).cuda()] == FILL).all()  # what the skipped entries claimed keeps its pre-fill
    for r in set(range(P)) - {slots[i] for i in good}:
        assert torch.equal(_bits(pool[r]), _bits(before[r])), r
    assert (out_g[:GUARD] == FILL).all() and (out_g[GUARD + total_rows:] == FILL).all()
    assert (pool_g[:GUARD] == FILL).all() and (pool_g[GUARD + P:] == FILL).all()
    assert torch.equal(_bits(x_g), _bits(x_before))
    # the flush with a slot outside the pool: that entry's L rows keep their fill, the others are flushed
    fl_g = torch.full((3 * L + 2 * GUARD, ocols), FILL, device="cuda")
    kept = pool.clone()
    rc = sslib.ss_add_deltas_stream_flush_device(3, torch.tensor([2, P, -1], dtype=torch.int32, device="cuda").data_ptr(), P, cols, order, window,
                                                 pool.data_ptr(), fl_g[GUARD:GUARD + 3 * L].data_ptr(), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, sslib.ss_last_error_string()
    torch.cuda.synchronize()
    assert not (fl_g[GUARD:GUARD + L] == FILL).any() and (fl_g[:GUARD] == FILL).all() and (fl_g[GUARD + L:] == FILL).all()
    assert not pool[2].any()
    for r in set(range(P)) - {2}:
        assert torch.equal(_bits(pool[r]), _bits(kept[r])), r
    assert (pool_g[:GUARD] == FILL).all() and (pool_g[GUARD + P:] == FILL).all()

    # ---- bad count words: read as 0, a fresh stream, whatever the history floats hold ----
    words = [float("nan"), -1.0, float(H + 1), 0.5, 1e9, float("inf")]
    gen = torch.Generator(device="cuda")
    gen.manual_seed(9)
    pool.copy_(torch.randn((P, len_), generator=gen, device="cuda") * 50)  # garbage history
    for r, w in enumerate(words):
        pool[r, -1] = w
    control = before[6].clone()
    pool[6] = control  # one valid state beside them
    assert control[-1] == H
    chunks = [s[r][200:200 + n] for r, n in zip(range(len(words)), (2, 1, 5, 35, 3, 2))] + [s[6][40:44]]
    ro2 = np.zeros(len(chunks) + 1, np.int64)
    np.cumsum([c.shape[0] for c in chunks], out=ro2[1:])
    R = int(ro2[-1])
    x2_g = torch.full((R + 2 * GUARD, cols), FILL, device="cuda")
    x2_g[GUARD:GUARD + R] = torch.cat(chunks)
    out2_g = torch.full((R + 2 * GUARD, ocols), FILL, device="cuda")
    fresh = torch.zeros(len_, device="cuda")
    want2 = [single(c, fresh) for c in chunks[:-1]] + [single(chunks[-1], control)]
    rc = _stream_raw(torch, sslib, x2_g[GUARD:GUARD + R], len(chunks), torch.from_numpy(ro2).cuda(), R,
                     torch.tensor(list(range(len(words))) + [6], dtype=torch.int32, device="cuda"), P, cols, order, window, pool,
                     out2_g[GUARD:GUARD + R])
    assert rc == 0, sslib.ss_last_error_string()
    torch.cuda.synchronize()
    for i, c in enumerate(chunks):
        slot = i if i < len(words) else 6
        assert torch.equal(_bits(out2_g[GUARD + ro2[i]:GUARD + ro2[i + 1]]), _bits(want2[i][0])), i
        assert torch.equal(_bits(pool[slot]), _bits(want2[i][1])), i
        if i < len(words):  # and a fresh stream is what the definition says
            ref = StreamModel(cols, order, window).push(c.cpu().numpy())
            assert np.array_equal(_u32(want2[i][0].cpu().numpy()), _u32(ref)), i
    assert (out2_g[:GUARD] == FILL).all() and (out2_g[GUARD + R:] == FILL).all()
    assert (pool_g[:GUARD] == FILL).all() and (pool_g[GUARD + P:] == FILL).all()


@pytest.mark.gpu
def test_zeroing_a_pool_row_and_flush_both_give_a_fresh_stream(sslib):
    import torch

    cols, order, window = 33, 2, 2
    L = order * window
    len_ = 2 * L * cols + 1
    s = [torch.from_numpy(_clip(cols, 90, seed=120 + b).copy()).cuda() for b in range(3)]
    pool = torch.zeros((5, len_), device="cuda")
    _stream_call(torch, sslib, [s[0][:50], s[1][:50], s[2][:50]], [2, 4, 0], pool, cols, order, window)
    pool[2] = 0.0                                                 # reset mid-stream
    _flush_call(torch, sslib, [4], pool, cols, order, window)      # flushed mid-stream
    out, ro = _stream_call(torch, sslib, [s[0][50:90], s[1][50:90], s[2][50:90]], [2, 4, 0], pool, cols, order, window)
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    for i in (0, 1):
        fresh = StreamModel(cols, order, window).push(_clip(cols, 90, seed=120 + i)[50:90])
        assert np.array_equal(_u32(out[ro[i]:ro[i + 1]]), _u32(fresh)), i
        assert not _u32(out[ro[i]:ro[i] + L]).any()
    cont = _want(cols, 90, order, window, seed=122)
    assert np.array_equal(_u32(out[ro[2]:ro[3]]), _u32(cont[50 - L:90 - L]))  # the untouched stream goes on


@pytest.mark.gpu
@pytest.mark.parametrize("order,window", [(2, 2), (1, 9)])
def test_host_forms_and_python_class_equal_the_device_forms(ss, sslib, order, window):
    import torch

    cols, P = 13, 9
    L = order * window
    len_, ocols = 2 * L * cols + 1, (order + 1) * cols
    s = [torch.from_numpy(_clip(cols, 200, seed=130 + b).copy()).cuda() for b in range(4)]
    calls = [([s[0][:3], s[1][:0], s[2][:40]], [4, 1, 7]),
             ([s[2][40:45], s[0][3:4]], [7, 4]),
             ([s[1][:150], s[0][4:6], s[3][:0]], [1, 4, 0])]  # 150 rows: the catch-up path
    pool_d = torch.zeros((P, len_), device="cuda")
    pool_h = np.zeros((P, len_), np.float32)
    m_np = ss.AddDeltasStreamPool(P, cols, order=order, window=window)
    m_t = ss.AddDeltasStreamPool(P, cols, order=order, window=window)
    seen = np.zeros(P, np.int64)
    for chunks, slots in calls:
        dev, ro = _stream_call(torch, sslib, chunks, slots, pool_d, cols, order, window)
        torch.cuda.synchronize()
        dev = dev.cpu().numpy()
        R = int(ro[-1])
        xh = torch.cat(chunks).cpu().numpy()
        FILL = np.float32(-3.0)
        outh = np.full((R, ocols), FILL)
        sl = np.asarray(slots, np.int32)
        before = pool_h.copy()
        dup = np.full(len(slots), slots[0], np.int32)
        rc = sslib.ss_add_deltas_stream_packed(xh.ctypes.data, len(slots), ro.ctypes.data, dup.ctypes.data, P, cols, order, window,
                                               pool_h.ctypes.data, outh.ctypes.data)
        assert rc == 3 and b"entry 1" in sslib.ss_last_error_string()  # a slot named twice: rejected, nothing written
        assert np.array_equal(pool_h, before) and (outh == FILL).all()
        rc = sslib.ss_add_deltas_stream_packed(xh.ctypes.data, len(slots), ro.ctypes.data, sl.ctypes.data, P, cols, order, window,
                                               pool_h.ctypes.data, outh.ctypes.data)
        assert rc == 0, sslib.ss_last_error_string()
        assert np.array_equal(_u32(outh), _u32(dev))
        assert np.array_equal(_u32(pool_h), _u32(pool_d.cpu().numpy()))
        changed = {int(r) for r in np.flatnonzero((pool_h != before).any(axis=1))}
        assert changed <= {int(v) for v, c in zip(slots, chunks) if c.shape[0] > 0}  # only named rows with new rows moved
        got_np = m_np(xh, ro, slots)
        got_t = m_t(torch.cat(chunks), ro, slots)
        assert isinstance(got_np, np.ndarray) and torch.is_tensor(got_t)
        assert np.array_equal(_u32(got_np), _u32(dev)) and np.array_equal(_u32(got_t.cpu().numpy()), _u32(dev))
        seen[sl] += np.diff(ro)
        assert np.array_equal(m_np.rows_seen, seen) and np.array_equal(m_t.rows_seen, seen)
    torch.cuda.synchronize()
    assert m_np.state.shape == (P, len_) and np.array_equal(_u32(m_np.state), _u32(pool_h))
    assert torch.equal(_bits(m_t.state), _bits(pool_d))
    with pytest.raises(ValueError):
        m_np(torch.cat(calls[0][0]), [0, 3, 3, 43], [4, 1, 7])  # the pool lives on the host
    assert np.array_equal(m_np.rows_seen, seen)
    # reset(slots=[...]) makes exactly those streams fresh
    for m in (m_np, m_t):
        m.reset(slots=[7])
        st = m.state if isinstance(m.state, np.ndarray) else m.state.cpu().numpy()
        assert not st[7].any() and np.array_equal(_u32(st[4]), _u32(pool_h[4])) and m.rows_seen[7] == 0 and m.rows_seen[4] == seen[4]
    pool_d[7] = 0.0
    pool_h[7] = 0.0
    seen[7] = 0
    # the flush: device form, host form and both classes
    fl = [1, 7, 4, 3]  # a long stream, a fresh one, a short one (6 rows) and a never-named one
    tail_d = _flush_call(torch, sslib, fl, pool_d, cols, order, window)
    torch.cuda.synchronize()
    tail_d = tail_d.cpu().numpy()
    tail_h = np.full((len(fl) * L, ocols), np.float32(-3.0))
    before = pool_h.copy()
    rc = sslib.ss_add_deltas_stream_flush(len(fl), np.array([1, 7, 1, 3], np.int32).ctypes.data, P, cols, order, window, pool_h.ctypes.data,
                                          tail_h.ctypes.data)
    assert rc == 3 and b"entry 2" in sslib.ss_last_error_string() and np.array_equal(pool_h, before) and (tail_h == -3.0).all()
    rc = sslib.ss_add_deltas_stream_flush(len(fl), np.array(fl, np.int32).ctypes.data, P, cols, order, window, pool_h.ctypes.data, tail_h.ctypes.data)
    assert rc == 0, sslib.ss_last_error_string()
    assert np.array_equal(_u32(tail_h), _u32(tail_d)) and np.array_equal(_u32(pool_h), _u32(pool_d.cpu().numpy()))
    assert not pool_h[fl].any()
    whole1 = restate(_clip(cols, 200, seed=131)[:150], order, window)
    assert np.array_equal(_u32(tail_d[:L]), _u32(whole1[150 - L:]))
    assert not _u32(tail_d[L:2 * L]).any() and not _u32(tail_d[3 * L:]).any()  # fresh streams flush to zero rows
    whole0 = restate(_clip(cols, 200, seed=130)[:6], order, window)
    short = tail_d[2 * L:3 * L]
    assert np.array_equal(_u32(short[max(L - 6, 0):]), _u32(whole0[max(6 - L, 0):])) and not _u32(short[:max(L - 6, 0)]).any()
    t_np, t_t = m_np.flush(fl), m_t.flush(fl)
    assert isinstance(t_np, np.ndarray) and torch.is_tensor(t_t)
    assert np.array_equal(_u32(t_np), _u32(tail_d)) and np.array_equal(_u32(t_t.cpu().numpy()), _u32(tail_d))
    seen[fl] = 0
    assert np.array_equal(m_np.rows_seen, seen) and np.array_equal(m_t.rows_seen, seen)
    assert np.array_equal(_u32(m_np.state), _u32(pool_h)) and torch.equal(_bits(m_t.state), _bits(pool_d))
    for m in (m_np, m_t):
        m.reset()
        st = m.state if isinstance(m.state, np.ndarray) else m.state.cpu().numpy()
        assert not st.any() and not m.rows_seen.any()


def _hip_runtime():
    """The HIP runtime this process has loaded (torch's), for the stream-capture calls the graph-shape check needs."""
    with open("/proc/self/maps") as f:
        paths = {line.split()[-1] for line in f if "libamdhip64" in line}
    assert paths, "no HIP runtime loaded"
    return C.CDLL(sorted(paths)[0])


@pytest.mark.gpu
def test_graph_of_the_feature_call_the_normalisation_and_the_deltas_on_the_same_tables(ss, sslib):
    import torch

    from speechsauce_amd import _lib

    cfg = ss.SpeechConfig(_lib.make_params())  # the default 512-point shape
    N, CAP, P, STEP, COLS_, WIN, NORM, ORDER, WINDOW = 5, 24, 8, 160, 13, 31, 100, 2, 2
    LC = (WIN - 1) * COLS_ + 1
    LD = 2 * ORDER * WINDOW * COLS_ + 1
    x = torch.zeros(CAP * STEP, device="cuda")
    d_so = torch.zeros(N + 1, dtype=torch.int64, device="cuda")
    d_ro = torch.zeros(N + 1, dtype=torch.int64, device="cuda")
    d_sl = torch.arange(N, dtype=torch.int32, device="cuda")
    feat = torch.zeros((CAP, COLS_), device="cuda")
    norm = torch.zeros((CAP, COLS_), device="cuda")
    out = torch.zeros((CAP, 3 * COLS_), device="cuda")
    pools_g = [torch.zeros((P, n), device="cuda") for n in (STEP, LC, LD)]
    pools_e = [torch.zeros((P, n), device="cuda") for n in (STEP, LC, LD)]

    def deltas(dpool, stream, n=N):
        return _stream_raw(torch, sslib, norm, n, d_ro, CAP, d_sl, P, COLS_, ORDER, WINDOW, dpool, out, stream=stream)

    def chain(pools, stream=None, n=N):
        stream = stream if stream is not None else torch.cuda.current_stream().cuda_stream
        st = C.c_void_p(stream)
        rc = sslib.ss_mfcc_stream_packed_device(cfg.handle, x.data_ptr(), n, d_so.data_ptr(), d_ro.data_ptr(), CAP, d_sl.data_ptr(), P, NORM,
                                                pools[0].data_ptr(), feat.data_ptr(), st)
        assert rc == 0, sslib.ss_last_error_string()
        rc = sslib.ss_cmvn_stream_packed_device(feat.data_ptr(), n, d_ro.data_ptr(), CAP, d_sl.data_ptr(), P, COLS_, WIN, 1, pools[1].data_ptr(),
                                                norm.data_ptr(), st)
        assert rc == 0, sslib.ss_last_error_string()
        assert deltas(pools[2], stream, n) == 0, sslib.ss_last_error_string()

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up outside the capture (the zero tables are N entries without rows)
        chain([p.clone() for p in pools_g], stream=side.cuda_stream)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    hip = _hip_runtime()
    hip.hipGraphGetNodes.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_size_t)]
    hip.hipGraphGetEdges.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_size_t)]
    hip.hipGraphNodeGetType.argtypes = [C.c_void_p, C.POINTER(C.c_int)]

    def captured(record):
        """-> (node handles, node kinds, edges) of what `record(stream)` puts on a capturing stream."""
        raw, graph = torch.cuda.Stream(), C.c_void_p()
        assert hip.hipStreamBeginCapture(C.c_void_p(raw.cuda_stream), 2) == 0  # hipStreamCaptureModeRelaxed
        try:
            record(raw.cuda_stream)
        finally:
            assert hip.hipStreamEndCapture(C.c_void_p(raw.cuda_stream), C.byref(graph)) == 0
        n_nodes = C.c_size_t()
        assert hip.hipGraphGetNodes(graph, None, C.byref(n_nodes)) == 0
        nodes = (C.c_void_p * n_nodes.value)()
        assert hip.hipGraphGetNodes(graph, nodes, C.byref(n_nodes)) == 0
        kinds = []
        for node in nodes:
            kind = C.c_int(-1)
            assert hip.hipGraphNodeGetType(node, C.byref(kind)) == 0
            kinds.append(kind.value)
        n_edges = C.c_size_t()
        assert hip.hipGraphGetEdges(graph, None, None, C.byref(n_edges)) == 0
        src, dst = (C.c_void_p * max(n_edges.value, 1))(), (C.c_void_p * max(n_edges.value, 1))()
        if n_edges.value:
            assert hip.hipGraphGetEdges(graph, src, dst, C.byref(n_edges)) == 0
        edges = [(src[i], dst[i]) for i in range(n_edges.value)]
        assert hip.hipGraphDestroy(graph) == 0
        return list(nodes), kinds, edges

    # the delta call alone: ONE kernel node, for 3 entries as for 5
    for n in (N, 3):
        nodes, kinds, edges = captured(lambda s, n=n: deltas(pools_g[2], s, n))
        assert kinds == [0] and not edges, (n, kinds)  # hipGraphNodeTypeKernel
    # the chain of the three calls: a linear chain, no parallel branches
    nodes, kinds, edges = captured(lambda s: chain(pools_g, stream=s))
    assert len(nodes) >= 3 and len(edges) == len(nodes) - 1, (len(nodes), len(edges))
    assert len({a for a, _ in edges}) == len(edges) and len({b for _, b in edges}) == len(edges)  # one successor, one predecessor at the most
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        chain(pools_g)
    rng = np.random.default_rng(44)
    for k in range(2):  # two ticks with changed tables
        hops = rng.integers(0, 5, N)
        hops[rng.integers(0, N)] = 0  # an entry without rows
        slots = rng.permutation(P)[:N].astype(np.int32)
        so = np.zeros(N + 1, np.int64)
        np.cumsum(hops * STEP, out=so[1:])
        ro = so // STEP
        gen = torch.Generator(device="cuda")
        gen.manual_seed(45 + k)
        xs = torch.randn(int(so[-1]), generator=gen, device="cuda").mul_(0.1)
        x.zero_()
        x[:xs.numel()] = xs
        d_so.copy_(torch.from_numpy(so))
        d_ro.copy_(torch.from_numpy(ro))
        d_sl.copy_(torch.from_numpy(slots))
        for t in (feat, norm, out):
            t.fill_(float("nan"))
        chain(pools_e)  # eager, on the other pools
        torch.cuda.synchronize()
        want = [t.clone() for t in (feat, norm, out)]
        for t in (feat, norm, out):
            t.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        R = int(ro[-1])
        assert R > 0 and torch.isfinite(out[:R]).all()
        for got_t, want_t in zip((feat, norm, out), want):
            assert torch.equal(_bits(got_t), _bits(want_t)), k
        assert torch.isnan(out[R:]).all()  # rows past the last entry are left alone
        for a, b in zip(pools_g, pools_e):
            assert torch.equal(_bits(a), _bits(b)), k
    assert sslib.ss_config_device_status(cfg.handle) == 0


@pytest.mark.gpu
def test_end_to_end_mfcc_cmvn_deltas_against_the_oracle(ss, oracle):
    """mfcc_packed of four clips of 0.3-2 s -> cmvn_packed -> add_deltas_packed, per clip within RTOL (relative to the clip's
    largest value, the block metric of test_packed_post.py) of the oracle's MFCC put through numpy CMVN and the restatement."""
    import torch

    rng = np.random.default_rng(77)
    lens = np.array([4800, 32000, 11111, 20480], np.int64)  # 0.3 s .. 2 s at 16 kHz
    x = (rng.standard_normal(int(lens.sum())) * 0.1).astype(np.float32)
    feats, fo = ss.mfcc_packed(torch.from_numpy(x).cuda(), lens, 16000)
    out = ss.add_deltas_packed(ss.cmvn_packed(feats, fo), fo)
    torch.cuda.synchronize()
    got, off = out.cpu().numpy(), fo.cpu().numpy()
    so = np.concatenate([[0], np.cumsum(lens)])
    p = oracle.make_params()
    assert got.shape == (int(off[-1]), 39)
    for b in range(len(lens)):
        m = np.asarray(oracle.mfcc(p, x[so[b]:so[b + 1]]), dtype=np.float64)
        assert m.shape[0] == off[b + 1] - off[b] > 2 * 4
        normed = (m - m.mean(axis=0)).astype(np.float32)
        want = restate(normed, 2, 2)
        e = rel(got[off[b]:off[b + 1]], want)
        print(f"clip {b}: {m.shape[0]} rows, rel {e:.3g}")
        assert e <= RTOL, (b, e)
