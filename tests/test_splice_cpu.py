"""Frame splicing and subsampling (ss_splice_*), the part that needs no device: the numpy restatement of the header's definition and
the numpy model of the pool (tests/splice_model.py) held to the invariant of the header over random cuts, the rule for a stream's
end, low frame rate against FunASR's apply_lfr, the two host-only calls against their formulas, every argument error, the symbols
and the Python front's argument rules."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from splice_model import LFR, PARAMS, StreamModel, apply_lfr, clip, delay_hist, splice_ref, u32

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"ss_splice_packed_offsets": 4, "ss_splice_packed_device": 12, "ss_splice_packed": 9, "ss_splice_stream_state_len": 6,
         "ss_splice_stream_packed_device": 13, "ss_splice_stream_packed": 11, "ss_splice_stream_flush_device": 10,
         "ss_splice_stream_flush": 9}
PERIODS = (0, 1, 2, 3, 7, 13)  # stream lengths K, in periods


def test_the_restatement_itself():
    x = np.arange(10, dtype=np.float32)[:, None] * np.array([1, 100], np.float32)  # row t = [t, 100 t]
    assert splice_ref(x, 1, 1, 1)[:, ::2].tolist() == [[max(t - 1, 0), t, min(t + 1, 9)] for t in range(10)]  # splice-feats
    assert np.array_equal(splice_ref(x, 0, 0, 3), x[::3])                                                      # subsample-feats --n=3
    assert splice_ref(x, 0, 0, 4).shape == (3, 2) and splice_ref(x, 2, 1, 4).shape == (3, 8)                   # ceil(10 / 4)
    assert splice_ref(x, 2, 1, 4)[:, ::2].tolist() == [[0, 0, 0, 1], [2, 3, 4, 5], [6, 7, 8, 9]]
    assert splice_ref(x[:0], 3, 2, 2).shape == (0, 12) and splice_ref(x[:1], 3, 2, 2)[:, ::2].tolist() == [[0] * 6]
    for left, right, stride in PARAMS:
        for T in (1, 2, 5, 31):
            xs = clip(3, T, seed=1)
            got = splice_ref(xs, left, right, stride)
            assert got.shape == (-(-T // stride), (left + 1 + right) * 3) and got.dtype == np.float32
            idx = np.clip(np.arange(0, T, stride)[:, None] + np.arange(-left, right + 1)[None, :], 0, T - 1)  # a second writing
            assert np.array_equal(u32(got), u32(xs[idx].reshape(len(idx), -1)))
    assert np.isnan(clip(13, 40)).any() and np.isinf(clip(13, 40)).any() and (u32(clip(13, 40)) == 0x80000000).any()


@pytest.mark.parametrize("m,n", LFR)
def test_lfr_is_funasr_apply_lfr(m, n):
    left = (m - 1) // 2
    for T in (0, 1, 2, 5, 6, 7, 12, 13, 50):
        x = clip(5, T, seed=2)
        assert np.array_equal(u32(splice_ref(x, left, m - 1 - left, n)), u32(apply_lfr(x, m, n))), T


@pytest.mark.parametrize("left,right,stride", PARAMS)
def test_the_stream_model_equals_the_one_shot_model_however_it_is_cut(left, right, stride):
    """Random cuts of 0-3 periods, empty entries included, then flush: all rows, the first D dropped, are the one-shot rows bit for
    bit; the first D are +0.0; the pool row is the header's layout after every call."""
    rng = np.random.default_rng(1000 * left + 10 * right + stride)
    D, H = delay_hist(left, right, stride)
    for cols in (1, 5):
        for K in PERIODS:
            x = clip(cols, K * stride, seed=3)
            ref = splice_ref(x, left, right, stride)
            for _ in range(3):
                st, outs, pos = StreamModel(cols, left, right, stride), [], 0
                while pos < len(x):
                    r = int(rng.integers(0, 4)) * stride
                    outs.append(st.push(x[pos:pos + r]))
                    assert outs[-1].shape[0] == min(r, len(x) - pos) // stride
                    pos += r
                    row, seen = st.pool_row(), min(pos, len(x))
                    assert row.shape == (H * cols + 1,) and row[-1] == min(seen, H)
                    keep = min(seen, H)
                    assert np.array_equal(u32(row[(H - keep) * cols:-1]), u32(x[seen - keep:seen]).reshape(-1)) and not u32(row[:(H - keep) * cols]).any()
                outs += [st.push(x[:0]), st.flush()]
                got = np.concatenate(outs)
                assert got.shape == (K + D, ref.shape[1])
                assert not u32(got[:D]).any()  # warm-up rows: +0.0
                assert np.array_equal(u32(got[D:]), u32(ref)), (cols, K)
                assert len(st.hist) == 0 and not u32(st.pool_row()).any()


@pytest.mark.parametrize("left,right,stride", PARAMS)
def test_a_stream_that_ends_inside_a_period_repeats_its_last_row(left, right, stride):
    """The rule for a stream's end: the last row repeated up to a whole period, then the pool calls and the flush, give the packed
    call on the UNPADDED clip."""
    D, _ = delay_hist(left, right, stride)
    for T in sorted({1, 2, stride - 1, stride + 1, 3 * stride - 1, 4 * stride + 1} - {0}):
        x = clip(4, T, seed=4)
        pad = -T % stride
        padded = np.concatenate([x, np.repeat(x[-1:], pad, axis=0)])
        st = StreamModel(4, left, right, stride)
        cut = (len(padded) // stride // 2) * stride
        got = np.concatenate([st.push(padded[:cut]), st.push(padded[cut:]), st.flush()])
        assert np.array_equal(u32(got[D:]), u32(splice_ref(x, left, right, stride))), T


def test_symbols_are_declared_exported_and_prototyped(sslib):
    from speechsauce_amd import _lib

    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "speechsauce_amd.h")).read(), flags=re.S)
    for name, arity in NAMES.items():
        assert re.search(r"^int %s\(" % name, header, flags=re.M), name
        assert name in _lib.PROTOTYPES, name
        fn = getattr(sslib, name)
        assert fn.restype is C.c_int and len(fn.argtypes) == len(_lib.PROTOTYPES[name][1]) == arity, name
    assert sorted(n for n in _lib.PROTOTYPES if n.startswith("ss_splice_")) == sorted(NAMES)
    assert sslib.ss_abi_version() == 7  # entry points only: the version stays
    assert "inline std::vector<float> splice_packed(" in open(os.path.join(ROOT, "include", "speechsauce_amd.hpp")).read()


def test_packed_offsets_formula_and_rejections(sslib):
    rng = np.random.default_rng(5)
    for stride in (1, 2, 3, 6, 32):
        lens = np.concatenate([[0, 1, stride - 1, stride, stride + 1], rng.integers(0, 200, 20)])
        ro = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        oo = np.full(ro.size, -9, np.int64)
        assert sslib.ss_splice_packed_offsets(len(lens), ro.ctypes.data, stride, oo.ctypes.data) == 0
        assert np.array_equal(oo, np.concatenate([[0], np.cumsum(-(-lens // stride))]))
        same = ro.copy()  # in place
        assert sslib.ss_splice_packed_offsets(len(lens), same.ctypes.data, stride, same.ctypes.data) == 0 and np.array_equal(same, oo)
    ro = np.array([0, 5, 9], np.int64)
    oo = np.full(3, -9, np.int64)
    r, o = ro.ctypes.data, oo.ctypes.data
    assert sslib.ss_splice_packed_offsets(0, r, 3, o) == 0 and oo[0] == 0  # no clips: the one entry
    oo[:] = -9
    for bad in ((2, None, 3, o), (2, r, 3, None), (2, r, 0, o), (2, r, 33, o), (1 << 31, r, 3, o)):
        assert sslib.ss_splice_packed_offsets(*bad) == 3, bad
    dec = np.array([0, 5, 4, 9], np.int64)
    big = np.full(4, -9, np.int64)
    assert sslib.ss_splice_packed_offsets(3, dec.ctypes.data, 3, big.ctypes.data) == 3 and b"clip 1" in sslib.ss_last_error_string()
    assert (oo == -9).all() and (big == -9).all()  # a rejected call writes nothing


def _state_len(sslib, cols, left, right, stride):
    L, D = C.c_size_t(12345), C.c_size_t(54321)
    return sslib.ss_splice_stream_state_len(cols, left, right, stride, C.byref(L), C.byref(D)), L.value, D.value


def test_state_len_formula_and_rejections(sslib):
    for cols in (1, 13, 33, 80):
        for left, right, stride in PARAMS + ((32, 32, 1), (0, 32, 32)):
            D, H = delay_hist(left, right, stride)
            assert _state_len(sslib, cols, left, right, stride) == (0, H * cols + 1, D)
    assert _state_len(sslib, 13, 3, 3, 6) == (0, 3 * 13 + 1, 0) and _state_len(sslib, 13, 5, 5, 1) == (0, 10 * 13 + 1, 5)  # the header's examples
    assert _state_len(sslib, 7, 0, 0, 3) == (0, 1, 0)  # H = 0: the one count word
    for bad in ((0, 1, 1, 1), (13, 33, 0, 1), (13, 0, 33, 1), (13, 0, 0, 0), (13, 0, 0, 33), (13, 1 << 40, 0, 1), (1 << 31, 0, 0, 1)):
        assert _state_len(sslib, *bad) == (3, 12345, 54321), bad  # SS_ERR_ARG, the outputs untouched
    assert _state_len(sslib, 1 << 25, 32, 31, 1)[0] == 3            # W * cols reaches 2^31 (the state is never longer than a row)
    assert _state_len(sslib, (1 << 25) - 1, 32, 31, 1) == (0, 63 * ((1 << 25) - 1) + 1, 31)  # just below
    L = C.c_size_t()
    assert sslib.ss_splice_stream_state_len(13, 1, 1, 1, None, C.byref(L)) == 3 and sslib.ss_splice_stream_state_len(13, 1, 1, 1, C.byref(L), None) == 3


def test_argument_errors_are_decided_before_the_device_is_touched(sslib):
    """Every call here is rejected (or has nothing to do) on the host: none of the pointers is ever handed to the device, so host
    arrays stand in for device buffers.  On a host without a device a call that got past its checks would return SS_ERR_HIP."""
    cols, left, right, stride, rows, P = 13, 4, 7, 3, 12, 4
    D, H = delay_hist(left, right, stride)
    W = left + 1 + right
    len_ = H * cols + 1
    vec = np.ones((rows, cols), np.float32)
    out = np.full((max(rows, 2 * D), W * cols), -5.0, np.float32)  # also large enough for a flush of two entries
    pool = np.full((P, len_), -7.0, np.float32)
    off = np.array([0, 3, 12], np.int64)
    oo = np.array([0, 1, 4], np.int64)
    sl = np.array([1, 3], np.int32)
    v, o, p, r, q, s = vec.ctypes.data, out.ctypes.data, pool.ctypes.data, off.ctypes.data, oo.ctypes.data, sl.ctypes.data

    def packed_dev(vec=v, n=2, ro=r, total=rows, oo=q, total_out=4, cols=cols, left=left, right=right, stride=stride, out=o):
        return sslib.ss_splice_packed_device(vec, n, ro, total, oo, total_out, cols, left, right, stride, out, None)

    def packed_host(vec=v, n=2, ro=r, total=rows, cols=cols, left=left, right=right, stride=stride, out=o):
        return sslib.ss_splice_packed(vec, n, ro, total, cols, left, right, stride, out)

    def stream_dev(vec=v, n=2, ro=r, total=rows, sl=s, P=P, cols=cols, left=left, right=right, stride=stride, pool=p, out=o):
        return sslib.ss_splice_stream_packed_device(vec, n, ro, total, sl, P, cols, left, right, stride, pool, out, None)

    def stream_host(vec=v, n=2, ro=r, sl=s, P=P, cols=cols, left=left, right=right, stride=stride, pool=p, out=o):
        return sslib.ss_splice_stream_packed(vec, n, ro, sl, P, cols, left, right, stride, pool, out)

    def flush_dev(n=2, sl=s, P=P, cols=cols, left=left, right=right, stride=stride, pool=p, out=o):
        return sslib.ss_splice_stream_flush_device(n, sl, P, cols, left, right, stride, pool, out, None)

    def flush_host(n=2, sl=s, P=P, cols=cols, left=left, right=right, stride=stride, pool=p, out=o):
        return sslib.ss_splice_stream_flush(n, sl, P, cols, left, right, stride, pool, out)

    every = (packed_dev, packed_host, stream_dev, stream_host, flush_dev, flush_host)
    # an empty call is SS_OK with nothing launched, also without a device and whatever else is passed
    for call in every:
        assert call(n=0) == 0, call.__name__
    assert sslib.ss_splice_packed_device(None, 0, None, 0, None, 0, 0, 99, 99, 0, None, None) == 0
    assert sslib.ss_splice_packed(None, 0, None, 0, 0, 99, 99, 0, None) == 0
    assert sslib.ss_splice_stream_packed_device(None, 0, None, 0, None, 0, 0, 99, 99, 0, None, None, None) == 0
    assert sslib.ss_splice_stream_packed(None, 0, None, None, 0, 0, 99, 99, 0, None, None) == 0
    assert sslib.ss_splice_stream_flush_device(0, None, 0, 0, 99, 99, 0, None, None, None) == 0
    assert sslib.ss_splice_stream_flush(0, None, 0, 0, 99, 99, 0, None, None) == 0
    # the scalars every call shares
    for call in every:
        what = call.__name__
        assert call(cols=0) == 3, what
        assert call(left=33) == 3 and call(right=33) == 3 and call(left=1 << 40) == 3, what
        assert call(stride=0) == 3 and call(stride=33) == 3, what
        assert b"stride" in sslib.ss_last_error_string()
        assert call(n=1 << 31) == 3 and call(cols=1 << 31) == 3, what
        assert call(cols=1 << 27, left=8, right=7) == 3, what  # W * cols = 2^31
        assert call(out=None) == 3, what
    for call in (packed_dev, packed_host):
        for name in ("vec", "ro", "out"):
            assert call(**{name: None}) == 3, (call.__name__, name)
        assert call(total=1 << 31) == 3
        assert call(out=v) == 3 and b"in place" in sslib.ss_last_error_string()  # out must not overlap vec
        assert call(out=v + 4 * (rows * cols - 1)) == 3                         # ... not even in its last float
        assert call(out=v - 4 * (4 * W * cols - 1)) == 3                        # out has 4 rows of W * cols floats
    assert packed_dev(oo=None) == 3 and packed_dev(total_out=1 << 31) == 3
    assert packed_dev(out=v - 4 * (6 * W * cols - 1), total_out=6) == 3          # the device form's out is as long as the caller says
    for call in (stream_dev, stream_host):
        for name in ("vec", "ro", "sl", "pool", "out"):
            assert call(**{name: None}) == 3, (call.__name__, name)
        assert call(P=0) == 3 and call(P=1 << 31) == 3
        assert call(out=v) == 3 and call(out=v + 4 * cols) == 3
        assert call(pool=v) == 3 and call(pool=o) == 3 and call(pool=o + 4 * (4 * W * cols - 1)) == 3  # the pool overlapping vec / out
    assert stream_dev(total=1 << 31) == 3
    for call in (flush_dev, flush_host):
        for name in ("sl", "pool", "out"):
            assert call(**{name: None}) == 3, (call.__name__, name)
        assert call(P=0) == 3 and call(P=1 << 31) == 3
        assert call(pool=o) == 3 and call(pool=o + 4 * (2 * D * W * cols - 1)) == 3  # the pool overlapping the 2 * D rows of out
    # the host forms' table errors name the first bad clip / entry
    for bad, where in (([1, 2, 12], b"clip 0"), ([0, 4, 3], b"clip 1"), ([0, 2, 13], b"clip 1")):
        b = np.array(bad, np.int64)
        assert packed_host(ro=b.ctypes.data) == 3 and where in sslib.ss_last_error_string(), bad
    for bad, where in (([1, 3, 12], b"entry 0"), ([0, 6, 3], b"entry 1"), ([0, 3, 11], b"entry 1"), ([0, 4, 12], b"entry 0")):
        b = np.array(bad, np.int64)
        assert stream_host(ro=b.ctypes.data) == 3 and where in sslib.ss_last_error_string(), bad
    assert b"whole periods" in sslib.ss_last_error_string()
    for call in (stream_host, flush_host):
        for bad, where in (([1, 4], b"entry 1"), ([-1, 3], b"entry 0"), ([3, 3], b"entry 1")):
            b = np.array(bad, np.int32)
            assert call(sl=b.ctypes.data) == 3 and where in sslib.ss_last_error_string(), (call.__name__, bad)
            assert (b"outside the pool" if bad[0] != bad[1] else b"named twice") in sslib.ss_last_error_string()
    # clips / entries without rows only: nothing to do, no device needed
    z = np.zeros(3, np.int64)
    assert packed_host(ro=z.ctypes.data) == 0 and stream_host(ro=z.ctypes.data) == 0
    assert packed_dev(total=0) == 0 and packed_dev(total_out=0) == 0 and stream_dev(total=0) == 0
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

    x = np.zeros((6, 13), np.float32)
    for call in (lambda: ss.splice(x, 2, 2), lambda: ss.splice_packed(x, [0, 2, 6], 1, 1, 2), lambda: ss.lfr(x, 7, 6),
                 lambda: ss.lfr_packed(x, [0, 6], 7, 6)):
        with pytest.raises(SpeechSauceError) as e:
            call()
        assert e.value.status == 4  # SS_ERR_HIP: there is no CPU path
    m = ss.SpliceStreamPool(4, 13, 3, 3, 3)
    with pytest.raises(SpeechSauceError) as e:
        m(x, [0, 3, 6], [2, 0])
    assert e.value.status == 4
    assert m.state is None and not m.rows_seen.any()  # rows_seen moves only after a call went through


def test_python_argument_rules(sslib):
    import speechsauce_amd as ss

    for name in ("splice", "splice_packed", "lfr", "lfr_packed", "SpliceStreamPool"):
        assert name in ss.__all__ and hasattr(ss, name)
    z = lambda r, c=13, dt=np.float32: np.zeros((r, c), dt)  # noqa: E731
    for bad in (dict(left=-1, right=0), dict(left=33, right=0), dict(left=0, right=33), dict(left=0, right=-1), dict(left=1, right=1, stride=0),
                dict(left=1, right=1, stride=33)):
        with pytest.raises(ValueError):
            ss.splice(z(4), **bad)
        with pytest.raises(ValueError):
            ss.splice_packed(z(4), [0, 4], **bad)
        with pytest.raises(ValueError):
            ss.SpliceStreamPool(4, 13, **bad)
    for bad in ((0, 1), (66, 1), (7, 0), (7, 33)):
        with pytest.raises(ValueError):
            ss.lfr(z(4), *bad)
        with pytest.raises(ValueError):
            ss.lfr_packed(z(4), [0, 4], *bad)
    with pytest.raises(TypeError):
        ss.splice(z(4, dt=np.float64), 1, 1)
    with pytest.raises(ValueError):
        ss.splice(np.zeros(13, np.float32), 1, 1)  # not a matrix
    with pytest.raises(TypeError):
        ss.splice_packed(z(4, dt=np.float64), [0, 4], 1, 1)
    for bad_off in ([1, 4], [0, 3, 2], [0, 5]):
        with pytest.raises(ValueError):
            ss.splice_packed(z(4), bad_off, 1, 1)
    with pytest.raises(TypeError):
        ss.splice_packed(z(4), np.array([0.0, 4.0]), 1, 1)
    # no clip has a row: nothing for the device to do
    got, oo = ss.splice_packed(z(0), [0, 0, 0], 5, 5)
    assert got.shape == (0, 11 * 13) and got.dtype == np.float32 and oo.tolist() == [0, 0, 0] and oo.dtype == np.int64
    assert ss.splice(z(0), 3, 3, 6).shape == (0, 7 * 13) and ss.lfr(z(0), 7, 6).shape == (0, 7 * 13)
    assert ss.splice(np.zeros((2, 3, 0, 13), np.float32), 1, 0, 2).shape == (2, 3, 0, 26)

    m = ss.SpliceStreamPool(4, 13, 4, 7, 3)
    assert (m.pool_streams, m.cols, m.left, m.right, m.stride, m.delay_rows, m.state_len, m.out_cols) == (4, 13, 4, 7, 3, 2, 10 * 13 + 1, 12 * 13)
    assert m.state is None and m.rows_seen.dtype == np.int64 and m.rows_seen.shape == (4,) and not m.rows_seen.any()
    assert ss.SpliceStreamPool(2, 40, 3, 3, 6).delay_rows == 0 and ss.SpliceStreamPool(2, 40, 0, 0, 3).state_len == 1
    with pytest.raises(TypeError):
        m(z(3, dt=np.float64), [0, 3], [0])  # wrong dtype
    with pytest.raises(ValueError):
        m(np.zeros(39, np.float32), [0, 3], [0])  # not 2-D
    with pytest.raises(ValueError):
        m(z(3, 12), [0, 3], [0])  # wrong number of columns
    with pytest.raises(ValueError):
        m(z(3), [0, 3, 3], [0])  # table length
    with pytest.raises(ValueError):
        m(z(3), [0, 3], [4])  # a slot outside the pool
    with pytest.raises(ValueError):
        m(z(3), [0, 3], [-1])
    with pytest.raises(ValueError):
        m(z(3), [0, 3, 3], [1, 1])  # a slot named twice
    with pytest.raises(ValueError):
        m(z(3), [1, 3], [0])  # ro[0] != 0
    with pytest.raises(ValueError):
        m(z(6), [0, 6, 3], [0, 1])  # a decreasing pair
    with pytest.raises(ValueError):
        m(z(3), [0, 6], [0])  # past the block
    with pytest.raises(ValueError):
        m(z(6), [0, 2, 6], [0, 1])  # not whole periods
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
    f = m.flush([2, 0])  # before the first call there is no state anywhere: D rows of zeros each, no device needed
    assert f.shape == (2 * 2, 12 * 13) and not f.any() and m.state is None
    got = m(z(0), [0, 0, 0], [2, 3])  # entries without rows: no device needed
    assert got.shape == (0, 12 * 13) and not m.rows_seen.any()
    for bad in (dict(pool_streams=0, cols=13), dict(pool_streams=4, cols=0)):
        with pytest.raises(ValueError):
            ss.SpliceStreamPool(left=1, right=1, **bad)
    with pytest.raises(ss.SpeechSauceError) as e:
        ss.SpliceStreamPool(1, 1 << 25, 32, 32)
    assert e.value.status == 3
