"""Energy VAD and voiced-row selection (ss_vad_* / ss_select_rows_*), the part that needs no device: the numpy restatement of the
header's definition (tests/vad_model.py) against a worked example and second writings, the summation order of the mean against
ss_cmvn_packed_kernel's, the f32 product of the proportion rule, IEEE behaviour of NaN / inf energies, the numpy model of the pool over
random cuts, every argument error, the symbols and the Python front's argument rules."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from vad_model import PARAMS, VadStreamModel, causal_ref, cmvn_mean, cmvn_sum, decide, energies, select_ref, u32, vad_ref, window_mask
from splice_model import clip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"ss_vad_energy_packed_device": 13, "ss_vad_energy_packed": 12, "ss_select_rows_packed_device": 9, "ss_select_rows_packed": 8,
         "ss_vad_energy_stream_state_len": 2, "ss_vad_energy_stream_packed_device": 15, "ss_vad_energy_stream_packed": 13,
         "ss_vad_energy_stream_flush_device": 10, "ss_vad_energy_stream_flush": 9}


def test_the_worked_example_and_a_second_writing_of_the_window_count():
    e = np.array([3, 7, 7, 3, 3, 3, 7], np.float32)[:, None]
    assert vad_ref(e, 0, 5.0, 0.0, 1, 0.6).tolist() == [0, 1, 1, 0, 0, 0, 0]
    assert vad_ref(e[:0], 0, 5.0, 0.5, 1, 0.6).shape == (0,)
    rng = np.random.default_rng(1)
    for thr, scale, L, p in PARAMS:
        for T in (1, 2, L, L + 1, 2 * L + 1, 70):
            if T == 0:
                continue
            x = np.stack([rng.standard_normal(T), energies(T, seed=2)], axis=1).astype(np.float32)
            got = vad_ref(x, 1, thr, scale, L, p)
            th = np.float64(np.float32(thr)) + np.float64(np.float32(scale)) * cmvn_mean(x[:, 1]) if scale else np.float64(np.float32(thr))
            raw = (x[:, 1].astype(np.float64) > th).astype(np.int64)
            num = np.convolve(raw, np.ones(2 * L + 1, np.int64))[L:L + T]                    # a second writing: a box filter,
            den = np.convolve(np.ones(T, np.int64), np.ones(2 * L + 1, np.int64))[L:L + T]   # on the flags and on the clip's extent
            want = (num.astype(np.float32) >= den.astype(np.float32) * np.float32(p)).astype(np.uint8)
            assert got.dtype == np.uint8 and np.array_equal(got, want), (thr, scale, L, p, T)


def _kernel_order_mean(e):
    """ss_cmvn_packed_kernel's column sum restated from the kernel text, independently of vad_model: part[k] per chunk, then k ascending"""
    rows = len(e)
    chunks = min(64, (rows + 31) // 32)
    rpc = (rows + chunks - 1) // chunks
    part = []
    for chunk in range(chunks):
        r0 = chunk * rpc
        r1 = min(rows, r0 + rpc)
        s1 = np.float64(0.0)
        for r in range(r0, r1):
            s1 += np.float64(e[r])
        part.append(s1)
    s1 = np.float64(0.0)
    for k in range(chunks):
        s1 += part[k]
    return s1 / np.float64(rows)


@pytest.mark.parametrize("T", (1, 31, 32, 33, 2047, 2048, 2049, 5000))
def test_the_mean_is_the_cmvn_kernels_mean(T):
    e = energies(T, seed=3)
    mean = cmvn_mean(e)
    assert mean.dtype == np.float64
    assert u32(np.array([mean])).tolist() == u32(np.array([_kernel_order_mean(e)])).tolist()  # bit for bit
    ref = np.mean(e.astype(np.float64))
    assert abs(mean - ref) <= np.spacing(abs(ref))  # 1 ulp of numpy's pairwise float64 mean
    assert cmvn_sum(e).dtype == np.float64


def test_the_proportion_rule_is_one_f32_product():
    # den 5, p 0.6: 0.6f = 0.60000002384 lies above 0.6, and 5 * 0.6f = 3.00000011921 is exactly half way between the floats 3 and
    # 3.0000002, so the ONE f32 product rounds (to even) to 3.0: THREE voiced rows of five are enough, as in Kaldi's int x float.  A
    # product kept in f64 (3.0000001192 > 3) would say no: the case tells the two apart.
    assert np.float32(5) * np.float32(0.6) == np.float32(3) and np.float64(5) * np.float64(np.float32(0.6)) > 3
    assert decide(3, 5, 0.6) and not decide(2, 5, 0.6)
    e = np.array([9, 9, 9, 0, 0, 9, 9, 0, 0, 0, 0], np.float32)[:, None]
    got = vad_ref(e, 0, 5.0, 0.0, 2, 0.6)
    assert got[2] == 1  # t = 2: rows 0 .. 4 hold three voiced of five: 3 >= 3.0f
    assert got[1] == 1  # t = 1: rows 0 .. 3, three of four: 3 >= 2.4
    assert got.tolist() == [1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0]  # t = 3, 4: three of five again; t = 5 ..: two of five at the most
    # exact products: 4 * 0.5 = 2, 2 * 0.5 = 1
    assert decide(2, 4, 0.5) and not decide(1, 4, 0.5) and decide(1, 2, 0.5)
    # 10 * 0.3f (3.00000012 in f64) and 10 * 0.7f (6.99999988) round to the integers in f32 too
    assert np.float32(10) * np.float32(0.3) == np.float32(3) and decide(3, 10, 0.3) and not decide(2, 10, 0.3)
    assert np.float32(10) * np.float32(0.7) == np.float32(7) and decide(7, 10, 0.7) and not decide(6, 10, 0.7)
    # a product that does not round to an integer: 7 * 0.6f = 4.2000003
    assert not decide(4, 7, 0.6) and decide(5, 7, 0.6)


def test_nan_and_inf_energies_follow_ieee():
    e = np.array([9, np.nan, 9, 1, np.inf, -np.inf, 9], np.float32)[:, None]
    # scale == 0: the mean is not formed, the NaN row itself compares false, nothing else notices it
    assert vad_ref(e, 0, 5.0, 0.0, 0, 0.6).tolist() == [1, 0, 1, 0, 1, 0, 1]
    # scale != 0: the mean is NaN (NaN, and inf - inf), every raw decision is false
    assert not vad_ref(e, 0, 5.0, 0.5, 0, 0.6).any() and not vad_ref(e, 0, 5.0, 0.5, 2, 0.12).any()
    f = np.array([9, 1, np.inf, 9], np.float32)[:, None]
    assert not vad_ref(f, 0, 5.0, 0.5, 0, 0.6).any()        # mean = +inf: nothing is above it, not even +inf
    g = np.array([9, 1, -np.inf, 1], np.float32)[:, None]
    assert vad_ref(g, 0, 5.0, 0.5, 0, 0.6).tolist() == [1, 1, 0, 1]  # mean = -inf: everything finite is above it
    # the other columns are never looked at
    x = clip(5, 40, seed=4).copy()
    x[:, 3] = energies(40, seed=4)
    y = np.zeros_like(x)
    y[:, 3] = x[:, 3]
    assert np.isnan(x).any() and np.array_equal(vad_ref(x, 3, 5.0, 0.5, 2, 0.3), vad_ref(y, 3, 5.0, 0.5, 2, 0.3))


def test_select_ref():
    x = clip(3, 10, seed=5)
    m = np.array([0, 1, 2, 0, 255, 0, 0, 1, 0, 1], np.uint8)
    out, oo = select_ref(x, [0, 4, 4, 10], m)
    assert oo.tolist() == [0, 2, 2, 5] and oo.dtype == np.int64
    assert np.array_equal(u32(out), u32(x[[1, 2, 4, 7, 9]]))


def _run_stream(model, x, rng):
    """random cuts of 0 - 3 rows (empties included), one more empty entry, then the flush -> all bytes, the pool row before the flush"""
    outs, pos = [], 0
    while pos < len(x):
        r = int(rng.integers(0, 4))
        outs.append(model.push(x[pos:pos + r]))
        assert outs[-1].shape == (min(r, len(x) - pos),)
        pos += r
    outs.append(model.push(x[:0]))
    row = model.pool_row()
    outs.append(model.flush())
    return np.concatenate(outs), row


@pytest.mark.parametrize("thr,scale,L,p", PARAMS)
def test_the_stream_model_over_random_cuts(thr, scale, L, p):
    """scale == 0: all bytes, the first L dropped, are vad_ref byte for byte.  scale != 0: they are the causal formula's bytes.
    Either way the bytes and the pool row do not depend on the cut, the first L bytes are 0 and the pool row has the header's layout."""
    rng = np.random.default_rng(int(1000 * abs(thr)) + 10 * L)
    for T in (0, 1, 2, L, L + 1, 2 * L + 1, 3 * L + 5, 71):
        x = np.stack([energies(T, seed=6), energies(T, seed=7, centre=0.0)], axis=1) if T else np.zeros((0, 2), np.float32)
        for sc in (scale, 0.0):
            runs = [_run_stream(VadStreamModel(0, thr, sc, L, p), x, rng) for _ in range(3)]
            got, row = runs[0]
            assert got.shape == (T + L,) and got.dtype == np.uint8 and not got[:L].any()
            for other, other_row in runs[1:]:
                assert np.array_equal(got, other) and np.array_equal(u32(row), u32(other_row))
            assert np.array_equal(got[L:], causal_ref(x[:, 0], thr, sc, L, p)), (T, sc)
            if sc == 0:
                assert np.array_equal(got[L:], vad_ref(x, 0, thr, sc, L, p)), T
            keep = min(T, 2 * L)
            assert row.shape == (2 * L + 4,) and row[-1] == keep and u32(row)[2] == T
            assert np.array_equal(u32(row[3 + 2 * L - keep:-1]), u32(x[T - keep:, 0])) and not u32(row[3:3 + 2 * L - keep]).any()
            s = np.cumsum(x[:, 0].astype(np.float64))[-1] if T else np.float64(0)
            assert u32(row)[:2].tolist() == u32(np.array([s])).tolist()
    m = VadStreamModel(0, thr, scale, L, p)
    assert not u32(m.pool_row()).any()  # a fresh stream is all zeros


def test_symbols_are_declared_exported_and_prototyped(sslib):
    from speechsauce_amd import _lib

    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "speechsauce_amd.h")).read(), flags=re.S)
    for name, arity in NAMES.items():
        assert re.search(r"^int %s\(" % name, header, flags=re.M), name
        assert name in _lib.PROTOTYPES, name
        fn = getattr(sslib, name)
        assert fn.restype is C.c_int and len(fn.argtypes) == len(_lib.PROTOTYPES[name][1]) == arity, name
    assert sorted(n for n in _lib.PROTOTYPES if n.startswith(("ss_vad_", "ss_select_rows_"))) == sorted(NAMES)
    assert sslib.ss_abi_version() == 7  # entry points only: the version stays
    hpp = open(os.path.join(ROOT, "include", "speechsauce_amd.hpp")).read()
    assert "inline std::vector<uint8_t> vad_energy_packed(" in hpp and "inline std::vector<float> select_rows_packed(" in hpp
    full = open(os.path.join(ROOT, "include", "speechsauce_amd.h")).read()
    assert "DEPARTURE FROM KALDI" in full and "2^32 - 1 rows is out of contract" in full


def test_state_len_formula_and_rejections(sslib):
    for L in (0, 1, 2, 32):
        n = C.c_size_t(12345)
        assert sslib.ss_vad_energy_stream_state_len(L, C.byref(n)) == 0 and n.value == 2 * L + 4
    n = C.c_size_t(12345)
    assert sslib.ss_vad_energy_stream_state_len(33, C.byref(n)) == 3 and sslib.ss_vad_energy_stream_state_len(1 << 40, C.byref(n)) == 3
    assert n.value == 12345 and sslib.ss_vad_energy_stream_state_len(2, None) == 3


def test_argument_errors_are_decided_before_the_device_is_touched(sslib):
    """Every call here is rejected (or has nothing to do) on the host: none of the pointers is ever handed to the device, so host
    arrays stand in for device buffers.  On a host without a device a call that got past its checks would return SS_ERR_HIP."""
    cols, rows, P, L = 13, 12, 4, 2
    vec = np.ones((rows, cols), np.float32)
    out = np.full((rows, cols), -5.0, np.float32)
    mask = np.full(rows, 0xA5, np.uint8)
    counts = np.full(2, -9, np.int64)
    oo = np.full(3, -9, np.int64)
    pool = np.full((P, 2 * L + 4), -7.0, np.float32)
    off = np.array([0, 3, 12], np.int64)
    sl = np.array([1, 3], np.int32)
    v, o, m, c, q, p, r, s = (a.ctypes.data for a in (vec, out, mask, counts, oo, pool, off, sl))
    nan, inf = float("nan"), float("inf")

    def vad_dev(vec=v, n=2, ro=r, total=rows, cols=cols, col=0, thr=5.0, scale=0.5, L=L, prop=0.6, mask=m, counts=c):
        return sslib.ss_vad_energy_packed_device(vec, n, ro, total, cols, col, thr, scale, L, prop, mask, counts, None)

    def vad_host(vec=v, n=2, ro=r, total=rows, cols=cols, col=0, thr=5.0, scale=0.5, L=L, prop=0.6, mask=m, counts=c):
        return sslib.ss_vad_energy_packed(vec, n, ro, total, cols, col, thr, scale, L, prop, mask, counts)

    def sel_dev(vec=v, n=2, ro=r, total=rows, cols=cols, mask=m, oo=q, out=o):
        return sslib.ss_select_rows_packed_device(vec, n, ro, total, cols, mask, oo, out, None)

    def sel_host(vec=v, n=2, ro=r, total=rows, cols=cols, mask=m, oo=q, out=o):
        return sslib.ss_select_rows_packed(vec, n, ro, total, cols, mask, oo, out)

    def stream_dev(vec=v, n=2, ro=r, total=rows, sl=s, P=P, cols=cols, col=0, thr=5.0, scale=0.5, L=L, prop=0.6, pool=p, mask=m):
        return sslib.ss_vad_energy_stream_packed_device(vec, n, ro, total, sl, P, cols, col, thr, scale, L, prop, pool, mask, None)

    def stream_host(vec=v, n=2, ro=r, sl=s, P=P, cols=cols, col=0, thr=5.0, scale=0.5, L=L, prop=0.6, pool=p, mask=m):
        return sslib.ss_vad_energy_stream_packed(vec, n, ro, sl, P, cols, col, thr, scale, L, prop, pool, mask)

    def flush_dev(n=2, sl=s, P=P, thr=5.0, scale=0.5, L=L, prop=0.6, pool=p, mask=m):
        return sslib.ss_vad_energy_stream_flush_device(n, sl, P, thr, scale, L, prop, pool, mask, None)

    def flush_host(n=2, sl=s, P=P, thr=5.0, scale=0.5, L=L, prop=0.6, pool=p, mask=m):
        return sslib.ss_vad_energy_stream_flush(n, sl, P, thr, scale, L, prop, pool, mask)

    every = (vad_dev, vad_host, sel_dev, sel_host, stream_dev, stream_host, flush_dev, flush_host)
    deciding = (vad_dev, vad_host, stream_dev, stream_host, flush_dev, flush_host)
    # an empty call is SS_OK with nothing launched, also without a device and whatever else is passed
    for call in every:
        assert call(n=0) == 0, call.__name__
    assert sslib.ss_vad_energy_packed_device(None, 0, None, 0, 0, 9, nan, nan, 99, 7.0, None, None, None) == 0
    assert sslib.ss_vad_energy_packed(None, 0, None, 0, 0, 9, nan, nan, 99, 7.0, None, None) == 0
    assert sslib.ss_select_rows_packed_device(None, 0, None, 0, 0, None, None, None, None) == 0
    assert sslib.ss_select_rows_packed(None, 0, None, 0, 0, None, None, None) == 0
    assert sslib.ss_vad_energy_stream_packed_device(None, 0, None, 0, None, 0, 0, 9, nan, nan, 99, 7.0, None, None, None) == 0
    assert sslib.ss_vad_energy_stream_packed(None, 0, None, None, 0, 0, 9, nan, nan, 99, 7.0, None, None) == 0
    assert sslib.ss_vad_energy_stream_flush_device(0, None, 0, nan, nan, 99, 7.0, None, None, None) == 0
    assert sslib.ss_vad_energy_stream_flush(0, None, 0, nan, nan, 99, 7.0, None, None) == 0
    # the scalars of the decision
    for call in deciding:
        what = call.__name__
        assert call(L=33) == 3 and call(L=1 << 40) == 3, what
        assert b"frames_context" in sslib.ss_last_error_string()
        for bad in (0.0, 1.0, -0.1, 1.5, nan, inf, -inf):
            assert call(prop=bad) == 3, (what, bad)
        assert b"proportion_threshold" in sslib.ss_last_error_string()
        for bad in (nan, inf, -inf):
            assert call(thr=bad) == 3 and call(scale=bad) == 3, (what, bad)
        assert call(mask=None) == 3, what
        assert call(n=1 << 31) == 3, what
    for call in (vad_dev, vad_host, stream_dev, stream_host):
        what = call.__name__
        assert call(cols=0) == 3 and call(cols=1 << 31) == 3, what
        assert call(col=cols) == 3 and call(col=1 << 40) == 3, what
        assert b"energy_col" in sslib.ss_last_error_string()
        assert call(vec=None) == 3 and call(ro=None) == 3, what
    assert vad_dev(total=1 << 31) == 3 and vad_host(total=1 << 31) == 3 and stream_dev(total=1 << 31) == 3
    # the selection
    for call in (sel_dev, sel_host):
        what = call.__name__
        for name in ("vec", "ro", "mask", "oo", "out"):
            assert call(**{name: None}) == 3, (what, name)
        assert call(cols=0) == 3 and call(cols=1 << 31) == 3 and call(total=1 << 31) == 3 and call(n=1 << 31) == 3, what
        assert call(out=v) == 3 and b"in place" in sslib.ss_last_error_string()  # out must not overlap vec
        assert call(out=v + 4 * (rows * cols - 1)) == 3 and call(out=v - 4 * (rows * cols - 1)) == 3  # ... not even in one float
        assert call(mask=o + 4 * rows * cols - 1) == 3 and b"mask" in sslib.ss_last_error_string()  # ... nor the mask, in one byte
        assert call(mask=o - rows + 1) == 3
    # the pool
    for call in (stream_dev, stream_host, flush_dev, flush_host):
        what = call.__name__
        assert call(sl=None) == 3 and call(pool=None) == 3, what
        assert call(P=0) == 3 and call(P=1 << 31) == 3, what
        assert call(pool=m - 4) == 3 and b"pool overlaps" in sslib.ss_last_error_string(), what  # the pool overlapping the mask
    for call in (stream_dev, stream_host):
        assert call(pool=v) == 3 and call(mask=v) == 3 and call(mask=v + 4 * rows * cols - 1) == 3, call.__name__
    # the host forms' table errors name the first bad clip / entry
    for call in (vad_host, sel_host):
        for bad, where in (([1, 2, 12], b"clip 0"), ([0, 4, 3], b"clip 1"), ([0, 2, 13], b"clip 1")):
            b = np.array(bad, np.int64)
            assert call(ro=b.ctypes.data) == 3 and where in sslib.ss_last_error_string(), (call.__name__, bad)
    for bad, where in (([1, 3, 12], b"entry 0"), ([0, 6, 3], b"entry 1")):
        b = np.array(bad, np.int64)
        assert stream_host(ro=b.ctypes.data) == 3 and where in sslib.ss_last_error_string(), bad
    for call in (stream_host, flush_host):
        for bad, where in (([1, 4], b"entry 1"), ([-1, 3], b"entry 0"), ([3, 3], b"entry 1")):
            b = np.array(bad, np.int32)
            assert call(sl=b.ctypes.data) == 3 and where in sslib.ss_last_error_string(), (call.__name__, bad)
            assert (b"outside the pool" if bad[0] != bad[1] else b"named twice") in sslib.ss_last_error_string()
    assert (out == -5.0).all() and (mask == 0xA5).all() and (counts == -9).all() and (oo == -9).all() and (pool == -7.0).all() and (vec == 1.0).all()
    # clips / entries without rows only: nothing to do, no device needed; the host forms still answer the tables
    z = np.zeros(3, np.int64)
    assert vad_host(ro=z.ctypes.data) == 0 and counts.tolist() == [0, 0]
    assert sel_host(ro=z.ctypes.data) == 0 and oo.tolist() == [0, 0, 0]
    assert stream_host(ro=z.ctypes.data) == 0 and stream_dev(total=0) == 0
    assert (out == -5.0).all() and (mask == 0xA5).all() and (pool == -7.0).all()


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
    keep = np.ones(6, np.uint8)
    for call in (lambda: ss.vad_energy(x), lambda: ss.vad_energy_packed(x, [0, 2, 6], 0, 5.5, 0.5, 2, 0.12), lambda: ss.select_rows(x, keep),
                 lambda: ss.select_rows_packed(x, [0, 6], keep), lambda: ss.select_rows_packed(x, [0, 6], keep, trim=False)):
        with pytest.raises(SpeechSauceError) as e:
            call()
        assert e.value.status == 4  # SS_ERR_HIP: there is no CPU path
    m = ss.VadEnergyStreamPool(4, 13, frames_context=2)
    with pytest.raises(SpeechSauceError) as e:
        m(x, [0, 3, 6], [2, 0])
    assert e.value.status == 4
    assert m.state is None and not m.rows_seen.any()  # rows_seen moves only after a call went through


def test_python_argument_rules(sslib):
    import speechsauce_amd as ss

    for name in ("vad_energy", "vad_energy_packed", "select_rows", "select_rows_packed", "VadEnergyStreamPool"):
        assert name in ss.__all__ and hasattr(ss, name)
    z = lambda r, c=13, dt=np.float32: np.zeros((r, c), dt)  # noqa: E731
    for bad in (dict(energy_col=13), dict(energy_col=-1), dict(frames_context=33), dict(frames_context=-1), dict(proportion_threshold=0.0),
                dict(proportion_threshold=1.0), dict(proportion_threshold=float("nan")), dict(energy_threshold=float("inf")),
                dict(energy_mean_scale=float("nan"))):
        with pytest.raises(ValueError):
            ss.vad_energy(z(4), **bad)
        with pytest.raises(ValueError):
            ss.vad_energy_packed(z(4), [0, 4], **bad)
        with pytest.raises(ValueError):
            ss.VadEnergyStreamPool(4, 13, **bad)
    with pytest.raises(TypeError):
        ss.vad_energy(z(4, dt=np.float64))
    with pytest.raises(ValueError):
        ss.vad_energy(np.zeros(13, np.float32))  # not a matrix
    with pytest.raises(TypeError):
        ss.vad_energy_packed(z(4, dt=np.float64), [0, 4])
    for bad_off in ([1, 4], [0, 3, 2], [0, 5]):
        with pytest.raises(ValueError):
            ss.vad_energy_packed(z(4), bad_off)
        with pytest.raises(ValueError):
            ss.select_rows_packed(z(4), bad_off, np.ones(4, np.uint8))
    with pytest.raises(TypeError):
        ss.vad_energy_packed(z(4), np.array([0.0, 4.0]))
    with pytest.raises(TypeError):
        ss.select_rows_packed(z(4), [0, 4], np.ones(4, np.float32))  # a float mask
    with pytest.raises(TypeError):
        ss.select_rows_packed(z(4, dt=np.float64), [0, 4], np.ones(4, np.uint8))
    with pytest.raises(ValueError):
        ss.select_rows_packed(z(4), [0, 4], np.ones(5, np.uint8))  # one entry per row
    with pytest.raises(ValueError):
        ss.select_rows_packed(z(4), [0, 4], np.ones((4, 1), np.uint8))
    with pytest.raises(ValueError):
        ss.select_rows(np.zeros(13, np.float32), np.ones(13, np.uint8))
    # no clip has a row: nothing for the device to do
    mask, counts = ss.vad_energy_packed(z(0), [0, 0, 0])
    assert mask.shape == (0,) and mask.dtype == np.uint8 and counts.tolist() == [0, 0] and counts.dtype == np.int64
    assert ss.vad_energy(z(0)).shape == (0,) and ss.vad_energy(z(0)).dtype == bool
    assert ss.vad_energy(np.zeros((2, 3, 0, 13), np.float32)).shape == (2, 3, 0)
    out, oo = ss.select_rows_packed(z(0), [0, 0, 0], np.zeros(0, np.uint8))
    assert out.shape == (0, 13) and out.dtype == np.float32 and oo.tolist() == [0, 0, 0] and oo.dtype == np.int64
    assert ss.select_rows(z(0), np.zeros(0, bool)).shape == (0, 13)

    m = ss.VadEnergyStreamPool(4, 13, 12, 5.5, 0.5, 2, 0.12)
    assert (m.pool_streams, m.cols, m.energy_col, m.frames_context, m.delay_rows, m.state_len) == (4, 13, 12, 2, 2, 8)
    assert m.state is None and m.rows_seen.dtype == np.int64 and m.rows_seen.shape == (4,) and not m.rows_seen.any()
    assert ss.VadEnergyStreamPool(2, 40).delay_rows == 0 and ss.VadEnergyStreamPool(2, 40).state_len == 4
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
        m(z(3), [0, 3, 3], [1, 1])  # a slot named twice
    with pytest.raises(ValueError):
        m(z(3), [1, 3], [0])  # ro[0] != 0
    with pytest.raises(ValueError):
        m(z(6), [0, 6, 3], [0, 1])  # a decreasing pair
    with pytest.raises(ValueError):
        m(z(3), [0, 6], [0])  # past the block
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
    f = m.flush([2, 0])  # before the first call there is no state anywhere: L zero bytes each, no device needed
    assert f.shape == (4,) and f.dtype == np.uint8 and not f.any() and m.state is None
    got = m(z(0), [0, 0, 0], [2, 3])  # entries without rows: no device needed
    assert got.shape == (0,) and got.dtype == np.uint8 and not m.rows_seen.any()
    for bad in (dict(pool_streams=0, cols=13), dict(pool_streams=4, cols=0)):
        with pytest.raises(ValueError):
            ss.VadEnergyStreamPool(**bad)
