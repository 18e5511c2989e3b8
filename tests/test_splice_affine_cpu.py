"""The fused splice + affine transform (ss_affine_*, ss_affine_splice_packed*), the part that needs no device: the numpy fmaf of
tests/affine_model.py against libm's, the model chain against its f64 restatement within the derived bar, the host-only calls, every
argument rule that is decided before the device is touched, the symbols and the Python front's argument rules."""
import ctypes as C
import ctypes.util
import os
import re

import numpy as np
import pytest

from affine_model import SHAPES, affine_f64, affine_ref, block, chain, chain_len, fmaf, matrix, rows, u32

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"ss_affine_create": 6, "ss_affine_destroy": 1, "ss_affine_dims": 3, "ss_affine_chain_len": 2, "ss_affine_splice_packed_device": 13,
         "ss_affine_splice_packed": 10}
OK, ARG, UNSUPPORTED = 0, 3, 5


def _libm_fmaf():
    libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    libm.fmaf.restype = C.c_float
    libm.fmaf.argtypes = [C.c_float] * 3
    return libm.fmaf


def test_the_numpy_fmaf_is_libm_fmaf():
    """10^5 seeded triples: wide-exponent values, then the hard cases -- products that cancel the addend almost or wholly, exact ties
    of the f32 rounding (a * b = an odd multiple of half an ulp of c), denormal results, -0.0 and infinities."""
    ref = _libm_fmaf()
    rng = np.random.default_rng(11)
    n = 25000
    wide = lambda: (rng.standard_normal(n) * 2.0 ** rng.integers(-60, 60, n)).astype(np.float32)  # noqa: E731
    a, b, c = [wide()], [wide()], [wide()]
    x, y = wide(), wide()
    a.append(x), b.append(y), c.append((-(x.astype(np.float64) * y).astype(np.float32)))  # cancellation: the product's low half is the result
    m = rng.integers(1 << 23, 1 << 24, n).astype(np.float32)                               # ties: c = m (24 bits), a * b = +-(odd) / 2
    a.append((2 * rng.integers(0, 1 << 10, n) + 1).astype(np.float32)), b.append(np.where(rng.random(n) < 0.5, 0.5, -0.5).astype(np.float32)), c.append(m)
    tiny = (rng.standard_normal(n) * 2.0 ** rng.integers(-80, -60, n)).astype(np.float32)  # denormal and underflowing results
    spec = rng.choice(np.array([0.0, -0.0, np.inf, -np.inf, 1e-45, -1e-45, 3e38], np.float32), n)
    a.append(tiny), b.append(wide() * np.float32(2.0 ** -70)), c.append(np.where(rng.random(n) < 0.5, spec, np.float32(1e-44) * rng.integers(-9, 9, n)).astype(np.float32))
    a, b, c = (np.concatenate(v) for v in (a, b, c))
    assert a.size == 100000
    got = fmaf(a, b, c)
    want = np.array([ref(float(p), float(q), float(r)) for p, q, r in zip(a, b, c)], np.float32)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan)
    bad = np.flatnonzero((u32(got) != u32(want)) & ~nan)
    assert bad.size == 0, (bad[:5], a[bad[:5]], b[bad[:5]], c[bad[:5]])
    assert (np.abs(want[~nan]) < 1.2e-38).sum() > 1000 and (u32(want) == 0x80000000).any()  # denormal results and -0.0 were met


def test_the_pad_steps_are_part_of_the_chain():
    """K = 1 -> K4 = 4: a -0.0 bias under a product of -0.0 stays -0.0 through the first step and is +0.0 after the pad steps."""
    assert [chain_len(k) for k in (1, 3, 4, 5, 91, 440, 4096)] == [4, 4, 4, 8, 92, 440, 4096]
    s, M = np.array([[1.0]], np.float32), np.array([[-0.0]], np.float32)
    assert u32(fmaf(M[0, 0], s[0, 0], np.float32(-0.0))) == 0x80000000
    assert u32(chain(s, M, np.array([-0.0], np.float32)))[0, 0] == 0           # fmaf(+0, +0, -0.0) = +0.0
    assert u32(chain(np.ones((1, 4), np.float32), np.full((1, 4), -0.0, np.float32), np.array([-0.0], np.float32)))[0, 0] == 0x80000000  # K = K4: no pad


@pytest.mark.parametrize("shape", SHAPES)
def test_the_chain_is_within_the_bar_of_its_f64_restatement(shape):
    cols, left, right, stride, out_dim = shape
    M, bias = matrix(out_dim, (left + 1 + right) * cols, denormals=False)  # the bar is one of relative roundings: no underflow
    worst = 0.0
    for x in block(cols, denormals=False)[0]:
        if not len(x):
            continue
        got = affine_ref(x, M, bias, left, right, stride)
        ref, bar = affine_f64(x, M, bias, left, right, stride)
        assert got.shape == ref.shape == (-(-len(x) // stride), out_dim) and got.dtype == np.float32
        assert (np.abs(got - ref) <= bar).all()
        worst = max(worst, float((np.abs(got - ref) / np.maximum(bar, 1e-300)).max()))
    assert worst < 0.5  # roundings do not all point one way: the bar is not tight


def test_symbols_are_declared_exported_and_prototyped(sslib):
    from speechsauce_amd import _lib

    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "speechsauce_amd.h")).read(), flags=re.S)
    for name, arity in NAMES.items():
        assert re.search(r"^(int|void) %s\(" % name, header, flags=re.M), name
        assert name in _lib.PROTOTYPES, name
        fn = getattr(sslib, name)
        assert len(fn.argtypes) == len(_lib.PROTOTYPES[name][1]) == arity, name
    assert sorted(n for n in _lib.PROTOTYPES if n.startswith("ss_affine_")) == sorted(NAMES)
    assert "typedef struct ss_affine ss_affine;" in header
    assert sslib.ss_abi_version() == 7  # entry points only: the version stays
    assert "class Affine {" in open(os.path.join(ROOT, "include", "speechsauce_amd.hpp")).read()
    shim = open(os.path.join(ROOT, "mfcc-rust_amd", "rust-shim", "src", "lib.rs")).read()
    for name in NAMES:
        assert "fn %s(" % name in shim, name


def test_chain_len_formula_and_limits(sslib):
    k4 = C.c_size_t(77)
    for k in (1, 2, 3, 4, 5, 91, 92, 440, 441, 4093, 4096):
        assert sslib.ss_affine_chain_len(k, C.byref(k4)) == OK and k4.value == chain_len(k)
    k4.value = 77
    assert sslib.ss_affine_chain_len(0, C.byref(k4)) == UNSUPPORTED and sslib.ss_affine_chain_len(4097, C.byref(k4)) == UNSUPPORTED
    assert sslib.ss_affine_chain_len(8, None) == ARG and k4.value == 77


def _create(lib, M, bias=None, ld=None):
    h = C.c_void_p()
    rc = lib.ss_affine_create(M.ctypes.data, M.shape[0], M.shape[1], M.shape[1] if ld is None else ld, None if bias is None else bias.ctypes.data,
                              C.byref(h))
    return rc, h


def test_create_limits_are_decided_without_a_device(sslib):
    M = np.zeros((256, 4096), np.float32)
    h = C.c_void_p(1)
    for out_dim, in_dim in ((0, 8), (257, 8), (8, 0), (8, 4097), (1 << 40, 1 << 40)):
        h.value = 1
        assert sslib.ss_affine_create(M.ctypes.data, out_dim, in_dim, max(in_dim, 1), None, C.byref(h)) == UNSUPPORTED, (out_dim, in_dim)
        assert not h.value  # the output is cleared
    assert sslib.ss_affine_create(None, 0, 8, 8, None, C.byref(h)) == UNSUPPORTED  # the limits come first
    assert sslib.ss_affine_create(None, 8, 8, 8, None, C.byref(h)) == ARG
    assert sslib.ss_affine_create(M.ctypes.data, 8, 8, 7, None, C.byref(h)) == ARG and b"ld" in sslib.ss_last_error_string()
    assert sslib.ss_affine_create(M.ctypes.data, 8, 8, 8, None, None) == ARG
    for out_dim, in_dim in ((1, 1), (256, 4096), (40, 441)):
        assert sslib.ss_affine_create(M.ctypes.data, out_dim, in_dim, 4096, None, C.byref(h)) == OK and h.value
        o, i = C.c_size_t(), C.c_size_t()
        assert sslib.ss_affine_dims(h, C.byref(o), C.byref(i)) == OK and (o.value, i.value) == (out_dim, in_dim)
        assert sslib.ss_affine_dims(h, None, C.byref(i)) == ARG and sslib.ss_affine_dims(None, C.byref(o), C.byref(i)) == ARG
        sslib.ss_affine_destroy(h)
    sslib.ss_affine_destroy(None)  # a null handle is nothing to destroy


def test_every_argument_error_is_decided_before_the_device(sslib):
    cols, left, right, stride, out_dim = 13, 3, 3, 1, 40
    M, bias = matrix(out_dim, 91)
    rc, h = _create(sslib, M, bias)
    assert rc == OK
    x = np.zeros((50, cols), np.float32)
    out = np.zeros((50, out_dim), np.float32)
    ro = np.array([0, 20, 50], np.int64)
    X, O, R = x.ctypes.data, out.ctypes.data, ro.ctypes.data
    dev = lambda **k: sslib.ss_affine_splice_packed_device(*[k.get(n, d) for n, d in (  # noqa: E731
        ("t", h), ("vec", X), ("n", 2), ("ro", R), ("rows", 50), ("oo", R), ("orows", 50), ("cols", cols), ("left", left), ("right", right),
        ("stride", stride), ("out", O), ("stream", None))])
    host = lambda **k: sslib.ss_affine_splice_packed(*[k.get(n, d) for n, d in (  # noqa: E731
        ("t", h), ("vec", X), ("n", 2), ("ro", R), ("rows", 50), ("cols", cols), ("left", left), ("right", right), ("stride", stride), ("out", O))])
    for call in (dev, host):
        assert call(n=0) == OK and call(n=0, vec=None, out=None, t=None) == OK  # no clips: nothing to do, nothing looked at
        for null in ("t", "vec", "ro", "out"):
            assert call(**{null: None}) == ARG, null
        assert call(cols=0) == ARG
        assert call(left=33) == ARG and call(right=33) == ARG and call(stride=0) == ARG and call(stride=33) == ARG
        assert call(n=1 << 31) == ARG and call(rows=1 << 31) == ARG and call(cols=1 << 31) == ARG
        assert call(cols=14) == ARG and b"91" in sslib.ss_last_error_string()       # in_dim != (left + 1 + right) * cols
        assert call(left=2) == ARG and call(right=4) == ARG
        assert call(out=X) == ARG and b"overlaps" in sslib.ss_last_error_string()  # not in place
        assert call(out=X + 4 * (50 * cols - 1)) == ARG
    assert dev(oo=None) == ARG and dev(orows=1 << 31) == ARG
    # the host form checks its table first and names the first bad clip
    for bad, word in ((np.array([1, 20, 50], np.int64), b"offsets[0]"), (np.array([0, 30, 20], np.int64), b"clip 1"),
                      (np.array([0, 20, 51], np.int64), b"clip 1")):
        assert host(ro=bad.ctypes.data) == ARG and word in sslib.ss_last_error_string(), bad
    assert host(ro=np.zeros(3, np.int64).ctypes.data) == OK  # clips without rows: no device needed
    assert not out.any()
    sslib.ss_affine_destroy(h)


def test_the_python_front_checks_its_arguments(sslib):
    import speechsauce_amd as ss

    M, bias = matrix(40, 91)
    t = ss.Affine(M, bias)
    assert (t.out_dim, t.in_dim, t.chain_len) == (40, 91, 92)
    assert ss.Affine(np.asfortranarray(M)).in_dim == 91  # any layout: the front makes it row-major
    with pytest.raises(TypeError):
        ss.Affine(M.astype(np.float64))
    with pytest.raises(ValueError):
        ss.Affine(M, bias[:-1])
    with pytest.raises(ValueError):
        ss.Affine(M[0])
    with pytest.raises(ss.SpeechSauceError) as e:
        ss.Affine(np.zeros((257, 4), np.float32))
    assert e.value.status == UNSUPPORTED
    x = rows(13, 20)
    with pytest.raises(ValueError):
        ss.splice_affine_packed(x, [0, 20], t, 3, 2)           # 6 * 13 != 91
    with pytest.raises(ValueError):
        ss.splice_affine_packed(x, [0, 20], t, 3, 33)
    with pytest.raises(TypeError):
        ss.splice_affine_packed(x, [0, 20], M, 3, 3)
    with pytest.raises(ValueError):
        ss.splice_affine_packed(x, [0, 21], t, 3, 3)           # the table ends past the block
    out, oo = ss.splice_affine_packed(x[:0], [0, 0, 0], t, 3, 3)  # no rows: no device needed
    assert out.shape == (0, 40) and oo.tolist() == [0, 0, 0]
    for name in ("Affine", "splice_affine", "splice_affine_packed", "transform_feats_packed"):
        assert name in ss.__all__ and hasattr(ss, name)


def test_from_kaldi_takes_the_offset_from_the_last_column(sslib):
    """Kaldi's affine convention: a transform of K + 1 columns on rows of K is [linear | offset]."""
    import speechsauce_amd as ss

    M, bias = matrix(40, 91)
    for t in (ss.Affine.from_kaldi(M), ss.Affine.from_kaldi(M, in_dim=91), ss.Affine.from_kaldi(np.hstack([M, bias[:, None]]), in_dim=91)):
        assert (t.out_dim, t.in_dim) == (40, 91)
    assert ss.Affine.from_kaldi(np.hstack([M, bias[:, None]])).in_dim == 92  # without in_dim a matrix is linear
    with pytest.raises(ValueError):
        ss.Affine.from_kaldi(M, in_dim=89)
    with pytest.raises(ValueError):
        ss.Affine.from_kaldi(M, in_dim=92)
