"""Padded-batch collation (ss_pad_*), the part that needs no device: the numpy restatement of the header's definition
(tests/pad_model.py) on hand-written bit patterns and against torch's CPU conversions, the symbols in every mirror, the host-only size
call, every argument error of both forms, and the Python front's argument rules."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from pad_model import DTYPES, PAD_ROUNDS, clip, conv_bits, is_nan_bits, pad_ref, same, to_bf16_bits, to_f16_bits, u32

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"ss_pad_packed_out_bytes": 5, "ss_pad_packed_device": 12, "ss_pad_packed": 11}
ERR_ARG = 3


def _f32(*bits):
    return np.array(bits, np.uint32).view(np.float32)


def test_the_conversions_on_hand_written_bit_patterns():
    # bfloat16: ties go to even, f32 denormals are not flushed, the largest finite float rounds to inf, +-inf and -0.0 stay
    cases = {0x3F808000: 0x3F80, 0x3F818000: 0x3F82, 0x3F808001: 0x3F81, 0x3F807FFF: 0x3F80, 0x3F800000: 0x3F80, 0xBF818000: 0xBF82,
             0x00000001: 0x0000, 0x00008000: 0x0000, 0x00008001: 0x0001, 0x00018000: 0x0002, 0x007FFFFF: 0x0080, 0x80018000: 0x8002,
             0x7F7FFFFF: 0x7F80, 0x7F800000: 0x7F80, 0xFF800000: 0xFF80, 0x80000000: 0x8000, 0x00000000: 0x0000}
    assert to_bf16_bits(_f32(*cases)).tolist() == list(cases.values())
    # float16: 65504 is the largest finite value and 65520 the first to round to inf; the denormal range 2^-24 .. 2^-14 is produced
    cases = {0x477FE000: 0x7BFF, 0x477FEFFF: 0x7BFF, 0x477FF000: 0x7C00, 0xC77FF000: 0xFC00, 0x7F800000: 0x7C00, 0xFF800000: 0xFC00,
             0x3F800000: 0x3C00, 0x3F801000: 0x3C00, 0x3F803000: 0x3C02, 0x3F801001: 0x3C01,            # ties to even at 1.0
             0x33800000: 0x0001, 0x33000000: 0x0000, 0x33000001: 0x0001, 0x33C00000: 0x0002,            # 2^-24, 2^-25 (tie), just above, 1.5 * 2^-24 (tie)
             0x387FC000: 0x03FF, 0x38800000: 0x0400, 0x387FE000: 0x0400, 0xB3800000: 0x8001,            # the largest denormal, 2^-14, the tie between
             0x00000001: 0x0000, 0x80000001: 0x8000, 0x007FFFFF: 0x0000, 0x80000000: 0x8000, 0x00000000: 0x0000}
    assert to_f16_bits(_f32(*cases)).tolist() == list(cases.values())
    nan = _f32(0x7FC00001, 0xFFC12345, 0x7F800001, 0x7FFFFFFF, 0xFF80FFFF)
    assert is_nan_bits(to_f16_bits(nan), "float16").all() and is_nan_bits(u32(nan), "float32").all()
    assert np.array_equal(conv_bits(nan, "float32"), u32(nan))  # float32 keeps every payload
    assert not is_nan_bits(np.array([0x7F80, 0xFF80, 0x7F7F], np.uint16), "bfloat16").any() and is_nan_bits(np.array([0x7F81, 0xFFC0], np.uint16), "bfloat16").all()


def test_the_conversions_are_torchs_on_the_cpu():
    """Off-NaN both formulas are torch.Tensor.to(float16 / bfloat16) bit for bit over 2 x 10^6 random bit patterns; a NaN stays one."""
    torch = pytest.importorskip("torch")
    bits = np.random.default_rng(7).integers(0, 1 << 32, 2_000_000, dtype=np.uint64).astype(np.uint32)
    bits[:8] = [0x3F808000, 0x3F818000, 0x477FE000, 0x477FF000, 0x33000000, 0x00000001, 0x80000000, 0x7F7FFFFF]
    x = bits.view(np.float32)
    nan = np.isnan(x)
    assert nan.sum() > 1000
    t = torch.from_numpy(x.copy())
    for dtype, tdt in (("float16", torch.float16), ("bfloat16", torch.bfloat16)):
        got = t.to(tdt).view(torch.int16).numpy().view(np.uint16)
        assert np.array_equal(is_nan_bits(got, dtype), nan), dtype
        assert np.array_equal(got[~nan], conv_bits(x, dtype)[~nan]), dtype


def test_the_restatement_itself():
    cols, lens = 5, [0, 3, 7, 2]
    ro = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    x = clip(cols, int(ro[-1]), seed=1)
    assert np.isnan(x).any()
    for dtype in DTYPES:
        for max_rows in (1, 3, 4, 9):
            btc, nan, lengths = pad_ref(x, ro, len(x), max_rows, "btc", dtype, -1.5)
            bct, nan_t, lengths_t = pad_ref(x, ro, len(x), max_rows, "bct", dtype, -1.5)
            assert btc.shape == (4, max_rows, cols) and bct.shape == (4, cols, max_rows) and btc.dtype == bct.dtype
            assert np.array_equal(bct, np.transpose(btc, (0, 2, 1))) and np.array_equal(nan_t, np.transpose(nan, (0, 2, 1)))  # bct is btc transposed
            assert lengths.tolist() == lengths_t.tolist() == [min(n, max_rows) for n in lens] and lengths.dtype == np.int32
            pad = conv_bits(np.float32(-1.5), dtype)
            for b, n in enumerate(lens):
                kept = min(n, max_rows)  # truncation: the clip's FIRST max_rows rows
                assert np.array_equal(btc[b, :kept], conv_bits(x[ro[b]:ro[b] + kept], dtype)) and (btc[b, kept:] == pad).all(), (dtype, max_rows, b)
            # the comparison itself: any NaN pattern passes where a NaN went in (float32: only the input's own), nothing else does
            got = btc.copy()
            if dtype != "float32":
                got[nan] = {"float16": 0x7E01, "bfloat16": 0xFFC1}[dtype]
            assert nan.any() == (max_rows > 1) and same(got, btc, nan, dtype) and not same(got[:, :, ::-1], btc, nan, dtype)
            flip = got.copy()
            flip[1, 0, 0] ^= 1
            assert not same(flip, btc, nan, dtype)
            if nan.any():
                lost = got.copy()
                lost[nan] = 0
                assert not same(lost, btc, nan, dtype)
    # bad segments: all pad, length -1; an empty clip: all pad, length 0
    #                 good | reversed | empty | good | past the end | reversed | reversed, ends below 0 | starts below 0 | good
    bad = np.array([0, 4, 2, 2, 6, 13, 12, -1, 3, 6], np.int64)
    bits, _, lengths = pad_ref(x, bad, 12, 4, "btc", "bfloat16", PAD_ROUNDS)
    assert lengths.tolist() == [4, -1, 0, 4, -1, -1, -1, -1, 3]
    assert to_bf16_bits(PAD_ROUNDS) == 0x3F80 and u32(PAD_ROUNDS) == 0x3F808000  # a pad value that rounds
    for b in (1, 2, 4, 5, 6, 7):
        assert (bits[b] == 0x3F80).all()
    assert np.array_equal(bits[8, :3], to_bf16_bits(x[3:6])) and (bits[8, 3] == 0x3F80).all()
    assert pad_ref(x, ro[:1], len(x), 3, "bct", "float16", 0.0)[0].shape == (0, cols, 3)


def test_symbols_are_declared_exported_and_prototyped(sslib):
    from speechsauce_amd import _lib

    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "speechsauce_amd.h")).read(), flags=re.S)
    shim = open(os.path.join(ROOT, "mfcc-rust_amd", "rust-shim", "src", "lib.rs")).read()
    externs = re.search(r'extern "C" \{(.*?)\n\}', shim, flags=re.S).group(1)
    hpp = open(os.path.join(ROOT, "include", "speechsauce_amd.hpp")).read()
    for name, arity in NAMES.items():
        decl = re.search(r"^int %s\(([^;]*?)\);" % name, header, flags=re.M | re.S)
        assert decl and len(decl.group(1).split(",")) == arity, name
        ext = re.search(r"fn %s\((.*?)\)\s*->\s*c_int;" % name, externs, flags=re.S)
        assert ext and len(ext.group(1).split(",")) == arity, name
        assert name in _lib.PROTOTYPES, name
        fn = getattr(sslib, name)  # exported by the library (ss_exports.map lets every ss_* symbol out)
        assert fn.restype is C.c_int and len(fn.argtypes) == len(_lib.PROTOTYPES[name][1]) == arity, name
        assert name.endswith("_device") or name + "(" in hpp, name  # the C++ mirror wraps the host forms, as for splice
    assert sorted(n for n in _lib.PROTOTYPES if n.startswith("ss_pad_")) == sorted(NAMES)
    assert "ss_*;" in open(os.path.join(ROOT, "mfcc-rust_amd", "csrc", "ss_exports.map")).read()
    assert re.search(r"enum \{ SS_PAD_F32 = 0, SS_PAD_F16 = 1, SS_PAD_BF16 = 2 \};", header) and re.search(r"enum \{ SS_PAD_BTC = 0, SS_PAD_BCT = 1 \};", header)
    assert "inline std::vector<uint8_t> pad_packed(" in hpp and "pub fn try_pad_packed(" in shim and "pub unsafe fn pad_packed_device(" in shim
    assert sslib.ss_abi_version() == 7 and _lib.ABI_VERSION == 7  # entry points only: the version stays


def _out_bytes(sslib, n, max_rows, cols, dtype):
    b = C.c_size_t(12345)
    return sslib.ss_pad_packed_out_bytes(n, max_rows, cols, dtype, C.byref(b)), b.value


def test_out_bytes_formula_and_rejections(sslib):
    for n, max_rows, cols in ((0, 5, 80), (1, 1, 1), (7, 131, 13), (1024, 1600, 240), ((1 << 31) - 1, 3, 5), (1 << 20, 1 << 20, 1 << 20)):
        for dtype, size in ((0, 4), (1, 2), (2, 2)):
            assert _out_bytes(sslib, n, max_rows, cols, dtype) == (0, n * max_rows * cols * size), (n, max_rows, cols, dtype)
    assert _out_bytes(sslib, 1 << 21, 1 << 21, 1 << 20, 1) == (0, 1 << 63)             # the largest power of two that fits
    for bad in ((1 << 21, 1 << 21, 1 << 21, 1), (1 << 21, 1 << 21, 1 << 20, 0), (1 << 40, 1 << 40, 1, 0), (3, 1 << 63, 2, 2), (1, 1, 1 << 63, 0)):
        assert _out_bytes(sslib, *bad) == (ERR_ARG, 12345), bad                     # overflow: SS_ERR_ARG, the output untouched
    assert b"overflow" in sslib.ss_last_error_string()
    for dtype in (-1, 3, 99):
        assert _out_bytes(sslib, 2, 3, 4, dtype) == (ERR_ARG, 12345), dtype
    assert sslib.ss_pad_packed_out_bytes(2, 3, 4, 0, None) == ERR_ARG


def test_argument_errors_are_decided_before_the_device_is_touched(sslib):
    """Every call here is rejected (or has nothing to do) on the host: none of the pointers is ever handed to the device, so host
    arrays stand in for device buffers.  On a host without a device a call that got past its checks would return SS_ERR_HIP (4)."""
    cols, rows, max_rows = 13, 12, 5
    vec = np.ones((rows, cols), np.float32)
    out = np.full((2, max_rows, cols), -5.0, np.float32)
    lengths = np.full(2, -7, np.int32)
    off = np.array([0, 3, 12], np.int64)
    v, o, ln, r = vec.ctypes.data, out.ctypes.data, lengths.ctypes.data, off.ctypes.data

    def dev(vec=v, n=2, ro=r, total=rows, cols=cols, max_rows=max_rows, layout=0, dtype=0, pad=0.0, out=o, lengths=ln):
        return sslib.ss_pad_packed_device(vec, n, ro, total, cols, max_rows, layout, dtype, pad, out, lengths, None)

    def host(vec=v, n=2, ro=r, total=rows, cols=cols, max_rows=max_rows, layout=0, dtype=0, pad=0.0, out=o, lengths=ln):
        return sslib.ss_pad_packed(vec, n, ro, total, cols, max_rows, layout, dtype, pad, out, lengths)

    for call in (dev, host):
        what = call.__name__
        assert call(n=0) == 0, what  # an empty call is SS_OK and writes nothing, also without a device and whatever else is passed
        for name in ("vec", "ro", "out", "lengths"):
            assert call(**{name: None}) == ERR_ARG, (what, name)
        assert call(cols=0) == ERR_ARG and call(max_rows=0) == ERR_ARG, what
        assert b"max_rows" in sslib.ss_last_error_string()
        for layout in (-1, 2, 7):
            assert call(layout=layout) == ERR_ARG, (what, layout)
        assert b"layout" in sslib.ss_last_error_string()
        for dtype in (-1, 3, 7):
            assert call(dtype=dtype) == ERR_ARG, (what, dtype)
        assert b"dtype" in sslib.ss_last_error_string()
        for name in ("n", "total", "cols", "max_rows"):
            assert call(**{name: 1 << 31}) == ERR_ARG and call(**{name: 1 << 40}) == ERR_ARG, (what, name)
        assert call(n=(1 << 31) - 1, cols=(1 << 31) - 1, max_rows=(1 << 31) - 1) == ERR_ARG and b"overflow" in sslib.ss_last_error_string(), what
        assert call(out=o + 1) == ERR_ARG and call(out=o + 2) == ERR_ARG and call(out=o + 3) == ERR_ARG, what  # float32: 4-byte aligned
        assert b"aligned" in sslib.ss_last_error_string()
        for dtype in (1, 2):
            assert call(dtype=dtype, out=o + 1) == ERR_ARG and call(dtype=dtype, out=o + 3) == ERR_ARG, (what, dtype)  # halves: 2-byte aligned
        for pad in (float("nan"), float("inf"), -0.0):  # any pad value is legal: the rejection is the other argument's
            assert call(pad=pad, cols=0) == ERR_ARG, what
    assert sslib.ss_pad_packed_device(None, 0, None, 0, 0, 0, 9, 9, 0.0, None, None, None) == 0
    assert sslib.ss_pad_packed(None, 0, None, 0, 0, 0, 9, 9, 0.0, None, None) == 0
    # the device form: out and lengths must not overlap vec
    assert dev(out=v) == ERR_ARG and b"in place" in sslib.ss_last_error_string()
    assert dev(out=v + 4 * (rows * cols - 1)) == ERR_ARG                      # ... not even in its last float
    assert dev(out=v - 4 * (2 * max_rows * cols - 1)) == ERR_ARG              # out has 2 * max_rows * cols floats
    assert dev(dtype=2, out=v - 2 * (2 * max_rows * cols - 1)) == ERR_ARG     # ... or as many halves
    assert dev(lengths=v) == ERR_ARG and b"lengths" in sslib.ss_last_error_string()
    assert dev(lengths=v + 4 * (rows * cols - 1)) == ERR_ARG and dev(lengths=v - 4) == ERR_ARG
    # the host form's table errors name the first bad clip
    for bad, where in (([1, 2, 12], b"clip 0"), ([0, 4, 3], b"clip 1"), ([0, 2, 13], b"clip 1")):
        b = np.array(bad, np.int64)
        assert host(ro=b.ctypes.data) == ERR_ARG and where in sslib.ss_last_error_string(), bad
    assert (out == -5.0).all() and (lengths == -7).all() and (vec == 1.0).all()  # nothing was written by any of it


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
    for call in (lambda: ss.pad_packed(x, [0, 2, 6]), lambda: ss.pad_packed(x, [0, 2, 6], 4, "bct", "bfloat16"), lambda: ss.pad([x[:2], x[2:]])):
        with pytest.raises(SpeechSauceError) as e:
            call()
        assert e.value.status == 4  # SS_ERR_HIP: there is no CPU path


class _DeviceTable:
    """stands in for a row_offsets tensor that lives on the device: the front must refuse before it looks at anything else"""
    is_cuda = True


_DeviceTable.__module__ = "torch"


def test_python_argument_rules(sslib):
    import speechsauce_amd as ss

    for name in ("pad", "pad_packed"):
        assert name in ss.__all__ and hasattr(ss, name)
    z = lambda r, c=13, dt=np.float32: np.zeros((r, c), dt)  # noqa: E731
    with pytest.raises(ValueError, match="max_rows"):
        ss.pad_packed(z(4), _DeviceTable())  # max_rows=None and a device table: no hidden synchronisation
    with pytest.raises(ValueError, match="max_rows"):
        ss.pad_packed(z(4), _DeviceTable(), max_rows=None, layout="bct", dtype="bfloat16")
    for bad in (dict(layout="tbc"), dict(layout=0), dict(dtype="float64"), dict(dtype="int8"), dict(dtype=np.float64), dict(dtype=None),
                dict(max_rows=0), dict(max_rows=-3)):
        with pytest.raises(ValueError):
            ss.pad_packed(z(4), [0, 4], **bad)
        with pytest.raises(ValueError):
            ss.pad([z(4)], **bad)
    with pytest.raises(TypeError):
        ss.pad_packed(z(4, dt=np.float64), [0, 4])
    with pytest.raises(ValueError):
        ss.pad_packed(np.zeros(13, np.float32), [0, 1])  # a flat block
    with pytest.raises(ValueError):
        ss.pad_packed(np.zeros((4, 0), np.float32), [0, 4])  # no columns
    for bad_off in ([1, 4], [0, 3, 2], [0, 5]):
        with pytest.raises(ValueError):
            ss.pad_packed(z(4), bad_off, 3)
    with pytest.raises(TypeError):
        ss.pad_packed(z(4), np.array([0.0, 4.0]), 3)
    with pytest.raises(ValueError):
        ss.pad([])
    with pytest.raises(ValueError):
        ss.pad([z(4), z(2, 12)])  # other cols
    with pytest.raises(ValueError):
        ss.pad([z(4), np.zeros(13, np.float32)])
    # nothing for the device to do: no clips, or no clip has a row and max_rows is taken from the table
    for dtype, np_dt in (("float32", np.float32), ("float16", np.float16), (np.float16, np.float16), ("bfloat16", np.uint16)):
        out, lengths = ss.pad_packed(z(0), [0], 5, "btc", dtype)
        assert out.shape == (0, 5, 13) and out.dtype == np_dt and lengths.shape == (0,) and lengths.dtype == np.int32
        out, lengths = ss.pad_packed(z(0), [0, 0, 0], None, "bct", dtype)
        assert out.shape == (2, 13, 0) and out.dtype == np_dt and lengths.tolist() == [0, 0]
    torch = pytest.importorskip("torch")
    with pytest.raises(ValueError):
        ss.pad_packed(z(4), [0, 4], dtype=torch.float64)
    out, _ = ss.pad_packed(z(0), [0], 5, "btc", torch.bfloat16)  # the torch dtypes name the same three types
    assert out.dtype == np.uint16 and ss.pad_packed(z(0), [0], 5, dtype=torch.float16)[0].dtype == np.float16
    with pytest.raises(TypeError):
        ss.pad([z(4), torch.zeros(2, 13)])  # numpy and tensors mixed
