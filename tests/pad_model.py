"""What tests/test_pad_cpu.py and tests/test_pad.py share: the numpy restatement of the ss_pad_* section of include/speechsauce_amd.h.
Everything is compared on bit patterns: float32 is a bit copy, float16 is numpy's astype, bfloat16 the header's integer formula; a
NaN input must give a NaN output whose payload is not specified, so the 16-bit comparisons are off-NaN plus the NaN positions."""
import numpy as np

from splice_model import clip, u32  # noqa: F401  (clip: the tests' salted input rows)

LAYOUTS = ("btc", "bct")
DTYPES = ("float32", "float16", "bfloat16")
LAYOUT_CODE = {"btc": 0, "bct": 1}   # SS_PAD_BTC / SS_PAD_BCT
DTYPE_CODE = {"float32": 0, "float16": 1, "bfloat16": 2}  # SS_PAD_F32 / SS_PAD_F16 / SS_PAD_BF16
BITS_DTYPE = {"float32": np.uint32, "float16": np.uint16, "bfloat16": np.uint16}
PAD_ROUNDS = np.float32(1.00390625)  # 0x3F808000: a tie in bfloat16 (to even: 0x3F80)


def to_f16_bits(x):
    with np.errstate(over="ignore", invalid="ignore"):
        return np.ascontiguousarray(np.asarray(x, np.float32).astype(np.float16)).view(np.uint16)


def to_bf16_bits(x):
    """(bits + 0x7FFF + ((bits >> 16) & 1)) >> 16 on the float32 bit pattern, in 64 bits so that nothing wraps; what it makes of a
    NaN is not looked at"""
    b = u32(np.asarray(x, np.float32)).astype(np.uint64)
    return (((b + 0x7FFF + ((b >> 16) & 1)) >> 16) & 0xFFFF).astype(np.uint16)


def conv_bits(x, dtype):
    if dtype == "float32":
        return u32(np.asarray(x, np.float32)).copy()
    return to_f16_bits(x) if dtype == "float16" else to_bf16_bits(x)


def is_nan_bits(bits, dtype):
    if dtype == "float32":
        return (bits & 0x7FFFFFFF) > 0x7F800000
    if dtype == "float16":
        return (bits & 0x7FFF) > 0x7C00
    return (bits & 0x7FFF) > 0x7F80


def pad_ref(x, ro, total_rows, max_rows, layout, dtype, pad_value):
    """The definition -> (bits [n, max_rows, cols] or [n, cols, max_rows], nan [same shape, bool], lengths int32 [n]).  A segment that
    is reversed, starts below 0 or ends past total_rows is all pad with length -1."""
    x = np.asarray(x, np.float32)
    cols, n = x.shape[1], len(ro) - 1
    vals = np.full((n, max_rows, cols), np.float32(pad_value), np.float32)
    lengths = np.zeros(n, np.int32)
    for b in range(n):
        lo, hi = int(ro[b]), int(ro[b + 1])
        if not 0 <= lo <= hi <= total_rows:
            lengths[b] = -1
            continue
        kept = min(hi - lo, max_rows)
        u32(vals)[b, :kept] = u32(x[lo:lo + kept])  # on bit patterns: an assignment of floats may quiet a signalling NaN
        lengths[b] = kept
    if layout == "bct":
        vals = np.ascontiguousarray(np.transpose(vals, (0, 2, 1)))
    return conv_bits(vals, dtype), np.isnan(vals), lengths


def same(got_bits, want_bits, want_nan, dtype):
    """the header's comparison: float32 bit for bit everywhere; the 16-bit types bit for bit off-NaN and NaN exactly where a NaN went in"""
    got_bits = np.asarray(got_bits)
    if got_bits.shape != want_bits.shape:
        return False
    if dtype == "float32":
        return bool(np.array_equal(got_bits, want_bits))
    return bool(np.array_equal(is_nan_bits(got_bits, dtype), want_nan) and np.array_equal(got_bits[~want_nan], want_bits[~want_nan]))
