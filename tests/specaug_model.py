"""What tests/test_specaug_cpu.py and tests/test_specaug.py share: the numpy restatement of the ss_specaug_* section of
include/speechsauce_amd.h -- Philox4x32-10 in uint64 arithmetic, the draw of one span, the spans table of a packed block and the
masking itself on uint32 bit patterns.  Nothing here is float arithmetic except the one f64 product of the time bound.
"""
import numpy as np

from splice_model import SENTINEL, clip, u32  # noqa: F401  (re-exported for the tests)

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK32 = 0xFFFFFFFF
FREQ_BASE = 0x10000  # mask index of frequency mask 0
MAX_MASKS = 16
# (counter, key) -> output: the known answers of the header
KNOWN = (((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
         ((MASK32,) * 4, (MASK32,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
         ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)))
# the worked pin: seed 2026, epoch 0, clip_base 0, T_b = 200, max_time_width = 40, ratio 1, n_time = 2; clips 0, 1, 2
PIN = (((96, 17), (1, 29)), ((56, 40), (105, 31)), ((124, 28), (130, 13)))


def philox(ctr, key):
    """Philox4x32-10 on arrays: ctr = four uint32 arrays (or ints) of one shape, key = two -> four uint32 arrays."""
    c = [np.asarray(v, np.uint64) & np.uint64(MASK32) for v in ctr]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = (int(v) & MASK32 for v in key)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]  # 32 x 32 -> 64 bits: no overflow in uint64
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & np.uint64(MASK32), (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & np.uint64(MASK32)]
        k0, k1 = (k0 + W0) & MASK32, (k1 + W1) & MASK32
    return [v.astype(np.uint32) for v in c]


def time_bound(T, max_width, ratio):
    """W_b: one f64 product of the float32 ratio and the row count, truncated"""
    return np.minimum(np.uint64(max_width), np.floor(np.float64(np.float32(ratio)) * np.asarray(T, np.float64)).astype(np.uint64))


def draw(seed, epoch, clip_id, k, bound, extent):
    """(start, width) of mask index k of the clips `clip_id` (arrays): width in [0, bound], start in [0, extent - width]"""
    seed, epoch = int(seed) & (2 ** 64 - 1), int(epoch) & (2 ** 64 - 1)
    clip_id = np.asarray(clip_id, np.uint64) & np.uint64(MASK32)
    u0, u1, _, _ = philox((clip_id, np.full(clip_id.shape, k, np.uint64), epoch & MASK32, epoch >> 32), (seed & MASK32, seed >> 32))
    bound, extent = np.asarray(bound, np.uint64), np.asarray(extent, np.uint64)
    width = (u0.astype(np.uint64) * (bound + np.uint64(1))) >> np.uint64(32)
    start = (u1.astype(np.uint64) * (extent - width + np.uint64(1))) >> np.uint64(32)
    return start.astype(np.int64), width.astype(np.int64)


def spans_ref(rng, clip_base, ro, total_rows, cols, n_time, max_time_width, time_ratio, n_freq, max_freq_width):
    """The spans table int32 [n_clips, n_time + n_freq, 2] of (start, width) pairs, time masks first; a segment that is reversed,
    starts below 0 or ends past total_rows has (-1, 0) in every span."""
    ro = np.asarray(ro, np.int64)
    n = len(ro) - 1
    lo, hi = ro[:-1], ro[1:]
    good = (lo >= 0) & (lo <= hi) & (hi <= total_rows)
    T = np.where(good, hi - lo, 0)
    ids = int(clip_base) + np.arange(n, dtype=np.int64)
    out = np.zeros((n, n_time + n_freq, 2), np.int32)
    W = time_bound(T, max_time_width, time_ratio)
    F = min(int(max_freq_width), int(cols))
    for k in range(n_time):
        out[:, k, 0], out[:, k, 1] = draw(rng[0], rng[1], ids, k, W, T)
    for j in range(n_freq):
        out[:, n_time + j, 0], out[:, n_time + j, 1] = draw(rng[0], rng[1], ids, FREQ_BASE + j, np.full(n, F, np.uint64), np.full(n, cols, np.uint64))
    out[~good] = (-1, 0)
    return out


def apply_ref(bits, ro, total_rows, spans, n_time, n_freq, mask_bits, out=None):
    """out (default: a copy of bits) with mask_bits where a row lies in a time span of its clip or a column in a frequency span; a span
    that is out of range (start < 0, width < 0, start + width > its extent) is skipped whole, and so are the rows of a bad segment
    and the rows in no clip.  bits and out are uint32 [total_rows, cols]."""
    bits = np.asarray(bits, np.uint32)
    out = bits.copy() if out is None else out
    cols = bits.shape[1]
    ro = np.asarray(ro, np.int64)
    for b in range(len(ro) - 1):
        lo, hi = int(ro[b]), int(ro[b + 1])
        if not 0 <= lo <= hi <= total_rows:
            continue
        T = hi - lo
        blk = bits[lo:hi].copy()
        for k in range(n_time + n_freq):
            start, width = int(spans[b, k, 0]), int(spans[b, k, 1])
            extent = T if k < n_time else cols
            if start < 0 or width < 0 or start + width > extent:
                continue
            if k < n_time:
                blk[start:start + width] = mask_bits
            else:
                blk[:, start:start + width] = mask_bits
        out[lo:hi] = blk
    return out


def chi2(counts, expected):
    return float(((counts - expected) ** 2 / expected).sum())
