"""What tests/test_cmvn_conditioning_cpu.py and tests/test_cmvn_conditioning.py share: feature blocks whose columns are hard for a
normalisation kernel (near-constant columns on a large offset, mixed scales), the per-column metric, and numpy restatements of the
column arithmetic of mfcc-rust_amd/csrc/ss_post.hip in the kernels' own order.  No device is touched here.

The restatements keep the kernels' chunking and serial summation order with float64 sums (np.cumsum along an axis is serial) and
round the result to float32; numpy has no fused multiply-add, so they are restatements of the formula, not of the bits.
"""
import functools

import numpy as np

EPS = 2.0 ** -30
KINDS = ("one_ulp_row", "alternating_ulp", "log_floor", "offset_1e5", "plain", "tiny", "big", "const")
LOG_FLOOR = np.float32(np.log(1e-10))  # a silent band of a log-mel block: ln(1e-10) in every row ...
LOG_BUMP = np.float32(-23.0258)        # ... but rows 5 .. 8


@functools.lru_cache(maxsize=None)
def hard_block(rows, cols, seed):
    """float32 [rows, cols], never modified; column c is of kind KINDS[c % 8]:
    one_ulp_row      1000.0, row rows // 3 one ulp up
    alternating_ulp  1000.0, rows ::2 one ulp up
    log_floor        f32(ln 1e-10), rows 5 .. 8 f32(-23.0258)
    offset_1e5       1000 + N(0, 0.01): the offset is 1e5 times the spread
    plain            N(1, 3)
    tiny             N(0, 1e-3)
    big              N(-3e4, 1e4)
    const            1.5"""
    rng = np.random.default_rng(seed)
    up = np.nextafter(np.float32(1000.0), np.float32(2000.0))
    x = np.empty((rows, cols), np.float32)
    for c in range(cols):
        noise = rng.standard_normal(rows)  # drawn for every column: a column's values do not depend on the kinds before it
        kind = KINDS[c % 8]
        if kind == "one_ulp_row":
            x[:, c] = 1000.0
            x[rows // 3, c] = up
        elif kind == "alternating_ulp":
            x[:, c] = 1000.0
            x[::2, c] = up
        elif kind == "log_floor":
            x[:, c] = LOG_FLOOR
            x[5:9, c] = LOG_BUMP
        elif kind == "offset_1e5":
            x[:, c] = (1000.0 + 0.01 * noise).astype(np.float32)
        elif kind == "plain":
            x[:, c] = (1.0 + 3.0 * noise).astype(np.float32)
        elif kind == "tiny":
            x[:, c] = (1e-3 * noise).astype(np.float32)
        elif kind == "big":
            x[:, c] = (-3e4 + 1e4 * noise).astype(np.float32)
        else:
            x[:, c] = 1.5
    x.setflags(write=False)
    return x


def col_rel(got, want):
    """Per column: max abs error over the column's max abs expected -> float64 [cols].  A column whose expected values are all zero
    must be all zero in got (compared with ==): it reports 0 if it is and inf if it is not.  Meant for ONE clip or ONE entry: never a
    block of several clips, where a quiet clip would hide behind a loud one.  Both sides must be finite (see finite_rel)."""
    got = np.asarray(got, np.float64)
    want = np.asarray(want, np.float64)
    assert got.shape == want.shape and got.ndim == 2, (got.shape, want.shape)
    assert np.isfinite(got).all() and np.isfinite(want).all()
    top = np.abs(want).max(axis=0)
    zero = top == 0
    err = np.abs(got - want).max(axis=0)
    return np.where(zero, np.where(err == 0, 0.0, np.inf), err / np.where(zero, 1.0, top))


def finite_rel(got, want):
    """-> (col_rel over the elements that are finite on both sides, the others counting as 0 on both; the number of elements that are
    finite on one side only).  The caller asserts that the second is 0."""
    got, want = np.asarray(got), np.asarray(want)
    fg, fw = np.isfinite(got), np.isfinite(want)
    both = fg & fw
    return col_rel(np.where(both, got, 0.0), np.where(both, want, 0.0)), int((fg != fw).sum())


# ---------------------------------------------------------------- cmvn: ss_cmvn_partial / _apply and ss_cmvn_packed_kernel ------

def _chunk_sums(x64, about):
    """s1 = sum x and s2 = sum (x - about)^2 per column in the kernels' order: min(64, ceil(T / 32)) chunks of ceil(T / chunks) rows,
    each summed serially, the chunk sums added serially in chunk order (vad_model.cmvn_sum is the same walk for s1)."""
    T = x64.shape[0]
    chunks = min(64, -(-T // 32))
    rpc = -(-T // chunks)
    s1 = np.zeros(x64.shape[1])
    s2 = np.zeros(x64.shape[1])
    for k in range(chunks):
        blk = x64[k * rpc:min(T, (k + 1) * rpc)]
        if len(blk):
            d = blk - about
            s1 = s1 + np.cumsum(blk, axis=0)[-1]
            s2 = s2 + np.cumsum(d * d, axis=0)[-1]
    return s1, s2


def _finish(x64, mean, var, variance):
    inv = 1.0 / (np.sqrt(np.maximum(var, 0.0)) + EPS) if variance else 1.0
    return ((x64 - mean) * inv).astype(np.float32)


def cmvn_one_pass(x, variance):
    """The form of the parent commit: var = sum(x^2) / n - mean^2.  x [T, cols] float32, one clip -> float32."""
    x64 = np.asarray(x, np.float64)
    T = x64.shape[0]
    s1, s2 = _chunk_sums(x64, 0.0)
    mean = s1 / T
    return _finish(x64, mean, s2 / T - mean * mean, variance)


def cmvn_shifted(x, variance):
    """The form the kernels ship: the squares about K, the clip's first row of the column; var = sum((x - K)^2) / n - (mean - K)^2.
    s1, and with it the mean, is formed exactly as in cmvn_one_pass."""
    x64 = np.asarray(x, np.float64)
    T = x64.shape[0]
    K = x64[0]
    s1, s2 = _chunk_sums(x64, K)
    mean = s1 / T
    d = mean - K
    return _finish(x64, mean, s2 / T - d * d, variance)


# ---------------------------------------------------------------- the stream pool: stream_window_sums / stream_normalise --------

def _stream(x, win, variance, shifted):
    x64 = np.asarray(x, np.float64)
    out = np.empty(x64.shape, np.float32)
    for t in range(x64.shape[0]):
        n = min(t + 1, win)
        W = x64[t - n + 1:t + 1]                      # oldest row first, the row itself the newest
        K = x64[t] if shifted else 0.0
        s1 = np.cumsum(W, axis=0)[-1]
        s2 = np.cumsum((W - K) ** 2, axis=0)[-1]
        mean = s1 / n
        d = mean - K
        out[t] = _finish(x64[t], mean, s2 / n - d * d, variance)
    return out


def stream_one_pass(x, win, variance):
    """The pool kernel's arithmetic in the parent commit on the rows of ONE stream since its reset: x [T, cols] -> float32."""
    return _stream(x, win, variance, False)


def stream_shifted(x, win, variance):
    """The pool kernel's arithmetic as shipped: the squares about the row being normalised."""
    return _stream(x, win, variance, True)


# ---------------------------------------------------------------- the cases both test files run on ------------------------------

CMVN_ROWS = (98, 301, 1598)              # one second, 3 s, 16 s of 10 ms frames: 4, 10 and 50 chunks
CMVN_COLS = (13, 40)                     # a partial first tile; the eight kinds again in the second 32-column tile
PACKED_ROWS = (98, 0, 1, 2, 301, 1598, 2100, 5)  # 2100 > kCmvnSplitRows: workgroups share the clip
CMVNW_ROWS = (98, 5, 301, 400)
CMVNW_WINS = (3, 31, 301)
STREAM_COLS = 40
STREAM_WINS = (2, 31, 301)
# the oracle's own |output| in every cmvnw variance case below stays under this (asserted on the CPU): the kernels round the
# mean-subtracted values to f32 between cmvnw's two passes, so an output of magnitude A carries a relative error of about A * 6e-8,
# and 160 keeps that at a tenth of RTOL (the reasoning of tests/test_packed_post.py)
CMVNW_ORACLE_BOUND = 160.0


def cmvn_block(rows, cols):
    return hard_block(rows, cols, 1000 + rows + cols)


def clips(rows_list, cols, seed0):
    """One hard_block per clip (None for an empty one), each with its own seed."""
    return [hard_block(r, cols, seed0 + b) if r else None for b, r in enumerate(rows_list)]


def pack(clip_list, cols):
    """-> (block [sum rows, cols] float32, offsets int64)"""
    off = np.zeros(len(clip_list) + 1, np.int64)
    np.cumsum([0 if c is None else c.shape[0] for c in clip_list], out=off[1:])
    block = np.concatenate([c for c in clip_list if c is not None] or [np.zeros((0, cols), np.float32)])
    return np.ascontiguousarray(block, np.float32), off


def stream_rows(ticks):
    """rows of stream b over the whole schedule ticks[k][b]"""
    return [sum(t[b] for t in ticks) for b in range(len(ticks[0]))]


def streams(ticks, cols=STREAM_COLS, seed0=3000):
    """One hard_block per stream, as long as the schedule feeds it."""
    return [hard_block(T, cols, seed0 + b) for b, T in enumerate(stream_rows(ticks))]


def poison(x, row, value, cols=(3, 35)):
    """A writable copy of x with `value` at `row` of the given columns (those that exist)."""
    y = np.array(x, np.float32)
    for c in cols:
        if c < y.shape[1]:
            y[row, c] = value
    return y


BAD_VALUES = (np.float32("nan"), np.float32("-inf"), np.float32("inf"))
