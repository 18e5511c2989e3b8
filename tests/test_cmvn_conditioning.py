"""The CMVN family (ss_cmvn*, ss_cmvnw*, their packed forms and the stream pool) against the two-pass references, per column and per
clip, on columns that are hard for a normalisation kernel: near-constant columns on a large offset, a log-mel band at its floor,
columns of very different scale in one matrix, and columns that hold one NaN or infinity (cmvn_model.hard_block).

Every comparison is cmvn_model.col_rel <= common.RTOL: the error of a column over THAT column's largest expected value, within one
clip or one entry.  tests/test_cmvn_conditioning_cpu.py shows on the same blocks that the references themselves use less than 1e-7
of that, and that a one-pass variance sum(x^2) / n - mean^2 misses it by orders of magnitude on the near-constant columns.  Where
the reference is not finite the kernels must not be finite either, element for element, and the other way round.

Every test prints its worst figure per case before it asserts.
"""
import numpy as np
import pytest

import cmvn_model as M
from common import RTOL
from test_cmvn_stream_packed import POOL, SLOTS, TICKS, _feed, restate

pytestmark = pytest.mark.gpu
ORDER = [[4, 0, 6, 2, 5, 1, 3], [6, 5, 4, 3, 2, 1, 0], [1, 3, 5, 0, 2, 4, 6]]  # where the entries stand in each tick


class Report:
    """Collects (case, worst column error, elements finite on one side only), prints them all, then asserts."""

    def __init__(self, what):
        self.what, self.lines, self.bounds = what, [], []

    def add(self, case, got, want):
        got = np.asarray(got)
        assert got.dtype == np.float32 and got.shape == want.shape, (case, got.dtype, got.shape)
        err, odd = M.finite_rel(got, want)
        self.lines.append((case, float(err.max()), int(err.argmax()), odd))

    def bound(self, case, got, n_t):
        """|out| <= sqrt(n_t) * (1 + 1e-6) wherever out is finite: a row is a member of its own window"""
        ok = np.isfinite(got)
        self.bounds.append((case, float((np.abs(np.where(ok, got, 0.0)) / np.sqrt(n_t)[:, None]).max())))

    def done(self):
        worst = max(self.lines, key=lambda l: (l[3], l[1]))
        bad = [l for l in self.lines if l[3] or not l[1] <= RTOL]
        over = [b for b in self.bounds if not b[1] <= 1.0 + 1e-6]
        if self.bounds:
            print(f"{self.what}: largest |out| / sqrt(n_t) {max(b[1] for b in self.bounds):.9g}")
        for case, ratio in over:
            print(f"  MISS {case}: |out| is {ratio:.4g} times sqrt(n_t)")
        print(f"{self.what}: {len(self.lines)} comparisons, worst {worst[0]}: {worst[1]:.3g} in column {worst[2]}"
              + (f", {worst[3]} elements finite on one side only" if worst[3] else ""))
        for case, e, c, odd in bad:
            print(f"  MISS {case}: {e:.3g} in column {c} ({M.KINDS[c % 8]}), finite on one side only: {odd}")
        assert not bad and not over, (self.what, over[:6], bad[:6])


def _oracle(fn, x, *args):
    with np.errstate(all="ignore"):
        return fn(x, *args)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---------------------------------------------------------------- cmvn -----------------------------------------------------------

@pytest.mark.parametrize("cols", M.CMVN_COLS)
@pytest.mark.parametrize("rows", M.CMVN_ROWS)
def test_cmvn_one_matrix_and_batch_block(ss, oracle, rows, cols):
    import torch

    blocks = [M.cmvn_block(rows, cols), M.hard_block(rows, cols, 1100 + rows), M.hard_block(rows, cols, 1200 + cols)]
    dev = torch.from_numpy(np.stack(blocks)).cuda()
    rep = Report(f"cmvn rows {rows} cols {cols}")
    for var in (False, True):
        batch = ss.cmvn(dev, var).cpu().numpy()  # [3, rows, cols]: ss_cmvn_batch_device on three clips
        for b, x in enumerate(blocks):
            want = oracle.cmvn(x, var)
            rep.add(f"batch clip {b} var {var}", batch[b], want)
        rep.add(f"one matrix var {var}", ss.cmvn(blocks[0], var), oracle.cmvn(blocks[0], var))
    rep.done()


@pytest.mark.parametrize("cols", M.CMVN_COLS)
def test_cmvn_packed(ss, oracle, cols):
    import torch

    clip_list = M.clips(M.PACKED_ROWS, cols, 2000)
    block, off = M.pack(clip_list, cols)
    d, doff = torch.from_numpy(block).cuda(), torch.from_numpy(off).cuda()
    rep = Report(f"cmvn_packed cols {cols}")
    for var in (False, True):
        got = ss.cmvn_packed(d, doff, var).cpu().numpy()
        host = ss.cmvn_packed(block, off, var)
        assert np.array_equal(_bits(host), _bits(got)), "the host form and the device form differ"
        for b, x in enumerate(clip_list):
            if x is None:
                continue
            lo, hi = int(off[b]), int(off[b + 1])
            rep.add(f"clip {b} ({hi - lo} rows) var {var}", got[lo:hi], oracle.cmvn(x, var))
            alone = ss.cmvn_packed(torch.from_numpy(np.array(x)).cuda(), np.array([0, hi - lo], np.int64), var).cpu().numpy()
            assert np.array_equal(_bits(alone), _bits(got[lo:hi])), (b, var, "a clip's bits depend on its place in the block")
    rep.done()


# ---------------------------------------------------------------- cmvnw ----------------------------------------------------------

@pytest.mark.parametrize("win", M.CMVNW_WINS)
@pytest.mark.parametrize("cols", M.CMVN_COLS)
def test_cmvnw_one_matrix_and_packed(ss, oracle, cols, win):
    import torch

    clip_list = M.clips(M.CMVNW_ROWS, cols, 4000)
    block, off = M.pack(clip_list, cols)
    d, doff = torch.from_numpy(block).cuda(), torch.from_numpy(off).cuda()
    rep = Report(f"cmvnw cols {cols} win {win}")
    for var in (False, True):
        got = ss.cmvnw_packed(d, doff, win, var).cpu().numpy()
        for b, x in enumerate(clip_list):
            want = oracle.cmvnw(x, win, var)
            assert not var or np.abs(want).max() < M.CMVNW_ORACLE_BOUND
            rep.add(f"packed clip {b} ({x.shape[0]} rows) var {var}", got[off[b]:off[b + 1]], want)
            rep.add(f"one matrix clip {b} var {var}", ss.cmvnw(x, win, var), want)
    rep.done()


@pytest.mark.parametrize("win", (3, 31))
def test_cmvnw_outlier_of_1e6_is_inside_the_documented_domain(ss, oracle, win):
    """The sliding sums keep a rounding residue of a value that has left the window: ulp(v^2) of an outlier v against the window's
    sum of squares.  The header draws the line at about 1e7 times the window's spread; 1e6 in N(1, 3) data is on the good side of it
    (a residue of 2^-53 * 1e12 = 1.1e-4 in a sum of squares of at least 3 * 9, 4e-6 of it).  The rows whose window holds the outlier
    (their column maximum is the outlier's own) and the rows behind it are held separately."""
    rows, row, col = 400, 205, 4
    x = np.array(M.hard_block(rows, 13, 4200))
    assert M.KINDS[col] == "plain"
    x[row, col] = 1e6
    pad = (win - 1) // 2
    rep = Report(f"cmvnw outlier win {win}")
    for var in (False, True):
        want = oracle.cmvnw(x, win, var)
        reach = pad * (2 if var else 1)
        near = np.zeros(rows, bool)
        near[row - reach:row + reach + 1] = True
        packed = ss.cmvnw_packed(x, np.array([0, rows], np.int64), win, var)
        for name, got in (("one matrix", ss.cmvnw(x, win, var)), ("packed", packed)):
            rep.add(f"{name} var {var}, rows that see the outlier", got[near], want[near])
            rep.add(f"{name} var {var}, the other rows", got[~near], want[~near])
    rep.done()


# ---------------------------------------------------------------- the stream pool ------------------------------------------------

def _run_pool(sslib, xs, win, variance):
    """The streams xs (one [T_b, 40] array each) through TICKS -> the rows per stream."""
    import torch

    T = max(x.shape[0] for x in xs)
    s = torch.zeros((POOL, T, M.STREAM_COLS), device="cuda")
    for b, x in enumerate(xs):
        s[b, :x.shape[0]] = torch.from_numpy(np.array(x)).cuda()
    pool = torch.zeros((POOL, (win - 1) * M.STREAM_COLS + 1), device="cuda")
    got = _feed(torch, sslib, s, TICKS, ORDER, pool, SLOTS, win, variance)
    torch.cuda.synchronize()
    return [g.cpu().numpy() for g in got]


def _check_pool(rep, got, xs, win, variance):
    for b, x in enumerate(xs):
        with np.errstate(all="ignore"):
            want, n_t = restate(x, win, variance)
        g = got[b]
        if variance:
            rep.bound(f"stream {b}", g, n_t)
        at = 0
        for k, tick in enumerate(TICKS):  # per entry
            r = tick[b]
            if r:
                rep.add(f"stream {b} tick {k} ({r} rows) var {variance}", g[at:at + r], want[at:at + r])
            at += r
        assert at == x.shape[0]


@pytest.mark.parametrize("win", M.STREAM_WINS)
def test_stream_pool_per_entry(sslib, win):
    xs = M.streams(TICKS)
    assert max(max(t) for t in TICKS) == 400  # 400 rows x 32 columns do not fit the kernel's LDS tile: the global-memory path runs too
    rep = Report(f"stream pool win {win}")
    for variance in (False, True):
        _check_pool(rep, _run_pool(sslib, xs, win, variance), xs, win, variance)
    rep.done()


# ---------------------------------------------------------------- non-finite values ---------------------------------------------

def test_cmvn_with_a_non_finite_value_in_a_column(ss, oracle):
    """Row 37 of 98 is the 13th row of the second chunk (chunks of 25 rows).  Columns 3 and 35 come out non-finite as the oracle's
    do; every other column is held as in the tests above."""
    import torch

    base = M.cmvn_block(98, 40)
    clip_list = [M.poison(base, 37, bad) for bad in M.BAD_VALUES] + [np.array(base)]
    block, off = M.pack(clip_list, 40)
    rep = Report("cmvn non-finite")
    for var in (False, True):
        batch = ss.cmvn(torch.from_numpy(np.stack(clip_list)).cuda(), var).cpu().numpy()
        packed = ss.cmvn_packed(torch.from_numpy(block).cuda(), torch.from_numpy(off).cuda(), var).cpu().numpy()
        for b, x in enumerate(clip_list):
            want = _oracle(oracle.cmvn, x, var)
            assert np.isfinite(want[:, [3, 35]]).any() == (b == 3) and np.isfinite(np.delete(want, [3, 35], axis=1)).all()
            rep.add(f"batch clip {b} var {var}", batch[b], want)
            rep.add(f"packed clip {b} var {var}", packed[off[b]:off[b + 1]], want)
            rep.add(f"one matrix clip {b} var {var}", ss.cmvn(x, var), want)
    rep.done()


@pytest.mark.parametrize("rows,win,row", [(98, 3, 37), (98, 31, 37), (400, 31, 205), (400, 301, 205)])
def test_cmvnw_with_a_non_finite_value_in_a_column(ss, oracle, rows, win, row):
    """The bad row sits in the middle of a chunk that is not the first (chunks of 8 rows, of 19 for win 301).  The oracle is
    non-finite within pad rows of it (2 * pad with variance normalisation) and finite beyond: a value that has left the window must
    leave the sliding sums too, and a window that holds a NaN must not come out as a number."""
    import torch

    base = M.hard_block(rows, 40, 4100)
    clip_list = [M.poison(base, row, bad) for bad in M.BAD_VALUES] + [np.array(base)]
    block, off = M.pack(clip_list, 40)
    rep = Report(f"cmvnw non-finite rows {rows} win {win}")
    for var in (False, True):
        packed = ss.cmvnw_packed(torch.from_numpy(block).cuda(), torch.from_numpy(off).cuda(), win, var).cpu().numpy()
        for b, x in enumerate(clip_list):
            want = _oracle(oracle.cmvnw, x, win, var)
            assert np.isfinite(want[row, 3]) == (b == 3) and np.isfinite(np.delete(want, [3, 35], axis=1)).all()
            rep.add(f"packed clip {b} var {var}", packed[off[b]:off[b + 1]], want)
            rep.add(f"one matrix clip {b} var {var}", ss.cmvnw(x, win, var), want)
    rep.done()


@pytest.mark.parametrize("win", M.STREAM_WINS)
def test_stream_pool_with_a_non_finite_value_in_a_column(sslib, win):
    """NaN in a 37-row entry (the LDS path; the next tick reads it from the pool row), -inf in a 400-row entry (the global-memory
    path), +inf ten rows before the end of a 400-row entry (the last tick meets it in the history only)."""
    xs = [np.array(x) for x in M.streams(TICKS)]
    for b, row, bad in ((4, 20, M.BAD_VALUES[0]), (2, 205, M.BAD_VALUES[1]), (6, 390, M.BAD_VALUES[2])):
        xs[b] = M.poison(xs[b], row, bad)
    rep = Report(f"stream pool non-finite win {win}")
    for variance in (False, True):
        _check_pool(rep, _run_pool(sslib, xs, win, variance), xs, win, variance)
    rep.done()


# ---------------------------------------------------------------- mixed scales, mean only ----------------------------------------

def test_tiny_and_big_columns_in_one_matrix_mean_only(ss, sslib, oracle):
    """Columns of N(0, 1e-3) and N(-3e4, 1e4) side by side: over the block's maximum the small column could be entirely wrong."""
    x = M.hard_block(301, 13, 5000)
    tiny, big = M.KINDS.index("tiny"), M.KINDS.index("big")
    off = np.array([0, 301], np.int64)
    xs = [M.hard_block(t, M.STREAM_COLS, 5000 + b) for b, t in enumerate(M.stream_rows(TICKS))]
    pool = _run_pool(sslib, xs, 31, False)
    cases = [("cmvn", ss.cmvn(x, False), oracle.cmvn(x, False)),
             ("cmvn_packed", ss.cmvn_packed(x, off, False), oracle.cmvn(x, False)),
             ("cmvnw 31", ss.cmvnw(x, 31, False), oracle.cmvnw(x, 31, False)),
             ("cmvnw_packed 31", ss.cmvnw_packed(x, off, 31, False), oracle.cmvnw(x, 31, False)),
             ("pool 31, stream 4", pool[4], restate(xs[4], 31, False)[0])]
    worst = 0.0
    for name, got, want in cases:
        e = M.col_rel(got, want)
        assert np.abs(want[:, big]).max() > 1e6 * np.abs(want[:, tiny]).max()
        print(f"{name}: tiny {e[tiny]:.3g}, big {e[big]:.3g}, all columns {e.max():.3g}")
        worst = max(worst, float(e.max()))
    assert worst <= RTOL
