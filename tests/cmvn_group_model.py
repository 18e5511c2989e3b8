"""What tests/test_cmvn_group_cpu.py and tests/test_cmvn_group.py share: the numpy restatement of grouped CMVN as the "grouped CMVN"
comment of include/speechsauce_amd.h defines it (per-clip statistics in the order of cmvn_model._chunk_sums, the left fold, the
apply, the Kaldi accumulator conversions), a two-pass longdouble reference on a group's concatenated rows, and the case both files
run on.  No device is touched here.

numpy rounds every operation on its own and has no fused multiply-add, which is what the merge and the apply are defined as; the
per-clip statistics are a restatement of the formula (the kernels fuse the products of their sums), as in cmvn_model.
"""
import numpy as np

import cmvn_model as M

EPS = M.EPS


def stats_len(cols):
    return 2 * cols + 1


def clip_stats(x):
    """-> (T, mean[cols], var[cols]) of one clip [T, cols] float32: s1 and s2 of cmvn_model._chunk_sums about the clip's first row K,
    mean = s1 / T, var = max(s2 / T - (mean - K)^2, 0)  (a NaN passes the max)."""
    x64 = np.asarray(x, np.float64)
    T = x64.shape[0]
    K = x64[0]
    with np.errstate(all="ignore"):
        s1, s2 = M._chunk_sums(x64, K)
        mean = s1 / T
        d = mean - K
        var = s2 / T - d * d
        var = np.where(var < 0.0, 0.0, var)
    return T, mean, var


def count(n):
    """a count word as the kernels read it: not finite or below 1 is 0"""
    return float(n) if np.isfinite(n) and n >= 1.0 else 0.0


def merge(row, T, mb, vb):
    """The left fold's step: statistics row [n | mean | var] merged with a clip's (T, mean, var) -> a new row.  Every operation is one
    numpy operation, in the header's order."""
    cols = len(mb)
    na = count(row[0])
    out = np.empty(stats_len(cols))
    if na == 0.0:
        out[0], out[1:1 + cols], out[1 + cols:] = float(T), mb, vb
        return out
    ma, va = row[1:1 + cols], row[1 + cols:]
    with np.errstate(all="ignore"):
        nb = np.float64(T)
        n = np.float64(na) + nb
        wa = np.float64(na) / n
        wb = nb / n
        d = mb - ma
        out[0] = n
        out[1:1 + cols] = ma + d * wb
        out[1 + cols:] = (wa * va + wb * vb) + (d * d) * (wa * wb)
    return out


def valid(off, groups, b, total_rows, n_groups):
    lo, hi = int(off[b]), int(off[b + 1])
    g = 0 if groups is None else int(groups[b])
    return 0 <= lo < hi <= total_rows and 0 <= g < n_groups


def fold(block, off, groups, n_groups, stats=None, per_clip=None):
    """ss_cmvn_stats_packed: -> the updated [n_groups, 2 cols + 1] block (a copy).  per_clip[b] = (T, mean, var) replaces the
    restated statistics of clip b where given (the device's own per-clip rows)."""
    cols = block.shape[1]
    st = np.zeros((n_groups, stats_len(cols))) if stats is None else np.array(stats, np.float64)
    for b in range(len(off) - 1):
        if not valid(off, groups, b, block.shape[0], n_groups):
            continue
        g = 0 if groups is None else int(groups[b])
        T, mb, vb = per_clip[b] if per_clip is not None else clip_stats(block[int(off[b]):int(off[b + 1])])
        st[g] = merge(st[g], T, mb, vb)
    return st


def apply_rows(x, row, variance):
    """(float)(((double)x - mean) * inv), inv = 1 / (sqrt(var) + 2^-30) or 1"""
    cols = x.shape[1]
    with np.errstate(all="ignore"):
        inv = 1.0 / (np.sqrt(row[1 + cols:]) + EPS) if variance else np.ones(cols)
        return ((np.asarray(x, np.float64) - row[1:1 + cols]) * inv).astype(np.float32)


def apply(block, off, groups, stats, variance, out):
    """ss_cmvn_apply_packed on a copy of `out`: skipped clips keep out's rows"""
    out = np.array(out, np.float32)
    st = np.asarray(stats, np.float64).reshape(-1, stats_len(block.shape[1]))
    for b in range(len(off) - 1):
        if not valid(off, groups, b, block.shape[0], st.shape[0]):
            continue
        g = 0 if groups is None else int(groups[b])
        if count(st[g, 0]) == 0.0:
            continue
        lo, hi = int(off[b]), int(off[b + 1])
        out[lo:hi] = apply_rows(block[lo:hi], st[g], variance)
    return out


def to_kaldi(row):
    cols = (len(row) - 1) // 2
    n = count(row[0])
    k = np.zeros((2, cols + 1))
    if n > 0.0:
        mean, var = row[1:1 + cols], row[1 + cols:]
        k[0, :cols] = n * mean
        k[1, :cols] = n * (var + mean * mean)
    k[0, cols] = n
    return k


def from_kaldi(k):
    k = np.asarray(k, np.float64).reshape(2, -1)
    cols = k.shape[1] - 1
    n = count(k[0, cols])
    row = np.zeros(stats_len(cols))
    if n > 0.0:
        mean = k[0, :cols] / n
        var = k[1, :cols] / n - mean * mean
        row[0], row[1:1 + cols], row[1 + cols:] = n, mean, np.where(var < 0.0, 0.0, var)
    return row


def two_pass(rows, variance):
    """The reference: mean and population deviation of a group's concatenated rows in two passes of longdouble, then the apply's
    formula -> float64 (not rounded to float32: the reference is not the thing under test)."""
    x = np.asarray(rows, np.longdouble)
    with np.errstate(all="ignore"):
        mean = x.sum(axis=0) / x.shape[0]
        c = x - mean
        if not variance:
            return np.asarray(c, np.float64)
        std = np.sqrt((c * c).sum(axis=0) / x.shape[0])
        return np.asarray(c / (std + np.longdouble(EPS)), np.float64)


# ---------------------------------------------------------------- the case -------------------------------------------------------

SHORT = 300          # clips of 1 .. 5 rows behind the eight of cmvn_model.PACKED_ROWS
N_GROUPS = 5         # 0 and 1 interleave the long clips, 2 holds the short clips, 3 has no clip; clip LEFT_OUT has id -1
LEFT_OUT = 7         # the 5-row clip


def case_rows():
    short = np.random.default_rng(77).integers(1, 6, SHORT)
    return list(M.PACKED_ROWS) + [int(r) for r in short]


def case(cols):
    """-> (clip list, block, offsets, groups int32)"""
    rows = case_rows()
    clip_list = M.clips(rows, cols, 7000)
    block, off = M.pack(clip_list, cols)
    groups = np.full(len(rows), 2, np.int32)
    groups[:len(M.PACKED_ROWS)] = [0, 1, 0, 1, 0, 1, 0, -1]  # 98 0 1 2 301 1598 2100 5 rows
    return clip_list, block, off, groups


def group_rows(clip_list, groups, g):
    """the concatenated rows of group g, and for every member clip its slice of them"""
    members = [b for b, x in enumerate(clip_list) if x is not None and groups[b] == g]
    rows = np.concatenate([clip_list[b] for b in members]) if members else None
    at, where = 0, {}
    for b in members:
        where[b] = slice(at, at + clip_list[b].shape[0])
        at += clip_list[b].shape[0]
    return rows, where
