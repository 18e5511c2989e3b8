"""What tests/test_vad_cpu.py and tests/test_vad.py share: the numpy restatement of the ss_vad_* / ss_select_rows_* section of
include/speechsauce_amd.h, a numpy model of the pool of stream states, the parameter sets and seeded inputs.  Masks are compared byte
for byte, selected rows on uint32 views (splice_model.clip salts them with the values an arithmetic instruction would change).
"""
import functools

import numpy as np

from splice_model import SENTINEL, clip, u32  # noqa: F401  (re-exported for the tests)

# (energy_threshold, energy_mean_scale, frames_context, proportion_threshold)
KALDI_DEFAULT = (5.0, 0.5, 0, 0.6)
XVECTOR = (5.5, 0.5, 2, 0.12)
PARAMS = (KALDI_DEFAULT, XVECTOR, (5.0, 0.0, 3, 0.6), (-2.5, 0.75, 1, 0.5), (4.0, 0.5, 32, 0.3), (5.0, 0.5, 2, 0.01), (5.0, 0.5, 2, 0.99))
MASK_SENTINEL = 0xA5  # never 0 or 1


def cmvn_sum(e):
    """The order in which ss_cmvn_packed_kernel sums one column of T >= 1 rows, in float64: min(64, ceil(T / 32)) chunks of ceil(T /
    chunks) rows, each summed serially, the chunk sums added serially in chunk order."""
    T = len(e)
    chunks = min(64, -(-T // 32))
    rpc = -(-T // chunks)
    s1 = np.float64(0.0)
    with np.errstate(all="ignore"):
        for k in range(chunks):
            part = np.float64(0.0)
            for v in np.asarray(e[k * rpc:min(T, (k + 1) * rpc)], np.float64):
                part = part + v
            s1 = s1 + part
    return s1


def cmvn_mean(e):
    with np.errstate(all="ignore"):
        return cmvn_sum(e) / np.float64(len(e))


def threshold(thr, scale, mean):
    """thr + scale * mean in float64: a rounded product and a rounded sum; the mean is not looked at where scale == 0"""
    if np.float32(scale) == 0:
        return np.float64(np.float32(thr))
    with np.errstate(all="ignore"):
        return np.float64(np.float32(thr)) + np.float64(np.float32(scale)) * np.float64(mean)


def decide(num, den, p):
    """(float)num >= (float)den * p with ONE float32 product"""
    return np.float32(num) >= np.float32(den) * np.float32(p)


def window_mask(raw, L, p):
    T = len(raw)
    out = np.zeros(T, np.uint8)
    for t in range(T):
        lo, hi = max(t - L, 0), min(t + L, T - 1)
        out[t] = decide(int(raw[lo:hi + 1].sum()), hi - lo + 1, p)
    return out


def vad_ref(x, col, thr, scale, L, p):
    """The definition on ONE clip, the header's own text: x [T, cols] -> uint8 [T]."""
    e = np.asarray(x, np.float32)[:, col]
    if len(e) == 0:
        return np.zeros(0, np.uint8)
    th = threshold(thr, scale, cmvn_mean(e) if np.float32(scale) != 0 else 0.0)
    with np.errstate(invalid="ignore"):
        raw = e.astype(np.float64) > th
    return window_mask(raw, L, p)


def select_ref(x, ro, mask):
    """x[mask != 0] clip by clip and the table of the result (for a gap-free table: x[mask != 0] and the running kept counts)"""
    keep = np.asarray(mask) != 0
    counts = [int(keep[ro[b]:ro[b + 1]].sum()) for b in range(len(ro) - 1)]
    rows = [x[ro[b]:ro[b + 1]][keep[ro[b]:ro[b + 1]]] for b in range(len(ro) - 1)]
    out = np.concatenate(rows) if rows else x[:0]
    return out, np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)


class VadStreamModel:
    """The pool calls on one stream.  Every energy is kept (a model need not forget); S is the ONE float64 accumulator, advanced row by
    row in stream order; the decision for row t compares the window's members with thr + scale * (S_n / n), n = min(t + L + 1, seen)."""

    def __init__(self, col, thr, scale, L, p):
        self.col, self.thr, self.scale, self.L, self.p = col, thr, scale, L, p
        self.reset()

    def reset(self):
        self.e = np.zeros(0, np.float32)
        self.sums = []  # sums[n - 1] = S_n

    def _decision(self, t, n, last):
        with np.errstate(all="ignore"):
            th = threshold(self.thr, self.scale, self.sums[n - 1] / np.float64(n))
            lo, hi = max(t - self.L, 0), min(t + self.L, last)
            raw = self.e[lo:hi + 1].astype(np.float64) > th
        return decide(int(raw.sum()), hi - lo + 1, self.p)

    def push(self, rows):
        new = np.asarray(rows, np.float32)[:, self.col]
        N = len(self.e)
        with np.errstate(all="ignore"):
            for v in new.astype(np.float64):
                self.sums.append((self.sums[-1] if self.sums else np.float64(0.0)) + v)
        self.e = np.concatenate([self.e, new])
        out = np.zeros(len(new), np.uint8)
        for k in range(len(new)):
            t = N + k - self.L
            if t >= 0:
                out[k] = self._decision(t, t + self.L + 1, len(self.e) - 1)
        return out

    def flush(self):
        N = len(self.e)
        out = np.zeros(self.L, np.uint8)
        for j in range(self.L):
            t = N - self.L + j
            if t >= 0:
                out[j] = self._decision(t, N, N - 1)
        self.reset()
        return out

    def pool_row(self):
        """the stream's pool row as the header lays it out"""
        H = 2 * self.L
        row = np.zeros(H + 4, np.float32)
        bits = row.view(np.uint32)
        s = np.array([self.sums[-1] if self.sums else 0.0], np.float64).view(np.uint32)  # little endian: low half first
        bits[0], bits[1] = s[0], s[1]
        bits[2] = len(self.e) & 0xFFFFFFFF
        keep = min(len(self.e), H)
        if keep:
            row[3 + H - keep:3 + H] = self.e[len(self.e) - keep:]
        row[-1] = keep
        return row


def causal_ref(e, thr, scale, L, p):
    """A second writing of the stream's bytes (the flush included, the first L dropped) for a whole clip of energies: np.cumsum in
    float64 is sequential, which is the accumulator's order."""
    e = np.asarray(e, np.float32)
    T = len(e)
    with np.errstate(all="ignore"):
        S = np.cumsum(e.astype(np.float64))
    out = np.zeros(T, np.uint8)
    for t in range(T):
        n = min(t + L + 1, T)
        with np.errstate(all="ignore"):
            th = threshold(thr, scale, S[n - 1] / np.float64(n))
            lo, hi = max(t - L, 0), min(t + L, T - 1)
            num = int((e[lo:hi + 1].astype(np.float64) > th).sum())
        out[t] = decide(num, hi - lo + 1, p)
    return out


@functools.lru_cache(maxsize=None)
def energies(T, seed=0, centre=5.0, spread=2.0):
    """Seeded log-energies [T] float32 that straddle `centre`, in runs (speech comes in runs), with a few exactly on it."""
    rng = np.random.default_rng(7919 * T + seed)
    run = np.repeat(rng.standard_normal(T // 5 + 1), 5)[:T]
    e = (centre + spread * (0.7 * run + 0.3 * rng.standard_normal(T))).astype(np.float32)
    e[rng.random(T) < 0.02] = np.float32(centre)
    e.setflags(write=False)
    return e


@functools.lru_cache(maxsize=None)
def feature_clip(cols, T, col, seed=0, centre=5.0):
    """Rows [T, cols] whose column `col` is energies(T, seed) and whose other columns are splice_model.clip's salted values (NaNs,
    infinities, denormals: the decision must not look at them)."""
    x = clip(cols, T, seed).copy()
    x[:, col] = energies(T, seed, centre)
    x.setflags(write=False)
    return x
