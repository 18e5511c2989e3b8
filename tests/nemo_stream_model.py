"""The pool and flush semantics of the ss_nstream_* comment of include/speechsauce_amd.h restated in numpy f64, on the pieces of
tests/nemo_model.py (the window, the bank, the guard, step 2's arithmetic): which samples a pool row reads (the pool row's tail, the
chunk's head, the one pre-emphasis predecessor), how the pool row moves on, and which positions the flush masks.  The rows of a frame
are formed one frame at a time (rows_of), so a row's bits do not depend on how many rows share a call: the cuts of one stream compare
EQUAL here; against nemo_model.log_mel, whose mel product is one BLAS call over all rows of a clip, the comparison carries TOL."""
import numpy as np

import nemo_model as nm

HOP = nm.HOP
WINDOWS = (258, 320, 322, 400, 416, 480, 512)
# |ln row - ln row'| where the two differ only in the order of f64 additions: a mel sum has at most 257 terms of relative error
# 2^-53 each, the guard keeps the logarithm's argument above 2^-24 times nothing smaller -- 1e-9 is more than 10^4 times that bound
# and 10^5 times below the GPU tests' bar
TOL = 1e-9


def sizes(W):
    """-> (S, L): the carried samples per stream and the delay in rows (ss_nstream_state_len)"""
    L = -(-W // (2 * HOP)) - 1
    return L * HOP + W // 2 + 1, L


def rows_of(y, n_mels, W):
    """steps 3 - 6 on pre-emphasised frames y [R x W] (f64), one frame at a time -> [R x n_mels]"""
    B = nm.mel_bank(n_mels).astype(np.float32).astype(np.float64)
    w = nm.window(W)
    out = np.empty((len(y), n_mels))
    for r, frame in enumerate(y):
        P = np.abs(np.fft.rfft(frame * w, n=nm.N_FFT)) ** 2
        out[r] = np.log((B * P[None, :]).sum(axis=1) + nm.GUARD)
    return out


class Pool:
    """One stream's state and calls: push(chunk) -> its R rows, flush() -> its L rows"""

    def __init__(self, n_mels, W=400, c=nm.PREEMPH):
        self.n_mels, self.W, self.c = n_mels, W, c
        self.S, self.L = sizes(W)
        self.state = np.zeros(self.S, np.float32)  # an all-zero row is a fresh stream

    def _frames(self, line, origin, starts, lim):
        """the frames whose first live samples are positions `starts` of `line` (position p is line[origin + p]); position n of a frame
        is zero AFTER the pre-emphasis where n >= lim"""
        line = np.asarray(line, np.float64)
        y = np.zeros((len(starts), self.W))
        for r, p0 in enumerate(starts):
            live = min(self.W, lim[r])
            seg = line[origin + p0 - 1:origin + p0 + live]  # the predecessor of the first sample is position p0 - 1
            y[r, :live] = seg[1:] - self.c * seg[:-1]
        return y

    def push(self, chunk):
        chunk = np.asarray(chunk, np.float32)
        assert chunk.size % HOP == 0, "an entry is whole hops"
        R = chunk.size // HOP
        both = np.concatenate([self.state, chunk])  # position p of the chunk is both[S + p]; p < 0 is the pool row
        starts = [HOP * (t - self.L) - self.W // 2 for t in range(R)]
        assert all(-self.S <= p0 - 1 and p0 + self.W <= HOP * (t + 1) for t, p0 in enumerate(starts))  # nothing is masked
        rows = rows_of(self._frames(both, self.S, starts, [self.W] * R), self.n_mels, self.W)
        self.state = both[both.size - self.S:]
        return rows

    def flush(self):
        starts = [HOP * (u - self.L) - self.W // 2 for u in range(self.L)]
        rows = rows_of(self._frames(self.state, self.S, starts, [-p0 for p0 in starts]), self.n_mels, self.W)
        self.state = np.zeros(self.S, np.float32)
        return rows


def serve(stream, cuts, n_mels, W=400, c=nm.PREEMPH):
    """a stream of whole hops cut into calls of `cuts` hops -> (the pool rows [K x n_mels], the flush rows [L x n_mels], the pool row
    in front of the flush)"""
    pool = Pool(n_mels, W, c)
    rows, at = [np.empty((0, n_mels))], 0
    for hops in cuts:
        rows.append(pool.push(stream[at:at + hops * HOP]))
        at += hops * HOP
    assert at == len(stream)
    state = pool.state.copy()
    tail = pool.flush()
    assert not pool.state.any()
    return np.concatenate(rows), tail, state


def three_cuts(K):
    """one call; two calls; one-hop calls with empty calls between them"""
    one_hop = [v for _ in range(K) for v in (1, 0)]
    return [[K], [K // 2, K - K // 2], one_hop]
