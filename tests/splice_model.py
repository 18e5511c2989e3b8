"""What tests/test_splice_cpu.py and tests/test_splice.py share: the numpy restatement of the ss_splice_* section of
include/speechsauce_amd.h, a numpy model of the pool of stream states, FunASR's apply_lfr restated, the parameter sets and seeded
inputs salted with the values an arithmetic instruction would change.  Everything is compared on uint32 views: the stage copies bits.
"""
import functools

import numpy as np

# (left, right, stride): D = right // stride, H = D * stride + left
PARAMS = ((5, 5, 1), (3, 3, 6), (0, 0, 3), (2, 0, 1), (0, 4, 1), (1, 6, 6), (4, 7, 3), (0, 2, 4), (3, 12, 5), (0, 0, 1))
LFR = ((7, 6), (5, 3), (3, 1), (1, 4))
SENTINEL = np.uint32(0xDEADBEEF)  # as a float: about -6.26e18; never among the inputs


def u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def splice_ref(x, left, right, s):
    """The definition on ONE clip, the header's own text: x [T, cols] -> [ceil(T / s), (left + 1 + right) * cols]."""
    T = len(x)
    return np.stack([np.concatenate([x[min(max(k * s + c, 0), T - 1)] for c in range(-left, right + 1)])
                     for k in range(-(-T // s))]) if T else np.zeros((0, (left + 1 + right) * x.shape[1]), x.dtype)


def apply_lfr(inputs, lfr_m, lfr_n):
    """FunASR's apply_lfr (funasr/frontends/wav_frontend.py), restated in numpy: left padding with (m - 1) // 2 copies of the first
    frame, T_lfr = ceil(T / n) windows of m frames every n, the last ones filled up with the last frame."""
    T = inputs.shape[0]
    if T == 0:
        return np.zeros((0, lfr_m * inputs.shape[1]), inputs.dtype)
    T_lfr = int(np.ceil(T / lfr_n))
    padded = np.vstack([np.tile(inputs[0], ((lfr_m - 1) // 2, 1)), inputs])
    T = T + (lfr_m - 1) // 2
    out = []
    for i in range(T_lfr):
        if lfr_m <= T - i * lfr_n:
            out.append(padded[i * lfr_n:i * lfr_n + lfr_m].reshape(-1))
        else:
            frame = padded[i * lfr_n:].reshape(-1)
            for _ in range(lfr_m - (T - i * lfr_n)):
                frame = np.hstack([frame, padded[-1]])
            out.append(frame)
    return np.stack(out)


def delay_hist(left, right, stride):
    D = right // stride
    return D, D * stride + left


class StreamModel:
    """The pool calls on one stream: the last H raw rows are kept; output row k of a push is centred on row count + (k - D) * stride of
    (history ++ new rows), all +0.0 while that is negative."""

    def __init__(self, cols, left, right, stride):
        self.cols, self.left, self.right, self.stride = cols, left, right, stride
        self.D, self.H = delay_hist(left, right, stride)
        self.ocols = (left + 1 + right) * cols
        self.hist = np.zeros((0, cols), np.float32)

    def _rows(self, buf, n_out, count, last):
        out = np.zeros((n_out, self.ocols), np.float32)
        for k in range(n_out):
            v = count + (k - self.D) * self.stride
            if v >= 0:
                out[k] = buf[np.clip(v + np.arange(-self.left, self.right + 1), 0, last)].reshape(-1)
        return out

    def push(self, new):
        assert len(new) % self.stride == 0
        if len(new) == 0:
            return np.zeros((0, self.ocols), np.float32)
        count = len(self.hist)
        buf = np.concatenate([self.hist, new])
        out = self._rows(buf, len(new) // self.stride, count, len(buf) - 1)
        self.hist = buf[len(buf) - min(len(buf), self.H):]
        return out

    def flush(self):
        count = len(self.hist)
        out = self._rows(self.hist, self.D, count, count - 1)
        self.hist = np.zeros((0, self.cols), np.float32)
        return out

    def pool_row(self):
        """the stream's pool row as the header lays it out"""
        row = np.zeros(self.H * self.cols + 1, np.float32)
        if len(self.hist):
            row[(self.H - len(self.hist)) * self.cols:-1] = self.hist.reshape(-1)
        row[-1] = len(self.hist)
        return row


@functools.lru_cache(maxsize=None)
def clip(cols, T, seed=0):
    """Seeded rows [T, cols], float32, never modified; about one value in six is one that arithmetic would not carry through: NaNs with
    distinct payloads (quiet and signalling, both signs), -0.0, +-inf and denormals."""
    rng = np.random.default_rng(100003 * cols + 1009 * T + seed)
    bits = u32((rng.standard_normal((T, cols)) * 3 + 1).astype(np.float32)).copy().reshape(-1)
    n = bits.size
    at = np.flatnonzero(rng.random(n) < 1 / 6)
    i = np.arange(at.size, dtype=np.uint32)
    special = np.choose(i % 8, [np.uint32(0x7FC00000) | (i + 1) & 0x3FFFFF,       # quiet NaN, payload i + 1
                                np.uint32(0xFFC00000) | (i + 1) & 0x3FFFFF,       # the same, sign set
                                np.uint32(0x7F800000) | ((i + 1) & 0x3FFFFF),     # signalling NaN (payload != 0)
                                np.full(i.size, 0x80000000, np.uint32),            # -0.0
                                np.full(i.size, 0x7F800000, np.uint32),            # +inf
                                np.full(i.size, 0xFF800000, np.uint32),            # -inf
                                (i + 1) & 0x7FFFFF,                                # denormals
                                np.uint32(0x80000000) | ((i + 1) & 0x7FFFFF)]).astype(np.uint32)
    bits[at] = special
    assert not (bits == SENTINEL).any()
    x = bits.view(np.float32).reshape(T, cols)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def want(cols, T, left, right, stride, seed=0):
    w = splice_ref(clip(cols, T, seed), left, right, stride)
    w.setflags(write=False)
    return w
