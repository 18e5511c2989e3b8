"""What tests/test_reverb_cpu.py and tests/test_reverb.py share: the numpy restatement of the ss_reverb_* section of
include/speechsauce_amd.h -- the draws (Philox4x32-10 of specaug_model in integers), the normalisation of a response in f64, the
partition spectra by numpy's f64 FFT and the output as the f64 direct sum -- and the shapes the device tests run on.
"""
import numpy as np

from specaug_model import MASK32, philox

ROW = np.dtype([("rir", np.int32), ("shift", np.int32)])
STREAM = 0x30000
LIMIT = 1 << 31
B, N, MAX_TAPS = 512, 1024, 16384
BAR = 1e-4  # max |got - want| / max |want| per clip: the project's block metric and bar
# the worked pin of the header: seed 2026, epoch 0, clip_base 0, prob 0.5, five responses with peaks at 0, 7, 100, 3 and 11, aligned,
# three clips of 16000 samples
PIN_PEAKS = (0, 7, 100, 3, 11)
PIN_ROWS = [(2, 100), (-1, 0), (0, 0)]


def table(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


def good(lo, hi, total):
    return 0 <= lo <= hi <= total and hi - lo < LIMIT


def draws_ref(rng, clip_base, so, total, shifts, prob):
    """Every clip's row; `shifts` is the handle's shift of every response."""
    seed, epoch = (int(v) & (2 ** 64 - 1) for v in rng)
    so = np.asarray(so, np.int64)
    n, n_rir = len(so) - 1, len(shifts)
    plan = np.zeros(n, ROW)
    ids = (int(clip_base) + np.arange(n, dtype=np.int64)) & MASK32
    key, e = (seed & MASK32, seed >> 32), (epoch & MASK32, epoch >> 32)
    u = philox((ids, np.full(n, STREAM), e[0], e[1]), key) if n else [np.zeros(0, np.uint32)] * 4
    bar = int(np.float64(np.float32(prob)) * 4294967296.0)
    for b in range(n):
        if not good(int(so[b]), int(so[b + 1]), total):
            plan[b] = (-2, 0)
        elif n_rir == 0 or not int(u[0][b]) < bar:
            plan[b] = (-1, 0)
        else:
            c = (int(u[1][b]) * n_rir) >> 32
            plan[b] = (c, shifts[c])
    return plan


def normalise(h, mode):
    """-> (taps f32, peak): mode 0 as given, 1 unit energy, 2 unit peak; squares, their sum in ascending order, root and quotient in f64"""
    h = np.asarray(h, np.float32)
    v = h.astype(np.float64)
    peak = int(np.argmax(np.abs(v)))  # the first index of the maximum
    div = {0: 1.0, 1: np.sqrt(np.cumsum(v * v)[-1]), 2: np.abs(v[peak])}[mode]  # cumsum adds one by one
    return (h if mode == 0 or not div > 0 else (v / div).astype(np.float32)), peak


def spectrum_ref(taps, p):
    """partition p of a response, zero-padded to N points, by numpy's f64 FFT"""
    z = np.zeros(N)
    seg = np.asarray(taps, np.float64)[p * B:(p + 1) * B]
    z[:seg.size] = seg
    return np.fft.fft(z)


def conv_ref(x, taps, shift):
    """out[i] = sum_k h[k] x[i + shift - k], i < len(x), in f64: np.convolve, shifted and trimmed"""
    x, taps = np.asarray(x, np.float64), np.asarray(taps, np.float64)
    if x.size == 0:
        return np.zeros(0)
    full = np.convolve(x, taps)  # len(x) + K - 1; shift < K
    return full[shift:shift + x.size]


def block_error(got, want):
    """max |got - want| / max |want| (0 where both are all zero)"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    if got.size == 0:
        return 0.0
    top = np.abs(want).max()
    err = np.abs(got - want).max()
    return float(err / top) if top > 0 else float(err)


def speech(lens, kind, seed=0):
    """packed float32 clips: Gaussian noise at 0.1, or a 440 Hz tone at 0.5 (16 kHz), every clip from its own phase 0"""
    if kind == "noise":
        return (np.random.default_rng(seed).standard_normal(int(np.sum(lens))) * 0.1).astype(np.float32)
    return np.concatenate([0.5 * np.sin(2 * np.pi * 440.0 * np.arange(n) / 16000.0) for n in lens] + [np.zeros(0)]).astype(np.float32)


def response(k, peak, seed):
    """an exponentially decaying noise tail of k taps with its largest tap, 1.0, at `peak`"""
    r = np.random.default_rng(1000 + seed)
    h = (r.standard_normal(k) * 0.3 * np.exp(-np.arange(k) / max(k / 4.0, 1.0))).astype(np.float32)
    h = np.clip(h, -0.9, 0.9)
    h[peak] = 1.0
    return h


# The device shapes, with B the kernel's block: clip lengths around every multiple of B a block pair can end at, one clip of more
# than one workgroup pass (4B + 1 is below that: 5000 is not a multiple of anything), and an empty clip
CLIP_LENS = [0, 1, B - 1, B, B + 1, 2 * B - 1, 2 * B, 2 * B + 1, 4 * B + 1, 5000]
# response lengths around one and two partitions, and the peaks: index 0, mid-response, last tap
RIR_LENS = [1, 2, B - 1, B, B + 1, 2 * B + 1, 3000]
RIR_PEAKS = [0, 1, (B - 1) // 2, B - 1, 0, 2 * B, 1500]
LONG_RIR, LONG_CLIP = MAX_TAPS, 3000
