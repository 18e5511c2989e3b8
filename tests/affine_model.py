"""What tests/test_splice_affine_cpu.py and tests/test_splice_affine.py share: an exact f32 fmaf in numpy, the numpy restatement of
the ss_affine_* section of include/speechsauce_amd.h built on splice_model.splice_ref (ONE serial fmaf chain per output element over
k = 0 .. K4 - 1 ascending, both factors +0.0 in the pad steps), the same product in f64, the per-element bar between the two, the
shapes and the seeded inputs.

fmaf.  The product of two f32 is exact in f64 (48 significant bits).  Its sum with the f32 addend is formed in f64 with the TwoSum
error term and ROUNDED TO ODD (an inexact sum whose last bit is even moves to its neighbour on the error's side), then rounded to
f32: 53 >= 2 * 24 + 2 bits, so the second rounding sees what a single rounding of the exact value would (Boldo & Melquiond, "Emulation
of FMA and correctly rounded sums", 2008).  Held against libm's fmaf through ctypes in the CPU tests, ties and denormals included.
"""
import functools

import numpy as np

from splice_model import splice_ref, u32  # noqa: F401  (u32 is re-exported)

# (cols, left, right, stride, out_dim): K = (left + 1 + right) * cols; the first has K = 91 -> K4 = 92, the last in_dim = 4096
SHAPES = ((13, 3, 3, 1, 40), (40, 5, 5, 1, 40), (80, 3, 3, 6, 32), (1, 0, 0, 1, 1), (13, 0, 0, 1, 17), (23, 2, 0, 1, 16), (40, 0, 4, 3, 256))
SHAPE_4096 = (128, 15, 16, 1, 8)
# one block: row tiles of 16 straddle clips, clips without rows lie among them
LENS = (1, 0, 2, 15, 16, 0, 0, 17, 31, 33, 0, 100)
SENTINEL = np.uint32(0xDEADBEEF)


def fmaf(a, b, c):
    """fmaf(a, b, c) elementwise on float32 arrays, correctly rounded, in numpy."""
    a, b, c = (np.asarray(v, np.float32) for v in (a, b, c))
    with np.errstate(all="ignore"):
        p = a.astype(np.float64) * b.astype(np.float64)  # exact
        c64 = c.astype(np.float64)
        s = p + c64
        bb = s - p
        err = (p - (s - bb)) + (c64 - bb)                # TwoSum: p + c == s + err exactly (finite s)
        inexact = np.isfinite(s) & (err != 0)
        even = (s.view(np.uint64) & np.uint64(1)) == 0
        toward = np.where(err > 0, np.inf, -np.inf)
        s = np.where(inexact & even, np.nextafter(s, toward), s)  # round to odd
        return s.astype(np.float32)


def chain_len(K):
    return 4 * -(-K // 4)


def chain(s, M, bias=None):
    """The header's chain on spliced rows s [R, K]: -> [R, out_dim] float32.  acc = bias (+0.0 without one); K4 steps, the pad steps
    on +0.0 factors."""
    R, K = s.shape
    acc = np.zeros((R, M.shape[0]), np.float32) if bias is None else np.broadcast_to(np.asarray(bias, np.float32), (R, M.shape[0])).copy()
    zero = np.zeros((), np.float32)
    for k in range(chain_len(K)):
        acc = fmaf(M[None, :, k], s[:, k, None], acc) if k < K else fmaf(zero, zero, acc)
    return acc


def affine_ref(x, M, bias, left, right, stride):
    """One clip x [T, cols] -> [ceil(T / stride), out_dim]: the chain on the rows splice_ref defines."""
    return chain(splice_ref(x, left, right, stride), M, bias)


def affine_f64(x, M, bias, left, right, stride):
    """The same product in f64 and the per-element bar (K4 + 1) * 2^-24 * (|bias_i| + sum_k |M_ik| |s_k|): every one of the K4 chain
    steps rounds once, by at most 2^-24 of a partial sum that is itself at most (1 + 2^-24)^k times the sum of magnitudes.  The
    roundings are taken as RELATIVE, so the bar holds for data whose products and sums do not underflow: the tests that use it
    switch the denormals of the seeded inputs off (-0.0 stays)."""
    s = splice_ref(x, left, right, stride).astype(np.float64)
    M64 = M.astype(np.float64)
    b = np.zeros(M.shape[0]) if bias is None else np.asarray(bias, np.float64)
    ref = s @ M64.T + b
    bar = (chain_len(s.shape[1]) + 1) * 2.0 ** -24 * (np.abs(s) @ np.abs(M64).T + np.abs(b))
    return ref, bar


@functools.lru_cache(maxsize=None)
def rows(cols, T, seed=0, denormals=True):
    """Seeded rows [T, cols], finite and normal, about one value in eight -0.0, +0.0 or (unless switched off) a denormal; never
    modified."""
    rng = np.random.default_rng(7919 * cols + 31 * T + seed)
    x = (rng.standard_normal((T, cols)) * 2).astype(np.float32)
    kind = rng.integers(0, 24, (T, cols))
    x[kind == 0] = -0.0
    x[kind == 1] = 0.0
    den = (rng.integers(1, 1 << 23, (T, cols)).astype(np.uint32) | (rng.integers(0, 2, (T, cols)).astype(np.uint32) << 31)).view(np.float32)
    x = np.where((kind == 2) & denormals, den, x)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def matrix(out_dim, K, seed=0, denormals=True):
    """Seeded M [out_dim, K] and bias [out_dim]; some weights -0.0 and (unless switched off) denormal, some bias entries -0.0."""
    rng = np.random.default_rng(104729 * out_dim + K + seed)
    M = (rng.standard_normal((out_dim, K)) / np.sqrt(K)).astype(np.float32)
    kind = rng.integers(0, 32, M.shape)
    M[kind == 0] = -0.0
    M = np.where((kind == 1) & denormals, np.float32(1e-41), M).astype(np.float32)
    bias = rng.standard_normal(out_dim).astype(np.float32)
    bias[::5] = -0.0
    M.setflags(write=False)
    bias.setflags(write=False)
    return M, bias


def block(cols, lens=LENS, seed=0, denormals=True):
    """-> (clips, row_offsets): the clips of one packed block"""
    clips = [rows(cols, T, seed + i, denormals) for i, T in enumerate(lens)]
    return clips, np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


@functools.lru_cache(maxsize=None)
def want(shape, with_bias, lens=LENS, seed=0):
    """The model's output for block(cols, lens, seed) under matrix(out_dim, K): the clips' rows in order."""
    cols, left, right, stride, out_dim = shape
    M, bias = matrix(out_dim, (left + 1 + right) * cols)
    w = np.concatenate([affine_ref(c, M, bias if with_bias else None, left, right, stride) for c in block(cols, lens, seed)[0]])
    w.setflags(write=False)
    return w
