"""What tests/test_noise_mix_cpu.py and tests/test_noise_mix.py share: the numpy restatement of the ss_noise_* section of
include/speechsauce_amd.h -- the draws (Philox4x32-10 of specaug_model in integers, the dB draws in f64), the f64 energies in the
normative order of additions, the gains in f64 and the mix with the exactly emulated fmaf of affine_model.
"""
import numpy as np

from affine_model import fmaf
from specaug_model import MASK32, philox

ROW = np.dtype([("noise_clip", np.int32), ("start", np.int32), ("snr_db", np.float32), ("gain_db", np.float32), ("speech_gain", np.float32),
                ("noise_gain", np.float32), ("speech_energy", np.float64), ("noise_energy", np.float64)])
DRAW_FIELDS = ("noise_clip", "start", "snr_db", "gain_db")
SNR_STREAM, GAIN_STREAM = 0x20000, 0x20001
CHUNK, LANES = 2048, 256
LIMIT = 1 << 31
# the worked pin of the header: seed 2026, epoch 0, clip_base 0, prob 0.5, SNR 10 .. 30 dB, gain -6 .. 6 dB, three speech clips of
# 16000 samples, noise clips of 8000, 1, 0, 50001 and 32000 samples
PIN_ARGS = dict(rng=(2026, 0), clip_base=0, so=[0, 16000, 32000, 48000], total=48000, no=[0, 8000, 8001, 8001, 58002, 90002], total_noise=90002,
                prob=0.5, snr=(10.0, 30.0), gain=(-6.0, 6.0))


def table(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


def good(lo, hi, total):
    return 0 <= lo <= hi <= total and hi - lo < LIMIT


def _db(lo, hi, u):
    lo, hi = np.float64(np.float32(lo)), np.float64(np.float32(hi))
    return np.float32(lo + (hi - lo) * (np.float64(u) * 2.0 ** -32))  # the product and the sum rounded once each, then once to f32


def draws_ref(rng, clip_base, so, total, no, total_noise, prob, snr, gain):
    """The draw fields of every clip's row; everything else 0."""
    seed, epoch = (int(v) & (2 ** 64 - 1) for v in rng)
    so, no = np.asarray(so, np.int64), np.asarray([0] if no is None else no, np.int64)
    n, n_noise = len(so) - 1, len(no) - 1
    plan = np.zeros(n, ROW)
    ids = (int(clip_base) + np.arange(n, dtype=np.int64)) & MASK32
    key, e = (seed & MASK32, seed >> 32), (epoch & MASK32, epoch >> 32)
    u = philox((ids, np.full(n, SNR_STREAM), e[0], e[1]), key) if n else [np.zeros(0, np.uint32)] * 4
    v = philox((ids, np.full(n, GAIN_STREAM), e[0], e[1]), key) if n else [np.zeros(0, np.uint32)] * 4
    bar = int(np.float64(np.float32(prob)) * 4294967296.0)
    for b in range(n):
        row = plan[b]
        row["snr_db"], row["gain_db"] = _db(snr[0], snr[1], int(u[3][b])), _db(gain[0], gain[1], int(v[0][b]))
        row["noise_clip"] = -1
        if not good(int(so[b]), int(so[b + 1]), total):
            row["noise_clip"] = -2
            continue
        if n_noise == 0 or not int(u[0][b]) < bar:
            continue
        c = (int(u[1][b]) * n_noise) >> 32
        lo, hi = int(no[c]), int(no[c + 1])
        if not (good(lo, hi, total_noise) and lo < hi):
            continue
        row["noise_clip"], row["start"] = c, (int(u[2][b]) * (hi - lo)) >> 32
    return plan


def energy(v):
    """sum of (double)v_i^2 in the normative order: chunks of 2048, 256 strided partials, the tree, the chunks in ascending order"""
    v = np.asarray(v, np.float32).astype(np.float64)
    if v.size == 0:
        return np.float64(0.0)
    chunks = -(-v.size // CHUNK)
    sq = np.zeros(chunks * CHUNK)
    sq[:v.size] = v * v  # exact; the zeros behind the clip's end add nothing to a non-negative sum
    sq = sq.reshape(chunks, CHUNK // LANES, LANES)
    p = sq[:, 0].copy()
    for j in range(1, CHUNK // LANES):
        p = p + sq[:, j]
    h = LANES // 2
    while h >= 1:
        p[:, :h] = p[:, :h] + p[:, h:2 * h]
        h //= 2
    return np.cumsum(p[:, 0])[-1]  # cumsum adds one by one


def noise_segment(nz, no, c, start, L):
    lo, N = int(no[c]), int(no[c + 1]) - int(no[c])
    return np.asarray(nz)[lo + (int(start) + np.arange(L, dtype=np.int64)) % N]


def gains(gain_db, snr_db, es, en, mixed):
    g = np.float64(1.0) if gain_db == 0 else np.float64(10.0) ** (np.float64(gain_db) / 20.0)
    ng = np.float32(0.0)
    if mixed and es > 0 and en > 0:
        ng = np.float32((g * np.sqrt(np.float64(es) / np.float64(en))) * np.float64(10.0) ** (-np.float64(snr_db) / 20.0))
    return np.float32(g), ng


def plan_ref(x, rng, clip_base, so, total, nz, no, total_noise, prob, snr, gain):
    """The whole plan: x and nz are the float32 samples (PCM already converted)."""
    plan = draws_ref(rng, clip_base, so, total, no, total_noise, prob, snr, gain)
    for b, row in enumerate(plan):
        if row["noise_clip"] == -2:
            continue
        lo, hi = int(so[b]), int(so[b + 1])
        mixed = row["noise_clip"] >= 0
        row["speech_energy"] = energy(x[lo:hi])
        row["noise_energy"] = energy(noise_segment(nz, no, row["noise_clip"], row["start"], hi - lo)) if mixed else 0.0
        row["speech_gain"], row["noise_gain"] = gains(row["gain_db"], row["snr_db"], row["speech_energy"], row["noise_energy"], mixed)
    return plan


def mix_ref(x, so, total, nz, no, total_noise, plan, out):
    """out[i] = fmaf(noise_gain, n_i, speech_gain * x_i) of every clip, into a copy of `out` (what the caller's block held)"""
    x, out = np.asarray(x, np.float32), np.array(out, np.float32)
    no = np.asarray([0] if no is None else no, np.int64)
    for b, row in enumerate(plan):
        lo, hi = int(so[b]), int(so[b + 1])
        if not good(lo, hi, total) or row["noise_clip"] == -2:
            continue
        s = row["speech_gain"] * x[lo:hi]  # rounded on its own
        c = int(row["noise_clip"])
        if row["noise_gain"] != 0 and 0 <= c < len(no) - 1 and good(int(no[c]), int(no[c + 1]), total_noise) and 0 <= row["start"] < no[c + 1] - no[c]:
            s = fmaf(np.full(hi - lo, row["noise_gain"], np.float32), noise_segment(nz, no, c, row["start"], hi - lo), s)
        out[lo:hi] = s
    return out


def adjacent_f32(a, b):
    """a == b or its neighbour, as f32 bit patterns of one sign (or both zero)"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    return (np.abs(ia - ib) <= 1) | ((a == 0) & (b == 0))


def speech(lens, seed=0, scale=0.1):
    """packed float32 clips of the given lengths"""
    return (np.random.default_rng(seed).standard_normal(int(np.sum(lens))) * scale).astype(np.float32)
