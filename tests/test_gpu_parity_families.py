"""Every kernel family behind the dispatcher against the split-column / per-band metrics of tools/parity_report.py, and
the bit-exact batch invariants, on one small batch per family (FAMILIES there: 25 rows per clip and an odd tail; all signal
classes plus two all-zero clips as the clips of ONE batch call per output kind).  tests/test_gpu_parity_strict.py holds the
three BASELINE configurations to the same kind of bar through the single-clip call.

Parity.  For each case that counts (tests/test_parity_families_cpu.py: the f32 port's own value is <= 1e-4), col0_norm,
rest_norm and col_norm on MFCC, and band_norm on the mfe features and the mel spectrogram, are at most
max(1e-4, 1.5 x the port's worst value of that metric over the family's counted cases): the HIP path may not be worse than
the reference's own arithmetic.  Without a port (chirp-z) the bar is 1e-4.  The port values are computed here, at run time.

Invariants, bit for bit unless stated:
  * the same call twice gives equal results (no atomics on data, fixed reduction orders);
  * the batch with its clips permuted gives the permuted result, and each clip alone equals its row of the batch when both
    calls report the same kernel build -- otherwise (another build of the same kernel: the compiler's FMA fusion may differ
    in the last bit) within 1e-6 of the clip's maximum.  Every kernel but one gives a frame / row its own lanes, registers,
    exchange slot and P row, whatever shares its wave: units of the flat frame list (quads in ss_mfcc_c256 / ss_mfcc_c256w,
    frame pairs in ss_mfcc_c512 / ss_mfcc_c1024) may straddle two clips without one frame seeing the other.
    ss_mfcc_c256x2 is the exception: TWO frames ride one complex transform (z = a + i b), and its octs of 8 frames are cut
    from the flat frame list, so with 25 frames per clip a pair straddles the clip boundary wherever a clip starts at an odd
    flat frame; beyond that, one wave-wide vote per oct (pair guard, tiny-bin check) decides whether all its frames are
    transformed alone.  What the code guarantees there: rounding noise of ~3e-7 of the pair's largest bin, pairs more than
    30 dB apart and octs with a bin under 1e-4 of its pair's maximum run one frame per transform.  So the last bits of a
    clip depend on its neighbours and on where it sits; asserted for that kernel instead: the permuted batch and every clip
    alone meet the SAME parity bars against the oracle, and an oct that holds frames of one clip only does not see the
    others (clip 0, frames 0 .. 23, alone and in the batch: bit for bit);
  * mfe(4x) == 4 mfe(x) and mel_spectrogram(2x) == 4 mel_spectrogram(x) exactly (powers of two commute with every rounding;
    the votes of ss_mfcc_c256x2 compare ratios).  On the frame path an exact zero becomes f32::EPSILON (functions.rs:66-71)
    at either scale, so cells that hold EPSILON stay EPSILON;
  * all-zero clips inside the mixed batch: exactly f32::EPSILON in every mfe feature and energy, exact zeros on the STFT path.
"""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

import parity_report as pr  # noqa: E402

EPS = np.float32(1.1920929e-7)
ZEROS = (3, 9)  # where the all-zero clips sit in the batch of 10


@pytest.fixture(scope="module")
def port_rep(oracle):
    return pr.port_families(oracle)


def _batch(fam):
    sig = pr.family_signals(fam)
    X = np.zeros((len(sig) + len(ZEROS), pr.family_samples(fam)), np.float32)
    rows = [i for i in range(len(X)) if i not in ZEROS]
    X[rows] = np.stack(list(sig.values()))
    return list(sig), rows, X


def _mfe_kw(fam):
    return {k: v for k, v in pr.family_kwargs(fam)[1].items() if k != "num_cepstral"}


def _check_parity(name, port_rep, got, want, names, rows, what):
    cnt, bar = pr.counted(port_rep, name), pr.bars(port_rep, name)
    for kind in want:
        for i, s in enumerate(names):
            m = pr.block_metrics(kind, got[kind][rows[i]], want[kind][i])
            for met in pr.BAR_METRICS[kind]:
                if (s, kind, met) in cnt:
                    print(f"{name} {what} {s} {kind} {met}={m[met]:.2e} bar={bar[(kind, met)]:.2e}")
                    assert m[met] <= bar[(kind, met)], (name, what, s, kind, met, m, bar[(kind, met)])
            if kind != "mfcc":
                # the share of bands band_norm leaves out is what the f64 oracle's block alone dictates
                w = want[kind][i] if kind == "mel" else want[kind][i].T
                peak = np.abs(w).max(axis=1)
                assert m["band_left_out"] == pytest.approx(float(np.mean(peak < pr.BAND_FLOOR * peak.max())), abs=1e-12), (name, s, kind)


@pytest.mark.parametrize("name", list(pr.FAMILIES))
def test_family(ss, oracle, port_rep, name):
    fam = pr.FAMILIES[name]
    names, rows, X = _batch(fam)
    x2 = fam["kernel"] == "ss_mfcc_c256x2"
    want = pr.family_reference(oracle, fam, X[rows])
    cnt = pr.counted(port_rep, name)
    out = sorted({s for s in names for k in want for m in pr.BAR_METRICS[k] if (s, k, m) not in cnt})
    assert len(out) <= (2 if fam["tag"] == "chirpz" else 1) and not set(out) & set(pr.ALWAYS_COUNTED), (name, out)

    # ---- dispatch and parity ----
    got, kernels = pr.family_outputs(ss, fam, X)
    for kind, k in kernels.items():
        assert pr.reaches(fam, k), (name, kind, k)
    for kind in want:
        assert got[kind].shape[1:] == want[kind].shape[1:] and np.isfinite(got[kind]).all(), (name, kind)
    _check_parity(name, port_rep, got, want, names, rows, "batch")

    # ---- the same call twice ----
    again, kernels2 = pr.family_outputs(ss, fam, X)
    assert kernels2 == kernels
    for kind in got:
        assert np.array_equal(again[kind], got[kind]), (name, kind)

    # ---- clips permuted ----
    perm = np.random.default_rng(5).permutation(len(X))
    gp, kp = pr.family_outputs(ss, fam, np.ascontiguousarray(X[perm]))
    assert kp == kernels
    if x2:
        back = np.argsort(perm)  # row of the permuted batch that holds clip i
        _check_parity(name, port_rep, {k: v[back] for k, v in gp.items()}, want, names, rows, "permuted")
    else:
        for kind in got:
            assert np.array_equal(gp[kind], got[kind][perm]), (name, kind)

    # ---- each clip alone ----
    alone = {kind: [] for kind in got}
    for i in range(len(X)):
        g1, k1 = pr.family_outputs(ss, fam, X[i:i + 1])
        if i == 0:
            print(f"{name} one clip alone: {k1} (the batch: {kernels})")
        for kind in got:
            assert pr.reaches(fam, k1[kind]), (name, kind, k1)
            a, b = g1[kind][0], got[kind][i]
            alone[kind].append(a)
            if x2:
                if k1[kind] == kernels[kind] and i == 0:
                    assert np.array_equal(a[:24], b[:24]), (name, kind)  # octs 0 .. 2 hold frames of clip 0 only
            elif k1[kind] == kernels[kind]:
                assert np.array_equal(a, b), (name, kind, i)
            else:
                assert np.abs(a.astype(np.float64) - b).max() <= 1e-6 * np.abs(b).max(), (name, kind, i, k1[kind], kernels[kind])
    if x2:
        _check_parity(name, port_rep, {k: np.stack(v) for k, v in alone.items()}, want, names, rows, "alone")

    # ---- homogeneity under powers of two, all-zero clips ----
    if fam["path"] == "stft":
        g2 = np.asarray(ss.mel_spectrogram(2.0 * X, fam["sr"], **pr.family_kwargs(fam)[1]))
        assert ss._lib.lib().ss_last_kernel_name().decode() == kernels["mel"]
        assert np.array_equal(g2, 4.0 * got["mel"]), name
        for z in ZEROS:
            assert np.all(got["mel"][z] == 0.0), (name, z)
    else:
        f1, e1 = (np.asarray(a) for a in ss.mfe_batch(X, fam["sr"], **_mfe_kw(fam)))
        f4, e4 = (np.asarray(a) for a in ss.mfe_batch(4.0 * X, fam["sr"], **_mfe_kw(fam)))
        assert ss._lib.lib().ss_last_kernel_name().decode() == kernels["mfe"]
        assert np.array_equal(f1, got["mfe"])
        assert np.array_equal(f4, np.where(f1 == EPS, EPS, 4.0 * f1)), name
        assert np.array_equal(e4, np.where(e1 == EPS, EPS, 4.0 * e1)), name
        for z in ZEROS:
            assert np.all(f1[z] == EPS) and np.all(e1[z] == EPS), (name, z)
            # MFCC of an all-zero clip: ln(f32::EPSILON) in column 0, every frame the same
            c = got["mfcc"][z]
            assert np.array_equal(c, np.broadcast_to(c[0], c.shape)) and np.array_equal(c, got["mfcc"][ZEROS[0]])
            np.testing.assert_allclose(c[:, 0], np.log(np.float64(EPS)), rtol=0, atol=2e-5)
