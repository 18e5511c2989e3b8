"""The switch and frame-length builds of every kernel family (tools/parity_report.py: VARIANTS, LENGTHS, EXPECT -- window,
fused pre-emphasis, power spectrum, ortho DCT, Slaney / HTK banks, centred and padded frames, the other first-pass classes)
against the split-column / per-band metrics, on the batch of tests/test_gpu_parity_families.py: the eight signal classes plus
two all-zero clips as the clips of ONE batch call per output kind, 25 rows per clip and an odd tail.  tests/test_gpu_sweep.py
and tests/test_librosa_switches.py reach these builds too, with the block metric on white noise.

test_variant_parity, per (family, row):
  * dispatch: ss_last_kernel_name() of the MFCC and of the mfe call starts with the row's prefix and carries its tags (they
    are different builds; some rows leave their family: see EXPECT);
  * the output shape is the oracle's, everything is finite;
  * parity: on the cases that count (tests/test_parity_variants_cpu.py: the f32 port's own value is <= 1e-4), col0_norm,
    rest_norm and col_norm on MFCC and band_norm on mfe features / mel spectrograms are at most
    max(1e-4, 1.5 x the port's worst value of that metric over this row's counted cases), the port values computed here;
    1e-4 where there is no port (chirp-z).  band_left_out is the share the oracle block alone dictates.  On ss_mfcc_c256x2
    (two frames per complex transform: a clip's last bits depend on its neighbours, see tests/test_gpu_parity_families.py)
    the permuted batch meets the same bars.
test_variant_invariants, per (family, row), bit for bit:
  * the same call twice gives the same result; the permuted batch gives the permuted result (every kernel but ss_mfcc_c256x2);
  * the two all-zero clips are equal, their frames are the same wherever the oracle's are, and their mfe features and energies
    are f32::EPSILON where the oracle says so (exact zeros on the STFT path).

Eight rows miss a bar (OVER_THE_BAR: strict expected failures of the parity check alone, with the measured figures; DESIGN.md,
"Parity of the switch and frame-length builds").  Each miss was traced to its source on the device's output: none is a wrong
table, index or epilogue -- they are f32 rounding in a quantity the metric divides by something near zero, in signal classes
outside the always-counted five or in a band more than 90 dB under the loudest.  The rows keep their bars.
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
ROWS = pr.variant_rows()


class OverTheBar(AssertionError):
    """A counted case above its parity bar (and nothing else: dispatch, shape and the invariants assert plainly)."""


# (family, row) -> the measured miss, worst case first: metric = value (bar) on signal class; what it is made of
OVER_THE_BAR = {
    ("mfcc_c256x2", "pow2"): "mfcc col0_norm = 1.003e-4 (1e-4) on impulse: every frame has ln E = 0.0155 (E = 1.0156); the kernels take ln as "
                             "log2(E 2^32) ln 2 - 32 ln 2, exact to an ulp of 32 (absolute 2.6e-6): the error is 1.6e-6, the mfe bands agree to 1e-7",
    ("mfcc_c256", "win"): "mfe band_norm = 1.014e-4 (1e-4) on tone: band 38 peaks at 1.6e-4 of the block maximum (amplitude: 76 dB under), its "
                          "error is 1.6e-8 of the block maximum, a quarter ulp; the port has 5.1e-5 there",
    ("mfcc_c256w", "vorbis"): "mfe band_norm = 1.254e-4 (1e-4) on tone: band 75 peaks at 1.2e-4 of the block maximum, its error is 1.5e-8 of the "
                              "block maximum; the port has 5.7e-5 there",
    ("mfcc_c256w", "pre"): "mfcc col_norm = 1.888e-4 (1.085e-4) on noise: mel band 1 (one tap next to DC, behind the pre-emphasis zero) is 2e-5 of "
                           "the loudest band in frame 15 and 1.6e-3 off (3.6e-8 of the loudest band); ln carries that into every cepstral "
                           "column (4.8e-5 absolute); the port has 7.2e-5, and 1.4e-4 / 1.5e-4 on the quiet clips, which do not count",
    ("mfcc_c256w", "lib"): "mfcc col_norm = 2.466e-4 (1e-4) on impulse: all frames alike, ln mel lies between -10.3 and -9.3 in all 80 bands and "
                           "column 3 cancels to 0.024; its error is 5.9e-6 (the port's 1.5e-6), the mfe bands agree to 1e-7",
    ("mfcc_c256w", "center_lib"): "mfcc col_norm = 1.481e-4 (1.203e-4) on impulse: as under lib, column 4 cancels to 0.022, error 3.3e-6; the port has 8.0e-5",
    ("mfcc_c2048", "flen3000"): "mfcc col_norm = 1.325e-4 (1.061e-4) on impulse: column 16 cancels to 6.0e-3 beside a block maximum of 5.6, error "
                                "7.9e-7; the port has 7.1e-5",
    ("front_generic_chirpz", "pre"): "mfcc col_norm = 4.51e-4 (1e-4) on quiet_1e-3 (noise 1.98e-4, quiet_1e-5 2.51e-4): mel band 0 (the DC bin "
                                     "behind the pre-emphasis zero) is 1e-5 of the loudest band in frame 18 and 2.8e-3 off (3e-8 of the loudest "
                                     "band); ln carries that into the cepstra (1.2e-4 absolute)",
}
PARITY_PARAMS = [pytest.param(k, marks=pytest.mark.xfail(strict=True, raises=OverTheBar, reason=OVER_THE_BAR[k])) if k in OVER_THE_BAR else k for k in ROWS]


def _batch(fam, row):
    sig = pr.family_signals(pr.variant_family(fam, row))
    X = np.zeros((len(sig) + len(ZEROS), pr.family_samples(fam, row)), np.float32)
    rows = [i for i in range(len(X)) if i not in ZEROS]
    X[rows] = np.stack(list(sig.values()))
    return list(sig), rows, X


def _parity_misses(key, port_rep, got, want, names, rows, what):
    fname, row = key[0], ROWS[key]
    cnt, bar = pr.counted(port_rep, fname, row), pr.bars(port_rep, fname, row)
    misses = []
    for kind in want:
        for i, s in enumerate(names):
            m = pr.block_metrics(kind, got[kind][rows[i]], want[kind][i])
            for met in pr.BAR_METRICS[kind]:
                if (s, kind, met) in cnt:
                    over = not m[met] <= bar[(kind, met)]
                    print(f"{'/'.join(key)} {what} {s} {kind} {met}={m[met]:.3e} bar={bar[(kind, met)]:.3e}{' OVER THE BAR' if over else ''}")
                    if over:
                        misses.append((what, s, kind, met, m[met], bar[(kind, met)]))
            if kind != "mfcc":
                # the share of bands band_norm leaves out is what the f64 oracle's block alone dictates
                w = want[kind][i] if kind == "mel" else want[kind][i].T
                peak = np.abs(w).max(axis=1)
                assert m["band_left_out"] == pytest.approx(float(np.mean(peak < pr.BAND_FLOOR * peak.max())), abs=1e-12), (key, s, kind)
    return misses


@pytest.mark.parametrize("key", PARITY_PARAMS, ids="/".join)
def test_variant_parity(ss, oracle, key):
    fname, row = key[0], ROWS[key]
    fam = pr.FAMILIES[fname]
    names, rows, X = _batch(fam, row)
    want = pr.family_reference(oracle, fam, X[rows], variant=row)
    port_rep = pr.port_variants(oracle, {key: row})
    cnt = pr.counted(port_rep, fname, row)
    assert {(s, k, m) for s in pr.ALWAYS_COUNTED for k in want for m in pr.BAR_METRICS[k] if m != "col_norm"} <= cnt, key

    got, kernels = pr.family_outputs(ss, fam, X, row)
    print("/".join(key), kernels)
    for kind, k in kernels.items():
        assert pr.reaches_variant(row["kernels"][kind], k), (key, kind, k, row["kernels"][kind])
    for kind in want:
        assert got[kind].shape[1:] == want[kind].shape[1:] and np.isfinite(got[kind]).all(), (key, kind)
    misses = _parity_misses(key, port_rep, got, want, names, rows, "batch")

    x2 = {kind for kind, k in kernels.items() if k.startswith("ss_mfcc_c256x2")}
    if x2:
        perm = np.random.default_rng(5).permutation(len(X))
        gp, kp = pr.family_outputs(ss, fam, np.ascontiguousarray(X[perm]), row)
        assert kp == kernels
        back = np.argsort(perm)  # row of the permuted batch that holds clip i
        misses += _parity_misses(key, port_rep, {k: gp[k][back] for k in x2}, {k: want[k] for k in x2}, names, rows, "permuted")
    if misses:
        raise OverTheBar((key, misses))


@pytest.mark.parametrize("key", list(ROWS), ids="/".join)
def test_variant_invariants(ss, oracle, sslib, key):
    fname, row = key[0], ROWS[key]
    fam = pr.FAMILIES[fname]
    _, _, X = _batch(fam, row)
    got, kernels = pr.family_outputs(ss, fam, X, row)

    # ---- the same call twice ----
    again, kernels2 = pr.family_outputs(ss, fam, X, row)
    assert kernels2 == kernels
    for kind in got:
        assert np.array_equal(again[kind], got[kind]), (key, kind)

    # ---- clips permuted ----
    perm = np.random.default_rng(5).permutation(len(X))
    gp, kp = pr.family_outputs(ss, fam, np.ascontiguousarray(X[perm]), row)
    assert kp == kernels
    for kind in got:
        if not kernels[kind].startswith("ss_mfcc_c256x2"):
            assert np.array_equal(gp[kind], got[kind][perm]), (key, kind)

    # ---- all-zero clips: what the oracle says of them ----
    zero = pr.family_reference(oracle, fam, X[ZEROS[0]][None], variant=row)
    for kind in got:
        z, w = got[kind][ZEROS[0]], zero[kind][0]
        assert z.shape == w.shape and np.array_equal(z, got[kind][ZEROS[1]]), (key, kind)
        if kind == "mel":
            if np.all(w == 0.0):
                assert np.all(z == 0.0), key
            continue
        same = [t for t in range(len(w)) if np.array_equal(w[t], w[-1])]
        assert len(same) >= len(w) - 1, (key, kind)  # (without dc_elimination, frame 0 has the reference's own scale in column 0)
        for t in same:
            assert np.array_equal(z[t], z[-1]), (key, kind, t)
    if fam["path"] == "frame":
        wf, we = oracle.mfe(oracle.make_params(**pr.family_kwargs(fam, row)[0]), X[ZEROS[0]])
        f, e = (np.asarray(a) for a in ss.mfe_batch(X, fam["sr"], **{k: v for k, v in pr.family_kwargs(fam, row)[1].items() if k not in pr.MFE_DROPS}))
        assert sslib.ss_last_kernel_name().decode() == kernels["mfe"]
        assert np.array_equal(f, got["mfe"])
        assert np.all(wf == np.float64(EPS)) and np.all(we == np.float64(EPS)), key  # every variant's oracle says f32::EPSILON
        for zc in ZEROS:
            assert np.all(f[zc] == EPS) and np.all(e[zc] == EPS), (key, zc)
