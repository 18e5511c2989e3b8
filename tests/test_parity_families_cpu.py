"""The bars of tests/test_gpu_parity_families.py are about the kernels, not about the inputs: for every kernel family of
tools/parity_report.py's FAMILIES that the oracle's f32 port accepts, and every signal class, the port -- the reference's own
operation order in f32 -- goes through the same metrics against the f64 oracle.  No GPU.

Counting rule (a condition, not a measurement): a (family, signal, metric) case counts if the port's own value is <= 1e-4;
per family at most one signal class may have a case that does not count, and `noise`, `tilted`, `quiet_1e-3`, `quiet_1e-5`
and `silent_frames` always count.  A case that does not count is ill-posed (exact zeros in f64 where f32 has rounding noise,
then ln): the GPU test leaves it out instead of failing a correct kernel on it.  The chirp-z families have no port (it
refuses fft_points that are not a power of two) and take the classes that count for the 128-point generic family, minus dc.

The last two tests show that col_norm / band_norm notice what the block metric lets through.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

import parity_report as pr  # noqa: E402

WITH_PORT = [n for n, f in pr.FAMILIES.items() if f["tag"] != "chirpz"]


@pytest.fixture(scope="module")
def port_rep(oracle):
    return pr.port_families(oracle)


def _not_counting(rep):
    return sorted({s for s, kinds in rep.items() for k in kinds for m in pr.BAR_METRICS[k] if not kinds[k][m] <= pr.TOL})


@pytest.mark.parametrize("name", WITH_PORT)
def test_port_cases_count(port_rep, name):
    rep = port_rep[name]
    assert rep is not None and set(rep) == set(pr.family_signals(pr.FAMILIES[name]))
    for s, kinds in rep.items():
        for k in kinds:
            print(name, s, k, " ".join(f"{m}={kinds[k][m]:.2e}{'' if kinds[k][m] <= pr.TOL else ' (does not count)'}" for m in pr.BAR_METRICS[k]),
                  f"max_norm={kinds[k]['max_norm']:.2e}" + (f" left_out={kinds[k]['band_left_out']:.2f}" if k != "mfcc" else ""))
    out = _not_counting(rep)
    assert len(out) <= 1, (name, out)
    assert not set(out) & set(pr.ALWAYS_COUNTED), (name, out)


@pytest.mark.parametrize("name", [n for n, f in pr.FAMILIES.items() if f["tag"] == "chirpz"])
def test_chirpz_families_take_the_generic_family_classes(port_rep, name):
    assert port_rep[name] is None  # the port refuses the configuration: no port number
    cnt = pr.counted(port_rep, name)
    sigs = {s for s, _, _ in cnt}
    print(name, sorted(sigs))
    assert "dc" not in sigs and set(pr.ALWAYS_COUNTED) <= sigs
    assert sigs == set(pr.family_signals(pr.FAMILIES[name])) - {"dc"} - set(_not_counting(port_rep["front_generic"]))
    assert cnt == {(s, k, m) for s in sigs for k in pr.family_kinds(pr.FAMILIES[name]) for m in pr.BAR_METRICS[k]}
    assert set(pr.bars(port_rep, name).values()) == {pr.TOL}


def test_family_table_and_signals():
    assert len(pr.FAMILIES) == 13
    for name, fam in pr.FAMILIES.items():
        sig = pr.family_signals(fam)
        n = pr.family_samples(fam)
        assert all(x.shape == (n,) and x.dtype == np.float32 for x in sig.values()), name
        # the tone glides from 1000 sqrt(2) Hz to twice that, under the Nyquist frequency: it rests on no bin centre
        t = np.arange(n)
        assert 2 * pr.TONE_HZ < fam["sr"] / 2
        assert np.array_equal(sig["tone"], (0.5 * np.sin(2 * np.pi * 1000.0 * np.sqrt(2.0) * (t + 0.5 * t * t / n) / fam["sr"])).astype(np.float32))
        assert np.flatnonzero(sig["impulse"])[1] == pr.family_hop(fam)
        # tilted noise: the power of the top tenth of the band is 30 .. 40 dB under the bottom tenth
        P = np.abs(np.fft.rfft(sig["tilted"].astype(np.float64))) ** 2
        q = len(P) // 10
        assert 30.0 <= 10 * np.log10(P[1:q].mean() / P[-q:].mean()) <= 40.0, name
    # signals() -- cfg1 / cfg3 / cfg5, the committed report and the strict test -- is as it was
    s = pr.signals(16000, 16000)
    assert list(s) == ["noise", "sine1k", "dc", "impulse", "quiet_1e-3", "quiet_1e-5", "silent_frames"]
    assert np.array_equal(np.flatnonzero(s["impulse"])[:3], [0, 160, 320])
    assert np.array_equal(s["sine1k"], (0.5 * np.sin(2 * np.pi * 1000.0 * np.arange(16000) / 16000)).astype(np.float32))


def test_col_norm_notices_a_wrong_last_column(oracle):
    """`want` with the last cepstral column 0.1 % off passes the block metric and fails col_norm (a quiet clip: column 0,
    ln of the frame energy, is then 50 times the last column)."""
    fam = pr.FAMILIES["mfcc_c256"]
    want = pr.family_reference(oracle, fam, pr.family_signals(fam)["quiet_1e-5"][None])["mfcc"][0]
    got = want.copy()
    got[:, -1] *= 1.001
    m = pr.metrics(got, want, True)
    assert m["max_norm"] <= 1e-4 < m["col_norm"], m
    assert m["col_norm"] == pytest.approx(1e-3, rel=1e-6)


@pytest.mark.parametrize("name,kind", [("mel_c256", "mel"), ("mfcc_c256", "mfe")])
def test_band_norm_notices_a_wrong_quiet_band(oracle, name, kind):
    """`want` with one band 30 dB under the maximum 0.1 % off passes the block metric and fails band_norm (the gliding tone:
    the bands it never reaches hold its leakage; mel spectrograms are power, mfe features amplitude)."""
    fam = pr.FAMILIES[name]
    want = pr.family_reference(oracle, fam, pr.family_signals(fam)["tone"][None])[kind][0]
    bands = want if kind == "mel" else want.T
    peak = bands.max(axis=1)
    db = (10.0 if kind == "mel" else 20.0) * np.log10(peak / peak.max())
    b = int(np.argmin(np.abs(db + 30.0)))
    assert -35.0 < db[b] < -25.0, db[b]
    got = bands.copy()
    got[b] *= 1.001
    m = pr.block_metrics(kind, got if kind == "mel" else got.T, want)
    assert m["max_norm"] <= 1e-4 < m["band_norm"], m
    # a band under the floor is left out, and the share is taken from `want`
    mute = np.where(np.arange(len(peak)) == b, 1e-6, 1.0)
    quiet = want * (mute[:, None] if kind == "mel" else mute[None, :])
    before, after = m["band_left_out"], pr.block_metrics(kind, quiet, quiet)["band_left_out"]
    assert after == pytest.approx(before + 1.0 / len(peak))
