"""The switch and frame-length builds of every kernel family (tools/parity_report.py: VARIANTS, LENGTHS, EXPECT) on the CPU:
which cases of tests/test_gpu_parity_variants.py are well-posed, the shape of the tables, the f32 port's centred frames, and
what the split metrics notice under a window and under the librosa switches.  No GPU.

Counting rule (a condition, not a measurement; the one of tests/test_parity_families_cpu.py per (family, variant)): a
(signal, kind, metric) case counts if the f32 port's own value against the f64 oracle is <= 1e-4.  For every row with a port,
col0_norm, rest_norm and band_norm count for `noise`, `tilted`, `quiet_1e-3`, `quiet_1e-5` and `silent_frames`, and col_norm
counts for at least three of them (a near-zero cepstral column divided by its own maximum: ss_mfcc_c256w with pre-emphasis on
the two quiet clips, 1.4e-4 and 1.5e-4; ss_mfcc_c2048 with window and pre-emphasis on `silent_frames`, 1.1e-4).  `dc`, `tone`
and `impulse` may fail to count: under a window their leakage is exact zero in f64 and rounding noise in f32, and ln makes the
comparison ill-posed.  The chirp-z rows have no port: they take the classes of which every case counts for the 128-point
generic family under the same switches, minus `dc`; their bar is 1e-4.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

import parity_report as pr  # noqa: E402

ROWS = pr.variant_rows()
CHIRPZ = [k for k in ROWS if pr.FAMILIES[k[0]]["tag"] == "chirpz"]
WITH_PORT = [k for k in ROWS if k not in CHIRPZ]
CENTRE_FAMILIES = ("mfcc_c256", "mfcc_c256w", "mfcc_c512", "mfcc_c1024", "front_generic")
ALWAYS_ON = ("col0_norm", "rest_norm", "band_norm")  # count for every always-counted class


def _id(key):
    return "/".join(key)


_PORT = {}


def _port(oracle, key):
    """The port's report for one row (and, for a chirp-z row, the generic family's under the same name), computed once."""
    if key not in _PORT:
        _PORT.update(pr.port_variants(oracle, {key: ROWS[key]}))
    return _PORT


@pytest.mark.parametrize("key", WITH_PORT, ids=_id)
def test_port_cases_count(oracle, key):
    fname, row = key[0], ROWS[key]
    rep = _port(oracle, key)[key]
    assert rep is not None and set(rep) == set(pr.family_signals(pr.variant_family(pr.FAMILIES[fname], row)))
    cnt = pr.counted(_PORT, fname, row)
    out = sorted(f"{s}.{k}.{m}={rep[s][k][m]:.2e}" for s in rep for k in rep[s] for m in pr.BAR_METRICS[k] if (s, k, m) not in cnt)
    worst = {(k, m): max(rep[s][k][m] for s, kk, mm in cnt if (kk, mm) == (k, m)) for k in pr.family_kinds(pr.FAMILIES[fname]) for m in pr.BAR_METRICS[k]}
    print(_id(key), "counted worst:", " ".join(f"{k}.{m}={v:.2e}" for (k, m), v in worst.items()), "| not counted:", " ".join(out) or "-")
    for s in pr.ALWAYS_COUNTED:
        for k in rep[s]:
            for m in pr.BAR_METRICS[k]:
                if m in ALWAYS_ON:
                    assert (s, k, m) in cnt, (key, s, k, m, rep[s][k][m])
    if "mfcc" in pr.family_kinds(pr.FAMILIES[fname]):
        miss = [s for s in pr.ALWAYS_COUNTED if (s, "mfcc", "col_norm") not in cnt]
        if miss:
            print(_id(key), "always-counted col_norm cases that do not count:", {s: f"{rep[s]['mfcc']['col_norm']:.2e}" for s in miss})
        assert len(pr.ALWAYS_COUNTED) - len(miss) >= 3, (key, miss)
    # the bars follow the counted cases
    bar = pr.bars(_PORT, fname, row)
    assert all(b == max(pr.TOL, 1.5 * worst[km]) for km, b in bar.items()), (key, bar, worst)


def test_known_col_norm_cases_that_do_not_count(oracle):
    """Over all rows, the always-counted cases that do not count are the three near-zero-column ones."""
    seen = set()
    for key in WITH_PORT:
        rep = _port(oracle, key)[key]
        seen |= {(key, s, k, m) for s in pr.ALWAYS_COUNTED for k in rep[s] for m in pr.BAR_METRICS[k] if not rep[s][k][m] <= pr.TOL}
    print(sorted(seen))
    assert seen == {(("mfcc_c256w", "pre"), "quiet_1e-3", "mfcc", "col_norm"), (("mfcc_c256w", "pre"), "quiet_1e-5", "mfcc", "col_norm"),
                    (("mfcc_c2048", "winpre"), "silent_frames", "mfcc", "col_norm")}


@pytest.mark.parametrize("key", CHIRPZ, ids=_id)
def test_chirpz_rows_take_the_generic_family_classes(oracle, key):
    fname, row = key[0], ROWS[key]
    rep = _port(oracle, key)
    assert rep[key] is None  # the port refuses fft_points that are not a power of two
    base = rep[("front_generic", key[1])]
    cnt = pr.counted(rep, fname, row)
    sigs = {s for s, _, _ in cnt}
    print(_id(key), sorted(sigs))
    bad = {s for s, kinds in base.items() for k in kinds for m in pr.BAR_METRICS[k] if not kinds[k][m] <= pr.TOL}
    assert "dc" not in sigs and set(pr.ALWAYS_COUNTED) <= sigs and sigs == set(base) - {"dc"} - bad
    assert cnt == {(s, k, m) for s in sigs for k in pr.family_kinds(pr.FAMILIES[fname]) for m in pr.BAR_METRICS[k]}
    assert set(pr.bars(rep, fname, row).values()) == {pr.TOL}


def test_table_shape():
    assert set(pr.EXPECT) == set(pr.FAMILIES)
    assert len(ROWS) == sum(len(t) for t in pr.EXPECT.values())  # (family, row name) is unique
    assert len(set(pr.VARIANTS)) == len(pr.VARIANTS) and not [v for v in pr.VARIANTS if "+" in v or v.startswith(("flen", "M"))]
    for (fname, vname), row in ROWS.items():
        fam = pr.FAMILIES[fname]
        assert set(row["kernels"]) == set(pr.family_kinds(fam)), (fname, vname)
        shape, _, sw = vname.partition("+")
        if shape in pr.VARIANTS:
            assert row["switches"] == pr.VARIANTS[shape] and row["flen"] is None and row["M"] is None
        else:
            over = {k: row[k] for k in ("flen", "M") if row[k] is not None}
            assert over in pr.LENGTHS[fname], (fname, vname)
            assert row["switches"] == (pr.VARIANTS[sw] if sw else {})
        okw, skw = pr.family_kwargs(fam, row)
        assert all(okw[k] == v for k, v in row["switches"].items()) and all(skw[k] == v for k, v in row["switches"].items())
        if row["flen"] is not None:
            assert okw["frame_length"] == row["flen"] / fam["sr"] and pr.family_samples(fam, row) == row["flen"] + 24 * fam["step"] + 3
        else:
            assert pr.family_samples(fam, row) == pr.family_samples(fam)  # centred rows keep the family's sample count
    for fname, fam in pr.FAMILIES.items():
        names = {v for f, v in ROWS if f == fname}
        if fam["path"] == "stft":
            assert names >= ({"slaney"} if fam["tag"] == "chirpz" else {"slaney", "htk", "band"}), fname
            continue
        if fname == "front_generic_chirpz":
            assert names >= {"win", "pre", "pow2", "slaney", "center_reflect"}
        # every length alone, and at least one of them with a window
        for over in pr.LENGTHS.get(fname, ()):
            assert "".join(f"{k}{v}" for k, v in over.items()) in names, (fname, over)
        assert not pr.LENGTHS.get(fname) or any("+win" in v for v in names), fname
        # every switch tag of the family's launcher is named by a row that stays on the family's kernel
        seen = set()
        for (f, v), row in ROWS.items():
            if f == fname:
                seen |= {t for prefix, tags in row["kernels"].values() if prefix in (fam["kernel"], fam["kernel"] + "<") for t in tags}
        assert set(pr.LAUNCHER_TAGS[fname]) <= seen, (fname, sorted(set(pr.LAUNCHER_TAGS[fname]) - seen))
    assert pr.reaches_variant(pr._k("ss_mfcc_c256<", "10,win"), "ss_mfcc_c256<10,exact,bank421,win>")
    assert not pr.reaches_variant(pr._k("ss_mfcc_c256<", "10,win"), "ss_mfcc_c256w<10,win>")
    assert not pr.reaches_variant(pr._k("ss_mfcc_c512", "mfe"), "ss_mfcc_c512") and pr.reaches_variant(pr._k("ss_mfcc_c512"), "ss_mfcc_c512")
    assert pr.kernel_tags("ss_mfcc_c1024<mfe,lib,pre>") == {"mfe", "lib", "pre"}


# ------------------------------------------------------------------------------------------------ centred frames in the port

@pytest.mark.parametrize("pad", ["reflect", "constant"])
@pytest.mark.parametrize("fname", CENTRE_FAMILIES)
def test_port_centred_frames(oracle, fname, pad):
    """The f32 port under framing = center against the f64 oracle: 1e-4 on every bar metric for the five always-counted
    classes, alone and under the `lib` switches.  The frames themselves are those of contract framing on
    np.pad(x, flen // 2, mode): the mfe features of both agree bit for bit over the frames they share."""
    fam = pr.FAMILIES[fname]
    for sw in (dict(framing="center", pad_mode=pad), dict(pr.VARIANTS["lib"], framing="center", pad_mode=pad)):
        row = dict(family=fname, name="centre", switches=sw, flen=None, M=None)
        rep = pr.port_families(oracle, {fname: fam}, variant=row)[fname]
        assert rep is not None
        for s in pr.ALWAYS_COUNTED:
            for k in rep[s]:
                for m in pr.BAR_METRICS[k]:
                    print(fname, pad, sorted(sw), s, k, f"{m}={rep[s][k][m]:.2e}")
                    assert rep[s][k][m] <= pr.TOL, (fname, pad, sw, s, k, m, rep[s][k][m])
    sig = pr.family_signals(fam)
    n, flen, hop = pr.family_samples(fam), fam["flen"], fam["step"]
    pc = oracle.make_params(**pr.family_kwargs(fam, dict(switches=dict(framing="center", pad_mode=pad)))[0])
    p0 = oracle.make_params(**pr.family_kwargs(fam)[0])
    assert oracle.num_frames(pc, n) == 1 + n // hop
    for s in ("noise", "tone"):
        f_c, e_c = oracle.port_mfe(pc, sig[s])
        assert f_c.shape == oracle.mfe(pc, sig[s])[0].shape == (1 + n // hop, fam["M"])
        f_p, e_p = oracle.port_mfe(p0, np.pad(sig[s], flen // 2, mode=pad))
        T = min(len(f_c), len(f_p))
        assert T >= 25 and np.array_equal(f_c[:T], f_p[:T]) and np.array_equal(e_c[:T], e_p[:T]), (fname, pad, s)
        assert not np.array_equal(f_c[0], oracle.port_mfe(p0, sig[s])[0][0])  # not the un-padded frames


def test_port_centred_frames_with_pre_emphasis(oracle):
    """Pre-emphasis runs over the clip before the padding, as in the oracle (its first sample takes the clip's last)."""
    fam = pr.FAMILIES["mfcc_c256"]
    x = pr.family_signals(fam)["noise"]
    pc = oracle.make_params(**pr.family_kwargs(fam, dict(switches=pr.VARIANTS["center_pre"]))[0])
    p0 = oracle.make_params(**pr.family_kwargs(fam)[0])
    y = (x - np.float32(0.97) * np.roll(x, 1)).astype(np.float32)
    f_c = oracle.port_mfe(pc, x)[0]
    f_p = oracle.port_mfe(p0, np.pad(y, fam["flen"] // 2, mode="reflect"))[0]
    assert np.array_equal(f_c[:len(f_p)], f_p[:len(f_c)])


def test_port_refuses_what_it_does_not_implement(oracle):
    fam = pr.FAMILIES["mfcc_c256"]
    x = pr.family_signals(fam)["noise"]
    for field, value in (("framing", 4), ("framing", -1)):
        p = oracle.make_params(**pr.family_kwargs(fam)[0])
        setattr(p, field, value)
        for call in (oracle.port_mfe, oracle.port_mfcc):
            with pytest.raises(oracle.OracleError) as e:
                call(p, x)
            assert e.value.code == oracle.ORC_ERR_BAD_CONFIG, (field, value)
    p = oracle.make_params(**pr.family_kwargs(fam, dict(switches=pr.VARIANTS["center_reflect"]))[0])
    p.pad_mode = 2
    with pytest.raises(oracle.OracleError) as e:
        oracle.port_mfe(p, x)
    assert e.value.code == oracle.ORC_ERR_BAD_CONFIG
    # every framing it takes agrees with the oracle on the frame count and on the features
    for framing in ("contract", "padded", "center"):
        q = oracle.make_params(**pr.family_kwargs(fam, dict(switches=dict(framing=framing)))[0])
        got, want = oracle.port_mfe(q, x)[0], oracle.mfe(q, x)[0]
        assert got.shape == want.shape and pr.block_metrics("mfe", got, want)["band_norm"] <= pr.TOL, framing


# --------------------------------------------------------------------------- what the split metrics notice under the switches

def test_band_norm_notices_a_wrong_slaney_band_under_lib(oracle):
    """`lib` (Hann window, power spectrum, area-normalised Slaney bank): `want` with one band 30 dB under the loudest 0.1 % off
    on the gliding tone passes the block metric and fails band_norm (mfe features are power here: 10 log10).  The band is the
    one nearest to 30 dB under the loudest: under the Hann window the leakage falls so steeply past the glide that this is the
    band at its edge, 24.7 dB under; the next one is 46 dB under, below band_norm's floor."""
    fam, row = pr.FAMILIES["mfcc_c256"], ROWS[("mfcc_c256", "lib")]
    want = pr.family_reference(oracle, fam, pr.family_signals(fam)["tone"][None], variant=row)["mfe"][0]
    peak = want.max(axis=0)
    db = 10.0 * np.log10(peak / peak.max())
    b = int(np.argmin(np.abs(db + 30.0)))
    assert -35.0 < db[b] < -24.0, db[b]
    got = want.copy()
    got[:, b] *= 1.001
    m = pr.block_metrics("mfe", got, want)
    assert m["max_norm"] <= 1e-4 < m["band_norm"], m
    assert m["band_norm"] == pytest.approx(1e-3, rel=1e-6)


def test_col_norm_notices_a_wrong_last_column_under_a_window(oracle):
    """`win`: `want` with the last cepstral column of the quiet clip 0.1 % off passes the block metric and fails col_norm."""
    fam, row = pr.FAMILIES["mfcc_c256"], ROWS[("mfcc_c256", "win")]
    want = pr.family_reference(oracle, fam, pr.family_signals(fam)["quiet_1e-5"][None], variant=row)["mfcc"][0]
    got = want.copy()
    got[:, -1] *= 1.001
    m = pr.metrics(got, want, True)
    assert m["max_norm"] <= 1e-4 < m["col_norm"], m
    assert m["col_norm"] == pytest.approx(1e-3, rel=1e-6)
