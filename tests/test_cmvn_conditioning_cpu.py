"""The reference side of tests/test_cmvn_conditioning.py, without a device: on the very blocks the GPU tests use (cmvn_model),

  * the two-pass references (the C oracle, oracle_np, `restate` of the stream test) are themselves good to far better than the
    RTOL the kernels are held to, per column: rounding their f64 output to f32 moves a column by at most 1e-6 of its maximum
    (measured: 9.4e-8), the C oracle and oracle_np agree to 1e-7 of a column's maximum (their sums differ only in order: 2^-53 * 1000
    per step against a column that varies by 2^-14), and |output| <= sqrt(n) holds with variance normalisation;
  * the inputs discriminate: the one-pass variance sum(x^2) / n - mean^2 of the parent commit, restated in the kernels' order with
    f64 sums, misses RTOL on the near-constant columns, and the form the kernels ship (squares about a value of the column) stays
    below 1e-6 on every kind of column.
"""
import numpy as np

import cmvn_model as M
from common import RTOL
from test_cmvn_stream_packed import TICKS, restate

F32_BOUND = 1e-6      # f32 rounding of the reference's value: 2^-24 = 6e-8 of the element, so of the column's maximum too
AGREE_BOUND = 1e-7    # two f64 two-pass evaluations of the same definition
KIND = {k: i for i, k in enumerate(M.KINDS)}


def _cmvn_cases():
    return [(rows, cols) for rows in M.CMVN_ROWS for cols in M.CMVN_COLS]


def _worst(a, b):
    return float(M.col_rel(a, b).max())


def test_hard_block_is_what_it_says():
    x = M.hard_block(301, 40, 5)
    assert x.dtype == np.float32 and x.shape == (301, 40) and not x.flags.writeable
    assert M.hard_block(301, 40, 5) is x
    up = np.nextafter(np.float32(1000), np.float32(2000))
    for base in (0, 32):  # the eight kinds again in the second 32-column tile
        one, alt, floor_, off, plain, tiny, big, const = (x[:, base + i].astype(np.float64) for i in range(8))
        assert (one == 1000).sum() == 300 and one[100] == up
        assert (alt[::2] == up).all() and (alt[1::2] == 1000).all()
        assert (floor_[5:9] == np.float32(-23.0258)).all() and (np.delete(floor_, range(5, 9)) == np.float32(np.log(1e-10))).all()
        assert abs(off.mean() - 1000) < 0.01 and 0.005 < off.std() < 0.02
        assert abs(plain.mean() - 1) < 1 and 2 < plain.std() < 4
        assert abs(tiny.mean()) < 1e-3 and 5e-4 < tiny.std() < 2e-3
        assert abs(big.mean() + 3e4) < 3e3 and 7e3 < big.std() < 1.3e4
        assert (const == 1.5).all()
    assert not np.array_equal(x[:, 4], x[:, 36])  # the second tile is not a copy of the first
    assert M.hard_block(2, 13, 0).shape == (2, 13) and M.hard_block(1, 13, 0)[0, 0] == up  # rows // 3 = 0


def test_col_rel_sees_a_small_column_beside_a_large_one():
    want = np.stack([np.linspace(-1e4, 1e4, 50), np.linspace(-1e-3, 1e-3, 50), np.zeros(50)], axis=1)
    got = want.copy()
    got[:, 1] *= 2.0  # the small column entirely wrong: invisible to an error taken over the block's maximum
    e = M.col_rel(got, want)
    assert np.abs(got - want).max() / np.abs(want).max() < 1e-6 and e[0] == 0 and e[1] == 1.0 and e[2] == 0
    got[3, 2] = 1e-30
    assert M.col_rel(got, want)[2] == np.inf  # an all-zero expected column is compared with ==
    bad = want.copy()
    bad[7, 0] = np.nan
    assert M.finite_rel(want, bad)[1] == 1  # finite on one side only
    e, n = M.finite_rel(bad, bad)
    assert e.max() == 0 and n == 0


def test_references_are_good_per_column_cmvn(oracle):
    import oracle_np

    worst = {"f32": 0.0, "np": 0.0, "out": 0.0}
    for rows, cols in _cmvn_cases():
        x = M.cmvn_block(rows, cols)
        for var in (False, True):
            want = oracle.cmvn(x, var)
            worst["f32"] = max(worst["f32"], _worst(want.astype(np.float32), want))
            worst["np"] = max(worst["np"], _worst(oracle_np.cmvn(x, var), want))
            if var:
                assert np.abs(want).max() <= np.sqrt(rows), (rows, cols)
                worst["out"] = max(worst["out"], float(np.abs(want).max()))
    for b, clip in enumerate(M.clips(M.PACKED_ROWS, 40, 2000)):
        if clip is not None:
            want = oracle.cmvn(clip, True)
            assert np.abs(want).max() <= np.sqrt(clip.shape[0]), b
            worst["f32"] = max(worst["f32"], _worst(want.astype(np.float32), want))
    print(f"cmvn: f32 rounding {worst['f32']:.3g}, oracle_np against the C oracle {worst['np']:.3g}, largest |want| {worst['out']:.4g}")
    assert worst["f32"] <= F32_BOUND and worst["np"] <= AGREE_BOUND


def test_references_are_good_per_column_cmvnw(oracle):
    import oracle_np

    worst = {"f32": 0.0, "np": 0.0, "out": 0.0}
    for cols in M.CMVN_COLS:
        for clip in M.clips(M.CMVNW_ROWS, cols, 4000):
            for win in M.CMVNW_WINS:
                for var in (False, True):
                    want = oracle.cmvnw(clip, win, var)
                    worst["f32"] = max(worst["f32"], _worst(want.astype(np.float32), want))
                    worst["np"] = max(worst["np"], _worst(oracle_np.cmvnw(clip, win, var), want))
                    if var:
                        worst["out"] = max(worst["out"], float(np.abs(want).max()))
    print(f"cmvnw: f32 rounding {worst['f32']:.3g}, oracle_np against the C oracle {worst['np']:.3g}, largest |want| {worst['out']:.4g}")
    assert worst["f32"] <= F32_BOUND and worst["np"] <= AGREE_BOUND and worst["out"] < M.CMVNW_ORACLE_BOUND


def test_references_are_good_per_column_stream():
    worst, top = 0.0, 0.0
    for x in M.streams(TICKS):
        for win in M.STREAM_WINS:
            for var in (False, True):
                want, n_t = restate(x, win, var)
                worst = max(worst, _worst(want.astype(np.float32), want))
                if var:
                    assert (np.abs(want) <= np.sqrt(n_t)[:, None]).all(), win
                    top = max(top, float(np.abs(want).max()))
    print(f"stream: f32 rounding {worst:.3g}, largest |want| {top:.4g}")
    assert worst <= F32_BOUND


def test_references_agree_where_a_column_holds_a_non_finite_value(oracle):
    """The C oracle and oracle_np are non-finite in the same places (the GPU tests take the C oracle's word for them)."""
    import oracle_np

    for bad in M.BAD_VALUES:
        with np.errstate(all="ignore"):
            x = M.poison(M.cmvn_block(98, 40), 37, bad)
            for var in (False, True):
                a, b = oracle.cmvn(x, var), oracle_np.cmvn(x, var)
                assert np.array_equal(np.isfinite(a), np.isfinite(b)) and not np.isfinite(a[:, [3, 35]]).any()
                assert np.isfinite(np.delete(a, [3, 35], axis=1)).all()
                for rows, win, row in ((98, 3, 37), (98, 31, 37), (400, 31, 205), (400, 301, 205)):
                    xw = M.poison(M.hard_block(rows, 40, 4100), row, bad)
                    a, b = oracle.cmvnw(xw, win, var), oracle_np.cmvnw(xw, win, var)
                    assert np.array_equal(np.isfinite(a), np.isfinite(b)), (bad, rows, win, var)
                    reach = (win - 1) // 2 * (2 if var else 1)  # the mean pass spreads it by pad rows, the variance pass by pad more
                    dead = ~np.isfinite(a[:, 3])
                    if rows == 400 and reach <= 150:  # the reach ends inside the clip: no reflection brings the value back
                        assert np.array_equal(np.flatnonzero(dead), np.arange(row - reach, row + reach + 1)), (bad, win, var)
                    if rows == 400 and reach == 300:
                        assert dead.all()
                    assert dead[row] and np.array_equal(dead, ~np.isfinite(a[:, 35]))


def test_one_pass_variance_fails_on_these_inputs_and_the_shifted_form_does_not(oracle):
    seen = {}
    for rows, cols in _cmvn_cases():
        x = M.cmvn_block(rows, cols)
        for var in (False, True):
            want = oracle.cmvn(x, var)
            old, new = M.col_rel(M.cmvn_one_pass(x, var), want), M.col_rel(M.cmvn_shifted(x, var), want)
            assert new.max() <= 1e-6, (rows, cols, var, new)
            if not var:
                assert np.array_equal(M.cmvn_one_pass(x, var), M.cmvn_shifted(x, var))  # the mean is formed the same way
                continue
            seen[rows, cols] = old
            for c in range(cols):
                kind = M.KINDS[c % 8]
                if kind in ("one_ulp_row", "log_floor") or (kind == "alternating_ulp" and rows >= 301):
                    assert old[c] > RTOL, (rows, cols, c, kind, old[c])
                if kind in ("plain", "tiny", "big", "const"):
                    assert old[c] <= 1e-6, (rows, cols, c, kind, old[c])  # well-conditioned columns never told the two apart
    for (rows, cols), old in seen.items():
        print(f"one-pass cmvn, rows {rows} cols {cols}: " + " ".join(f"{M.KINDS[c]}={old[c]:.2g}" for c in range(8)))


def test_one_pass_stream_variance_fails_on_these_inputs_and_the_shifted_form_does_not():
    for b, x in enumerate(M.streams(TICKS)):
        for win in M.STREAM_WINS:
            for var in (False, True):
                want, _ = restate(x, win, var)
                new = M.col_rel(M.stream_shifted(x, win, var), want)
                assert new.max() <= 1e-6, (b, win, var, new)
            if win > 2 and x.shape[0] > 31:
                old = M.col_rel(M.stream_one_pass(x, win, True), restate(x, win, True)[0])
                for c in (KIND["one_ulp_row"], 32 + KIND["one_ulp_row"]):
                    assert old[c] > RTOL, (b, win, c, old[c])
                print(f"one-pass stream {b} ({x.shape[0]} rows) win {win}: " + " ".join(f"{M.KINDS[c]}={old[c]:.2g}" for c in range(8)))
