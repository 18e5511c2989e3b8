"""Grouped CMVN without a device: the numpy restatement of tests/cmvn_group_model.py against the two-pass longdouble reference on
the case tests/test_cmvn_group.py runs on the GPU, the properties of the left fold, the Kaldi accumulator round trip, and through the
library everything it decides before it touches a device (ss_cmvn_stats_len, the two conversions, n_clips == 0, every SS_ERR_ARG
rule of the host-pointer forms with the first bad clip named)."""
import ctypes as C

import numpy as np
import pytest

import cmvn_group_model as G
import cmvn_model as M

SS_OK, SS_ERR_ARG = 0, 3
# The restatement against the reference: 2.5e-7 was measured when the fold was chosen (f32 rounding of the output is 6e-8 of an
# element; the rest is the f64 fold's error on the near-constant columns, relative to a spread 1e-5 .. 1e-7 of the offset)
MODEL_BOUND = 1e-6


@pytest.mark.parametrize("cols", M.CMVN_COLS)
def test_the_restatement_meets_the_two_pass_reference_on_the_case(cols):
    clip_list, block, off, groups = G.case(cols)
    stats = G.fold(block, off, groups, G.N_GROUPS)
    assert stats[3].tolist() == [0.0] * G.stats_len(cols) and stats[2, 0] == sum(G.case_rows()[len(M.PACKED_ROWS):])
    worst = 0.0
    for var in (False, True):
        got = G.apply(block, off, groups, stats, var, np.full(block.shape, -7.0, np.float32))
        for g in (0, 1, 2):
            rows, where = G.group_rows(clip_list, groups, g)
            want = G.two_pass(rows, var)
            for b, sl in where.items():
                err = M.col_rel(got[int(off[b]):int(off[b + 1])], want[sl]).max()
                worst = max(worst, err)
                assert err < MODEL_BOUND, (cols, var, g, b, err)
        lo, hi = int(off[G.LEFT_OUT]), int(off[G.LEFT_OUT + 1])
        assert (got[lo:hi] == -7.0).all()  # id -1: left out
    print(f"cols {cols}: restatement against the two-pass reference, worst col_rel {worst:.3g} (bound {MODEL_BOUND:g})")


@pytest.mark.parametrize("cols", M.CMVN_COLS)
@pytest.mark.parametrize("rows", M.CMVN_ROWS + (1, 2, 5, 2100))
def test_a_fresh_one_clip_group_is_cmvn_shifted_bit_for_bit(rows, cols):
    x = M.hard_block(rows, cols, 7100 + rows)
    row = G.merge(np.zeros(G.stats_len(cols)), *G.clip_stats(x))
    assert row[0] == rows
    for var in (False, True):
        with np.errstate(all="ignore"):
            want = M.cmvn_shifted(x, var)
        assert np.array_equal(G.apply_rows(x, row, var).view(np.uint32), want.view(np.uint32)), var


def test_the_left_fold_cut_at_every_position_is_the_uncut_fold():
    cols = 13
    clip_list, block, off, groups = G.case(cols)
    n = len(M.PACKED_ROWS) + 24
    off, groups = off[:n + 1], groups[:n]
    per_clip = [G.clip_stats(x) if x is not None else None for x in clip_list[:n]]
    whole = G.fold(block, off, groups, G.N_GROUPS, per_clip=per_clip)
    assert (whole[:3, 0] > 0).all()
    for cut in range(n + 1):
        first = np.array(groups)
        first[cut:] = -1  # the clips behind the cut are left out of the first call, those in front of it out of the second
        second = np.array(groups)
        second[:cut] = -1
        st = G.fold(block, off, first, G.N_GROUPS, per_clip=per_clip)
        st = G.fold(block, off, second, G.N_GROUPS, stats=st, per_clip=per_clip)
        assert np.array_equal(st.view(np.uint64), whole.view(np.uint64)), cut


def test_a_bad_count_word_is_a_fresh_group():
    x = M.hard_block(40, 13, 1)
    fresh = G.merge(np.zeros(27), *G.clip_stats(x))
    for bad in (np.nan, np.inf, -np.inf, -3.0, 0.5, 0.0):
        row = np.full(27, 123.0)
        row[0] = bad
        assert np.array_equal(G.merge(row, *G.clip_stats(x)).view(np.uint64), fresh.view(np.uint64)), bad


# ---------------------------------------------------------------- the Kaldi accumulator ------------------------------------------

def test_kaldi_round_trip_bounds():
    """to_kaldi then from_kaldi.  With integer-valued n, mean and var every product, sum and quotient is exact: the row comes back bit
    for bit.  Otherwise, with u = 2^-53 and every operation within (1 + u):
      mean' = fl(fl(n mean) / n): two roundings, |mean' - mean| <= (2u + u^2) |mean| < 3 ulp(mean);
      var'  = fl(fl(fl(n fl(var + fl(mean^2))) / n) - fl(mean'^2)): the quotient carries four roundings of var + mean^2, mean'^2 the
              error of mean' twice and one rounding, the difference one more: |var' - var| <= (4 + 5 + 1) u (var + mean^2), which is
              at most 10 ulp(var + mean^2) -- NOT of var: the accumulator form cancels, which is Kaldi's own conditioning."""
    rng = np.random.default_rng(5)
    cols = 40
    exact = np.concatenate([[64.0], rng.integers(-1000, 1000, cols), rng.integers(0, 1000, cols)]).astype(np.float64)
    assert np.array_equal(G.from_kaldi(G.to_kaldi(exact)).view(np.uint64), exact.view(np.uint64))
    k = G.to_kaldi(exact)
    assert k.shape == (2, cols + 1) and k[0, cols] == 64.0 and k[1, cols] == 0.0
    assert np.array_equal(k[0, :cols], 64.0 * exact[1:1 + cols]) and np.array_equal(k[1, :cols], 64.0 * (exact[1 + cols:] + exact[1:1 + cols] ** 2))
    x = M.hard_block(301, cols, 9)
    row = G.merge(np.zeros(G.stats_len(cols)), *G.clip_stats(x))
    back = G.from_kaldi(G.to_kaldi(row))
    mean, var = row[1:1 + cols], row[1 + cols:]
    assert back[0] == 301.0
    assert (np.abs(back[1:1 + cols] - mean) <= 3 * np.spacing(np.abs(mean))).all()
    assert (np.abs(back[1 + cols:] - var) <= 10 * np.spacing(var + mean * mean)).all()
    for bad in (0.0, 0.99, -2.0, np.nan, np.inf):  # a count below 1 (or not finite): a fresh row, both ways
        kk = np.array(k)
        kk[0, cols] = bad
        assert not G.from_kaldi(kk).any()
        rr = np.array(row)
        rr[0] = bad
        assert not G.to_kaldi(rr).any()


def test_the_library_converts_as_the_restatement(sslib):
    cols = 13
    n = C.c_size_t(0)
    assert sslib.ss_cmvn_stats_len(cols, C.byref(n)) == SS_OK and n.value == G.stats_len(cols) == 27
    assert sslib.ss_cmvn_stats_len(0, C.byref(n)) == SS_ERR_ARG and sslib.ss_cmvn_stats_len(cols, None) == SS_ERR_ARG
    assert sslib.ss_cmvn_stats_len(1 << 30, C.byref(n)) == SS_ERR_ARG
    x = M.hard_block(98, cols, 3)
    rows = [G.merge(np.zeros(27), *G.clip_stats(x)), np.zeros(27), np.concatenate([[np.nan], np.ones(26)])]
    for row in rows:
        k = np.full((2, cols + 1), 5.0)
        assert sslib.ss_cmvn_stats_to_kaldi(row.ctypes.data, cols, k.ctypes.data) == SS_OK
        assert np.array_equal(k.view(np.uint64), G.to_kaldi(row).view(np.uint64))
        back = np.full(27, 5.0)
        assert sslib.ss_cmvn_stats_from_kaldi(k.ctypes.data, cols, back.ctypes.data) == SS_OK
        assert np.array_equal(back.view(np.uint64), G.from_kaldi(k).view(np.uint64))
    k = np.zeros((2, cols + 1))
    assert sslib.ss_cmvn_stats_to_kaldi(None, cols, k.ctypes.data) == SS_ERR_ARG
    assert sslib.ss_cmvn_stats_to_kaldi(rows[0].ctypes.data, 0, k.ctypes.data) == SS_ERR_ARG
    assert sslib.ss_cmvn_stats_from_kaldi(k.ctypes.data, cols, None) == SS_ERR_ARG


def test_the_python_front_converts(sslib):
    import speechsauce_amd as ss

    x = M.hard_block(98, 13, 3)
    row = G.merge(np.zeros(27), *G.clip_stats(x))
    k = ss.cmvn_stats_to_kaldi(row)
    assert k.shape == (2, 14) and np.array_equal(k, G.to_kaldi(row))
    assert np.array_equal(ss.cmvn_stats_from_kaldi(k), G.from_kaldi(k))
    with pytest.raises(ValueError):
        ss.cmvn_stats_to_kaldi(np.zeros(26))


# ---------------------------------------------------------------- what the host forms decide before the device -------------------

class Call:
    """One valid set of host arguments (3 clips of 4 / 0 / 6 rows, 2 groups); each rule changes one of them."""

    def __init__(self, cols=5):
        self.cols, self.n, self.total, self.n_groups = cols, 3, 12, 2
        self.vec = np.ones((self.total, cols), np.float32)
        self.out = np.full((self.total, cols), -7.0, np.float32)
        self.off = np.array([0, 4, 4, 10], np.int64)
        self.grp = np.array([1, 0, -1], np.int32)
        self.stats = np.full((self.n_groups, 2 * cols + 1), 3.0)

    def run(self, lib, which, **kw):
        a = dict(vec=self.vec.ctypes.data, n=self.n, off=self.off.ctypes.data, total=self.total, cols=self.cols, grp=self.grp.ctypes.data,
                 n_groups=self.n_groups, stats=self.stats.ctypes.data, out=self.out.ctypes.data)
        a.update(kw)
        head = (a["vec"], a["n"], a["off"], a["total"], a["cols"], a["grp"], a["n_groups"])
        if which == "stats":
            return lib.ss_cmvn_stats_packed(*head, a["stats"])
        if which == "apply":
            return lib.ss_cmvn_apply_packed(*head, a["stats"], 1, a["out"])
        return lib.ss_cmvn_grouped_packed(*head, 1, a["out"])


FORMS = ("stats", "apply", "grouped")


@pytest.mark.parametrize("which", FORMS)
def test_host_forms_reject_before_the_device(sslib, which):
    c = Call()
    keep_stats, keep_out = c.stats.copy(), c.out.copy()

    def rejected(what, **kw):
        assert c.run(sslib, which, **kw) == SS_ERR_ARG, what
        return sslib.ss_last_error_string().decode()

    assert c.run(sslib, which, n=0) == SS_OK  # nothing to do: SS_OK, also without a device
    assert c.run(sslib, which, n=0, vec=None, off=None, stats=None, out=None) == SS_OK
    rejected("null vec", vec=None)
    rejected("null offsets", off=None)
    if which != "grouped":
        rejected("null stats", stats=None)
    if which != "stats":
        rejected("null out", out=None)
        assert "partially" in rejected("out overlaps vec partially", out=c.vec.ctypes.data + 4 * c.cols)
    assert "cols == 0" in rejected("cols == 0", cols=0)
    assert "n_groups" in rejected("n_groups == 0", n_groups=0)
    for name in ("total", "n", "n_groups"):
        assert "too large" in rejected(name + " = 2^31", **{name: 1 << 31})
    assert "too large" in rejected("cols = 2^30", cols=1 << 30)
    if which == "stats":
        assert "overlaps" in rejected("stats inside vec", stats=c.vec.ctypes.data)
    if which == "apply":
        assert "overlaps" in rejected("stats inside out", stats=c.out.ctypes.data)
    # the tables: the first bad clip is named
    first = np.array([1, 4, 4, 10], np.int64)
    assert "offsets[0] must be 0" in rejected("offsets[0] != 0", off=first.ctypes.data)
    rev = np.array([0, 4, 3, 10], np.int64)
    assert "decreasing offsets at clip 1" in rejected("a reversed pair", off=rev.ctypes.data)
    past = np.array([0, 4, 4, 13], np.int64)
    assert "clip 2 ends past total_rows" in rejected("a clip past total_rows", off=past.ctypes.data)
    for bad, at in ((np.array([1, 2, -1], np.int32), "clip 1: group 2 is outside the 2 groups"),
                    (np.array([1, 0, -2], np.int32), "clip 2: group -2 is outside the 2 groups")):
        assert at in rejected("a bad group id", grp=bad.ctypes.data)
    assert np.array_equal(c.stats, keep_stats) and np.array_equal(c.out, keep_out)  # nothing was written
