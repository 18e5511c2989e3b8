"""Grouped CMVN on the device (ss_cmvn_stats_packed* / ss_cmvn_apply_packed* / ss_cmvn_grouped_packed*) on the case of
tests/cmvn_group_model.py: the eight clips of cmvn_model.PACKED_ROWS (an empty one, one above kCmvnSplitRows) followed by 300 clips
of 1 .. 5 rows, all hard_blocks with their own seeds, in 5 groups -- two that interleave the long clips, one that holds all the short
clips, one without a clip, and id -1 on one clip.

Parity is cmvn_model.col_rel <= common.RTOL per clip against the two-pass longdouble reference on the group's concatenated rows
(every test prints its worst figure before it asserts).  Everything else is bit for bit, with no tolerance."""
import ctypes as C

import numpy as np
import pytest

import cmvn_group_model as G
import cmvn_model as M
from common import RTOL

pytestmark = pytest.mark.gpu
SENT = np.float32(-7777.0)
NAN_SENT = np.array([0x7FF8DEADBEEF0001], np.uint64).view(np.float64)[0]  # a NaN with a payload: a statistics sentinel


def _st(torch):
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _cuda(torch, a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _ptr(t):
    return None if t is None else t.data_ptr()


def _u32(t):
    return (t.cpu().numpy() if hasattr(t, "cpu") else np.ascontiguousarray(t)).view(np.uint32)


def _u64(t):
    return (t.cpu().numpy() if hasattr(t, "cpu") else np.ascontiguousarray(t)).view(np.uint64)


def stats_dev(torch, lib, x, off, grp, n_groups, stats, total=None, n=None, stream=None):
    rc = lib.ss_cmvn_stats_packed_device(x.data_ptr(), off.numel() - 1 if n is None else n, off.data_ptr(), x.shape[0] if total is None else total,
                                         x.shape[1], _ptr(grp), n_groups, stats.data_ptr(), _st(torch) if stream is None else stream)
    assert rc == 0, lib.ss_last_error_string()


def apply_dev(torch, lib, x, off, grp, n_groups, stats, var, out, total=None, n=None, stream=None):
    rc = lib.ss_cmvn_apply_packed_device(x.data_ptr(), off.numel() - 1 if n is None else n, off.data_ptr(), x.shape[0] if total is None else total,
                                         x.shape[1], _ptr(grp), n_groups, stats.data_ptr(), int(var), out.data_ptr(),
                                         _st(torch) if stream is None else stream)
    assert rc == 0, lib.ss_last_error_string()


def grouped_dev(torch, lib, x, off, grp, n_groups, var, out):
    rc = lib.ss_cmvn_grouped_packed_device(x.data_ptr(), off.numel() - 1, off.data_ptr(), x.shape[0], x.shape[1], _ptr(grp), n_groups, int(var),
                                           out.data_ptr(), _st(torch))
    assert rc == 0, lib.ss_last_error_string()


def run(torch, lib, block, off, groups, n_groups, var, stats=None):
    """stats on `stats` (zeros if None) then apply on a sentinel block -> (stats, out) as numpy"""
    x, doff, dgrp = _cuda(torch, block), _cuda(torch, off), _cuda(torch, groups)
    st = torch.zeros((n_groups, G.stats_len(block.shape[1])), dtype=torch.float64, device="cuda") if stats is None else _cuda(torch, stats)
    out = torch.full(block.shape, float(SENT), dtype=torch.float32, device="cuda")
    stats_dev(torch, lib, x, doff, dgrp, n_groups, st)
    apply_dev(torch, lib, x, doff, dgrp, n_groups, st, var, out)
    torch.cuda.synchronize()
    return st.cpu().numpy(), out.cpu().numpy()


@pytest.fixture(scope="module")
def cases():
    return {cols: G.case(cols) for cols in M.CMVN_COLS}


@pytest.fixture(scope="module")
def references(cases):
    """per cols, variance and group: the two-pass reference of the group's rows and where each member clip sits in it"""
    ref = {}
    for cols, (clip_list, _, _, groups) in cases.items():
        for g in (0, 1, 2):
            rows, where = G.group_rows(clip_list, groups, g)
            for var in (False, True):
                ref[cols, var, g] = (G.two_pass(rows, var), where)
    return ref


# ---------------------------------------------------------------- parity ---------------------------------------------------------

@pytest.mark.parametrize("cols", M.CMVN_COLS)
def test_parity_with_the_two_pass_reference(ss, sslib, cases, references, cols):
    import torch

    clip_list, block, off, groups = cases[cols]
    for var in (False, True):
        got = ss.cmvn_grouped_packed(torch.from_numpy(block).cuda(), torch.from_numpy(off).cuda(), torch.from_numpy(groups).cuda(), G.N_GROUPS,
                                     var).cpu().numpy()
        worst, bad = (0.0, None), []
        for g in (0, 1, 2):
            want, where = references[cols, var, g]
            for b, sl in where.items():
                err = float(M.col_rel(got[int(off[b]):int(off[b + 1])], want[sl]).max())
                worst = max(worst, (err, (g, b)))
                if not err <= RTOL:
                    bad.append((g, b, err))
        print(f"grouped cmvn cols {cols} var {var}: worst col_rel {worst[0]:.3g} at (group, clip) {worst[1]}")
        assert not bad, bad[:6]


@pytest.mark.parametrize("bad", M.BAD_VALUES, ids=["nan", "-inf", "inf"])
@pytest.mark.parametrize("cols", M.CMVN_COLS)
def test_a_poisoned_column_is_not_finite_in_its_group_only(sslib, cases, cols, bad):
    import torch

    clip_list, block, off, groups = cases[cols]
    victim = 5  # 1598 rows, group 1
    assert groups[victim] == 1
    dirty = np.array(block)
    dirty[int(off[victim]):int(off[victim + 1])] = M.poison(clip_list[victim], 700, bad)
    members = [b for b, x in enumerate(clip_list) if x is not None and groups[b] == 1]
    rows = np.concatenate([dirty[int(off[b]):int(off[b + 1])] for b in members])
    for var in (False, True):
        st_clean, clean = run(torch, sslib, block, off, groups, G.N_GROUPS, var)
        st, got = run(torch, sslib, dirty, off, groups, G.N_GROUPS, var)
        want, at = G.two_pass(rows, var), 0
        for b in members:
            lo, hi = int(off[b]), int(off[b + 1])
            err, odd = M.finite_rel(got[lo:hi], want[at:at + hi - lo])
            print(f"poison {bad} cols {cols} var {var} clip {b}: col_rel {err.max():.3g}, finite on one side only {odd}")
            assert odd == 0 and err.max() <= RTOL, (b, odd, err.max())
            at += hi - lo
        others = np.ones(block.shape[0], bool)
        for b in members:
            others[int(off[b]):int(off[b + 1])] = False
        assert np.array_equal(_u32(got[others]), _u32(clean[others]))  # the other groups keep their bits
        assert np.array_equal(_u64(st[[0, 2, 3]]), _u64(st_clean[[0, 2, 3]]))


# ---------------------------------------------------------------- bit for bit ----------------------------------------------------

@pytest.mark.parametrize("cols", M.CMVN_COLS)
def test_one_clip_groups_are_cmvn_packed(ss, sslib, cases, cols):
    import torch

    _, block, off, _ = cases[cols]
    n = len(off) - 1
    own = np.arange(n, dtype=np.int32)
    x, doff = torch.from_numpy(block).cuda(), torch.from_numpy(off).cuda()
    for var in (False, True):
        want = ss.cmvn_packed(x, doff, var)
        got = ss.cmvn_grouped_packed(x, doff, torch.from_numpy(own).cuda(), n, var)
        torch.cuda.synchronize()
        assert np.array_equal(_u32(got), _u32(want)), var


@pytest.mark.parametrize("cols", M.CMVN_COLS)
def test_rows_are_the_fold_and_apply_is_the_formula(ss, sslib, cases, cols):
    """The group rows equal the numpy fold of the per-clip rows that one-clip groups give; apply equals the numpy formula on the
    returned rows; a group without clips keeps a sentinel row; the combined call and the host forms give the same bits."""
    import torch

    _, block, off, groups = cases[cols]
    n, L = len(off) - 1, G.stats_len(cols)
    own, _ = run(torch, sslib, block, off, np.arange(n, dtype=np.int32), n, False)
    per_clip = [(int(own[b, 0]), own[b, 1:1 + cols], own[b, 1 + cols:]) for b in range(n)]
    assert [p[0] for p in per_clip] == [int(off[b + 1] - off[b]) for b in range(n)]
    prior = np.zeros((G.N_GROUPS, L))
    prior[3] = NAN_SENT  # no clip names group 3
    prior[3, 0] = 123.0
    want_st = G.fold(block, off, groups, G.N_GROUPS, stats=prior, per_clip=per_clip)
    for var in (False, True):
        st, out = run(torch, sslib, block, off, groups, G.N_GROUPS, var, stats=prior)
        assert np.array_equal(_u64(st), _u64(want_st))
        assert np.array_equal(_u64(st[3]), _u64(prior[3]))
        # group 3's row is a valid count with NaN statistics: no clip uses it.  The formula on the returned rows:
        want = G.apply(block, off, groups, st, var, np.full(block.shape, SENT, np.float32))
        assert np.array_equal(_u32(out), _u32(want)), var
        lo, hi = int(off[G.LEFT_OUT]), int(off[G.LEFT_OUT + 1])
        assert (out[lo:hi] == SENT).all()
        # the combined call is statistics on zeros plus apply
        st0, out0 = run(torch, sslib, block, off, groups, G.N_GROUPS, var)
        x, doff, dgrp = _cuda(torch, block), _cuda(torch, off), _cuda(torch, groups)
        both = torch.full(block.shape, float(SENT), dtype=torch.float32, device="cuda")
        grouped_dev(torch, sslib, x, doff, dgrp, G.N_GROUPS, var, both)
        torch.cuda.synchronize()
        assert np.array_equal(_u32(both), _u32(out0)), var
        # host forms
        h_st = ss.cmvn_stats_packed(block, off, groups, G.N_GROUPS)
        assert np.array_equal(_u64(h_st), _u64(st0))
        h_out = ss.cmvn_apply_packed(block, off, h_st, groups, var, out=np.full(block.shape, SENT, np.float32))
        assert np.array_equal(_u32(h_out), _u32(out0)), var
        keep = np.ones(block.shape[0], bool)
        keep[lo:hi] = False
        assert np.array_equal(_u32(ss.cmvn_grouped_packed(block, off, groups, G.N_GROUPS, var)[keep]), _u32(out0[keep])), var


def test_counts_that_are_not_whole_numbers_fold_the_same_way(sslib, cases):
    """A prior row whose count was written by hand -- not a whole number, or past 2^52 where f64 no longer holds every integer --
    is folded with the same serial sums as any other (the kernel forms whole-numbered counts another way)."""
    import torch

    cols = 13
    _, block, off, groups = cases[cols]
    n = len(off) - 1
    own, _ = run(torch, sslib, block, off, np.arange(n, dtype=np.int32), n, False)
    per_clip = [(int(own[b, 0]), own[b, 1:1 + cols], own[b, 1 + cols:]) for b in range(n)]
    prior = np.random.default_rng(6).standard_normal((G.N_GROUPS, G.stats_len(cols)))
    prior[:, 1 + cols:] **= 2
    prior[:, 0] = [2.5, 2.0 ** 53 + 2.0, 1e300, 7.0, 1.25]
    st, _ = run(torch, sslib, block, off, groups, G.N_GROUPS, False, stats=prior)
    assert np.array_equal(_u64(st), _u64(G.fold(block, off, groups, G.N_GROUPS, stats=prior, per_clip=per_clip)))
    assert st[0, 0] != prior[0, 0] and np.array_equal(_u64(st[3]), _u64(prior[3]))


def test_a_split_of_the_clips_is_one_call(sslib, cases):
    import torch

    cols = 40
    _, block, off, groups = cases[cols]
    whole, _ = run(torch, sslib, block, off, groups, G.N_GROUPS, False)
    n = len(off) - 1
    for cut in (1, 5, 6, 100, n - 1):
        r = int(off[cut])
        st, _ = run(torch, sslib, block[:r], off[:cut + 1], groups[:cut], G.N_GROUPS, False)
        st, _ = run(torch, sslib, block[r:], off[cut:] - r, groups[cut:], G.N_GROUPS, False, stats=st)
        assert np.array_equal(_u64(st), _u64(whole)), cut


def test_other_groups_clips_do_not_matter(sslib, cases):
    """Group 0's row and its clips' outputs keep their bits when the other groups' clips are permuted, removed or inserted and the block
    is laid out anew, as long as group 0's own clips keep their order."""
    import torch

    cols = 13
    clip_list, block, off, groups = cases[cols]
    st, out = run(torch, sslib, block, off, groups, G.N_GROUPS, True)
    mine = [b for b in range(len(groups)) if groups[b] == 0 and clip_list[b] is not None]
    rng = np.random.default_rng(3)
    for trial in range(3):
        others = [b for b in range(len(groups)) if groups[b] != 0]
        others = [others[i] for i in rng.permutation(len(others))][:len(others) - 60 * trial]  # permuted; then some removed
        order, gi = [], 0
        slots = sorted(rng.choice(len(others) + 1, len(mine)))  # where group 0's clips go, in their own order
        for k in range(len(others) + 1):
            while gi < len(mine) and slots[gi] == k:
                order.append(mine[gi])
                gi += 1
            if k < len(others):
                order.append(others[k])
        extra = [M.hard_block(17, cols, 900 + trial)] * trial  # inserted clips of group 4
        new_list = [clip_list[b] for b in order] + extra
        new_groups = np.array([groups[b] for b in order] + [4] * len(extra), np.int32)
        new_block, new_off = M.pack(new_list, cols)
        st2, out2 = run(torch, sslib, new_block, new_off, new_groups, G.N_GROUPS, True)
        assert np.array_equal(_u64(st2[0]), _u64(st[0])), trial
        for b in mine:
            k = order.index(b)
            assert np.array_equal(_u32(out2[int(new_off[k]):int(new_off[k + 1])]), _u32(out[int(off[b]):int(off[b + 1])])), (trial, b)


def test_null_table_is_group_zero_and_in_place_is_out_of_place(ss, sslib, cases):
    import torch

    cols = 40
    _, block, off, _ = cases[cols]
    zeros = np.zeros(len(off) - 1, np.int32)
    st0, out0 = run(torch, sslib, block, off, zeros, 1, True)
    st1, out1 = run(torch, sslib, block, off, None, 1, True)
    assert np.array_equal(_u64(st0), _u64(st1)) and np.array_equal(_u32(out0), _u32(out1))
    assert st0[0, 0] == block.shape[0]
    x, doff = _cuda(torch, block), _cuda(torch, off)
    st = _cuda(torch, st0)
    apply_dev(torch, sslib, x, doff, None, 1, st, True, x)  # out == vec
    torch.cuda.synchronize()
    assert np.array_equal(_u32(x), _u32(out0))
    front = ss.cmvn_apply_packed(_cuda(torch, block), doff, st[0], None, True)  # one row, no table: global CMVN
    assert np.array_equal(_u32(front), _u32(out0))


# ---------------------------------------------------------------- containment ----------------------------------------------------

@pytest.mark.parametrize("cols", M.CMVN_COLS)
def test_containment(sslib, cases, cols):
    """Bad tables and bad rows: a pair that ends past total_rows and a reversed pair (the table's last two, so that the clips in front
    of them are still found), group ids -1 and n_groups, and statistics rows with n = 0, NaN and -3 under apply.  The affected clips'
    rows keep the sentinel, every other clip has its clean bits, and the guard rows around out, the statistics and the block are
    untouched."""
    import torch

    clip_list, block, off, groups = cases[cols]
    n, R, L = len(off) - 1, block.shape[0], G.stats_len(cols)
    GUARD, NG = 64, G.N_GROUPS + 3  # groups 5, 6, 7: their rows get n = 0, NaN, -3 in front of apply
    keep = n - 3                    # the last three short clips give way to a pair that ends past total_rows and a reversed pair
    Rk = int(off[keep])
    bad_off = np.concatenate([off[:keep + 1], [R + 5, R - 4]]).astype(np.int64)
    bad_grp = np.concatenate([groups[:keep], [2, 2]]).astype(np.int32)
    bad_grp[10], bad_grp[11], bad_grp[12], bad_grp[13] = NG, 5, 6, 7
    assert Rk < R - 2 and len(bad_off) == keep + 3
    big_x = torch.full((R + 2 * GUARD, cols), 1e30, dtype=torch.float32, device="cuda")
    big_x[GUARD:GUARD + R] = torch.from_numpy(block)
    x = big_x[GUARD:GUARD + R]
    doff, dgrp = _cuda(torch, bad_off), _cuda(torch, bad_grp)
    big_st = torch.full((NG + 2, L), float(NAN_SENT), dtype=torch.float64, device="cuda")
    big_st.view(torch.int64)[:] = int(np.array([NAN_SENT]).view(np.int64)[0])
    big_st[1:1 + NG] = 0
    st = big_st[1:1 + NG]
    stats_dev(torch, sslib, x, doff, dgrp, NG, st)
    torch.cuda.synchronize()
    own, _ = run(torch, sslib, block, off, np.arange(n, dtype=np.int32), n, False)
    per_clip = [(int(own[b, 0]), own[b, 1:1 + cols], own[b, 1 + cols:]) for b in range(keep)] + [None, None]
    want_st = G.fold(block, bad_off, bad_grp, NG, per_clip=per_clip)
    assert np.array_equal(_u64(st), _u64(want_st))
    assert want_st[5, 0] > 0 and want_st[6, 0] > 0 and want_st[7, 0] > 0
    guard_bits = int(np.array([NAN_SENT]).view(np.int64)[0])
    assert (big_st.view(torch.int64)[0] == guard_bits).all() and (big_st.view(torch.int64)[-1] == guard_bits).all()
    st[5, 0], st[6, 0], st[7, 0] = 0.0, float("nan"), -3.0
    torch.cuda.synchronize()
    for var in (False, True):
        big_out = torch.full((R + 2 * GUARD, cols), float(SENT), dtype=torch.float32, device="cuda")
        out = big_out[GUARD:GUARD + R]
        apply_dev(torch, sslib, x, doff, dgrp, NG, st, var, out)
        torch.cuda.synchronize()
        want = G.apply(block, bad_off, bad_grp, st.cpu().numpy(), var, np.full(block.shape, SENT, np.float32))
        got = out.cpu().numpy()
        assert np.array_equal(_u32(got), _u32(want)), var
        for b in (10, 11, 12, 13, G.LEFT_OUT):
            assert (got[int(off[b]):int(off[b + 1])] == SENT).all(), b
        assert (got[Rk:] == SENT).all() and (got[:Rk] != SENT).sum() > (Rk - 100) * cols
        assert (big_out[:GUARD] == SENT).all() and (big_out[GUARD + R:] == SENT).all()
    assert (big_x[:GUARD] == 1e30).all() and (big_x[GUARD + R:] == 1e30).all() and np.array_equal(_u32(x), _u32(block))
    assert (big_st.view(torch.int64)[0] == guard_bits).all() and (big_st.view(torch.int64)[-1] == guard_bits).all()


# ---------------------------------------------------------------- graphs ---------------------------------------------------------

def _warm(torch, fn):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn(C.c_void_p(side.cuda_stream))
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()


def test_graph_replay_over_changed_tables_equals_eager_calls(sslib):
    """Statistics plus apply captured once behind a warm-up call of the same sizes, then replayed after the device tables and the rows
    were changed: the bits of the eager calls, whatever the memory pool holds from the tests in front of this one (inside a capture
    the scratch rows come from the library's capture block, not from an allocation node)."""
    import torch

    cols, n, NG, CAP = 13, 12, 4, 2600
    x = torch.zeros((CAP, cols), device="cuda")
    d_off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    d_grp = torch.zeros(n, dtype=torch.int32, device="cuda")
    st_g = torch.zeros((NG, G.stats_len(cols)), dtype=torch.float64, device="cuda")
    out_g = torch.full((CAP, cols), float(SENT), device="cuda")
    st_e, out_e = st_g.clone(), out_g.clone()

    def chain(st, out, stream=None):
        stats_dev(torch, sslib, x, d_off, d_grp, NG, st, stream=stream)
        apply_dev(torch, sslib, x, d_off, d_grp, NG, st, True, out, stream=stream)

    _warm(torch, lambda s: chain(st_g.clone(), out_g.clone(), s))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        chain(st_g, out_g)
    rng = np.random.default_rng(12)
    for k, lens in enumerate(([98, 0, 1, 2, 301, 5, 2100, 3, 4, 40, 7, 9], [5, 700, 0, 0, 31, 64, 1, 1, 1, 200, 33, 2], [1] * 12)):
        clip_list = M.clips(lens, cols, 8000 + 100 * k)
        block, off = M.pack(clip_list, cols)
        grp = rng.integers(-1, NG, n).astype(np.int32)
        x[:block.shape[0]] = torch.from_numpy(block)
        d_off.copy_(torch.from_numpy(off))
        d_grp.copy_(torch.from_numpy(grp))
        for t in (st_g, st_e):
            t.zero_()
        for t in (out_g, out_e):
            t.fill_(float(SENT))
        chain(st_e, out_e)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(st_g.view(torch.int64), st_e.view(torch.int64)) and torch.equal(out_g.view(torch.int32), out_e.view(torch.int32)), k
        want = G.apply(block, off, grp, st_e.cpu().numpy(), True, np.full(block.shape, SENT, np.float32))
        assert np.array_equal(_u32(out_g[:block.shape[0]]), _u32(want)) and (out_g[block.shape[0]:] == SENT).all(), k


def test_online_global_cmvn_behind_a_pool_tick_in_one_graph(ss, sslib):
    """ss_kstream_fbank_packed_device followed by ss_cmvn_apply_packed_device on the tick's row_offsets (no group table: global CMVN
    with stored statistics), captured once and replayed over changing tables: the rows equal apply on the eager tick's rows."""
    import torch

    from test_kaldi_stream import FBANK, FILL, HOPS, HOPS_13, KINDS, POOL, SLOTS, Rig, gpu_case_signal

    rig = Rig(ss, sslib, False, **FBANK)
    N, CAP, sh, cols = len(HOPS), 16, 160, rig.cols
    assert (POOL, N) == (16, 9)
    x = torch.zeros(CAP * sh, device="cuda")
    d_so, d_ro = torch.zeros(N + 1, dtype=torch.int64, device="cuda"), torch.zeros(N + 1, dtype=torch.int64, device="cuda")
    d_sl = torch.arange(N, dtype=torch.int32, device="cuda")
    out, en = rig.outs(torch, CAP)
    norm = torch.full((CAP, cols), FILL, device="cuda")
    pool_g = torch.zeros((POOL, rig.S), device="cuda")
    pool_e = pool_g.clone()
    stored = np.zeros(G.stats_len(cols))  # a stored global row: 5000 rows seen, means around -8, variances around 4
    rng = np.random.default_rng(4)
    stored[0], stored[1:1 + cols], stored[1 + cols:] = 5000.0, -8.0 + rng.standard_normal(cols), 4.0 + rng.random(cols)
    d_stats = torch.from_numpy(stored).cuda()

    def tick(pool, stream=None):
        assert rig.raw(torch, x, d_so, d_ro, CAP, d_sl, POOL, pool, out, en, stream=None if stream is None else stream.value) == 0
        apply_dev(torch, sslib, out, d_ro, None, 1, d_stats, True, norm, total=CAP, n=N, stream=stream)

    _warm(torch, lambda s: tick(pool_g.clone(), s))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        tick(pool_g)
    for k, hops in enumerate((HOPS, HOPS_13, [3, 0, 0, 2, 1, 4, 0, 0, 5])):
        slots = rng.permutation(POOL)[:N].astype(np.int32) if k else np.asarray(SLOTS, np.int32)
        so = np.concatenate([[0], np.cumsum(np.asarray(hops) * sh)]).astype(np.int64)
        ro = so // sh
        xs = torch.from_numpy(gpu_case_signal(70 + k, int(so[-1]), KINDS[k])).cuda()
        rows, _, _ = rig.call(torch, [xs[int(so[i]):int(so[i + 1])] for i in range(N)], slots.tolist(), pool_e)
        R = int(ro[-1])
        want = torch.full((R, cols), FILL, device="cuda")
        rows = rows.contiguous()
        apply_dev(torch, sslib, rows, _cuda(torch, ro), None, 1, d_stats, True, want)
        x[:xs.numel()] = xs
        d_so.copy_(torch.from_numpy(so))
        d_ro.copy_(torch.from_numpy(ro))
        d_sl.copy_(torch.from_numpy(slots))
        out.fill_(FILL)
        norm.fill_(FILL)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(norm[:R].view(torch.int32), want.view(torch.int32)) and (norm[R:] == FILL).all(), k
        assert np.array_equal(_u32(want), _u32(G.apply_rows(rows.cpu().numpy(), stored, True))), k
        assert torch.equal(pool_g, pool_e), k


def test_a_captured_statistics_call_needs_its_scratch_set_aside(sslib):
    """Inside a stream capture the statistics call takes its scratch from the capture block that the calls outside a capture size.  A
    captured call larger than anything run before it fails with SS_ERR_HIP, says what to do, and puts nothing on the stream."""
    import torch

    with open("/proc/self/maps") as f:
        paths = {line.split()[-1] for line in f if "libamdhip64" in line}
    hip = C.CDLL(sorted(paths)[0])
    cols, n = 4096, 1 << 20  # 64 GiB of per-clip rows: never set aside
    x = torch.zeros((1, cols), device="cuda")
    off = torch.zeros(2, dtype=torch.int64, device="cuda")
    st = torch.zeros((1, G.stats_len(cols)), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    raw, graph = torch.cuda.Stream(), C.c_void_p()
    assert hip.hipStreamBeginCapture(C.c_void_p(raw.cuda_stream), 2) == 0  # hipStreamCaptureModeRelaxed
    try:
        rc = sslib.ss_cmvn_stats_packed_device(x.data_ptr(), n, off.data_ptr(), 1, cols, None, 1, st.data_ptr(), C.c_void_p(raw.cuda_stream))
        msg = sslib.ss_last_error_string().decode()
    finally:
        assert hip.hipStreamEndCapture(C.c_void_p(raw.cuda_stream), C.byref(graph)) == 0
    n_nodes = C.c_size_t(99)
    hip.hipGraphGetNodes.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_size_t)]
    assert hip.hipGraphGetNodes(graph, None, C.byref(n_nodes)) == 0 and n_nodes.value == 0
    assert hip.hipGraphDestroy(graph) == 0
    assert rc == 4 and "outside the capture" in msg, (rc, msg)
