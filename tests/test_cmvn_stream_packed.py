"""Causal sliding-window CMVN over a pool of stream states: ss_cmvn_stream_state_len, ss_cmvn_stream_packed (host pointers), its
*_device form and the Python front's CmvnStreamPool.

Entry i of a call owns rows ro[i] .. ro[i+1] of the [total_rows x cols] blocks and pool row slots[i]: the last win - 1 raw rows of
its stream and their count.  Row t of a stream is normalised over rows max(t - win + 1, 0) .. t of that stream.  The reference
crate has no causal variant, so the yardstick is `restate` below: a float64 numpy restatement of the definition in
include/speechsauce_amd.h (two passes: the window mean, then the population deviation about it).  An f32-rounded one-pass f64
evaluation in the kernel's order differs from it by at most 5.3e-8 of the block maximum (standard_normal * 3 + 1 blocks, seeds
102 / 105 / 111, cols 13 / 40 / 80, win 1 / 2 / 4 / 31 / 301, both modes), so RTOL = 1e-4 has four orders of margin; the bitwise
tests are the sharp ones.
"""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

from common import RTOL, rel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ss_cmvn_stream_state_len", "ss_cmvn_stream_packed_device", "ss_cmvn_stream_packed")
EPS = 2.0 ** -30
COLS = (13, 40, 80)          # under, over and well over one 32-column tile
WINS = (1, 2, 4, 31, 301)
SEEDS = {13: 102, 40: 105, 80: 111}
POOL = 7
SLOTS = [3, 0, 6, 1, 5, 2, 4]  # stream b lives in pool row SLOTS[b]: a non-identity permutation
# rows per stream and tick: 400 > 301 slides a window fully inside one call, 0 is an untouched entry, every stream meets
# different counts, and from the second tick on the history comes from the state
TICKS = [[0, 1, 2, 5, 0, 37, 400], [5, 0, 400, 1, 37, 2, 0], [37, 5, 1, 0, 400, 0, 2]]
CONST_COL = 2  # this column of every stream is constant: exact zeros out


def restate(x, win, variance):
    """The definition, in float64: x [T, cols] the rows of ONE stream since its reset -> (out [T, cols], n_t [T])."""
    x = np.asarray(x, dtype=np.float64)
    T = x.shape[0]
    out = np.empty_like(x)
    n_t = np.minimum(np.arange(T) + 1, win)
    for t in range(T):
        W = x[t - n_t[t] + 1:t + 1]
        mean = W.sum(axis=0) / n_t[t]
        out[t] = x[t] - mean
        if variance:
            std = np.sqrt(np.maximum(((W - mean) ** 2).sum(axis=0) / n_t[t], 0.0))
            out[t] /= std + EPS
    return out, n_t


@functools.lru_cache(maxsize=None)
def _streams(cols, n_streams=POOL, T=450):
    """Seeded raw rows [n_streams, T, cols], float32, one constant column; never modified."""
    rng = np.random.default_rng(SEEDS[cols])
    x = (rng.standard_normal((n_streams, T, cols)) * 3 + 1).astype(np.float32)
    x[:, :, CONST_COL] = np.float32(1.5)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def _want(cols, win, variance, stream, T):
    out, n_t = restate(_streams(cols)[stream, :T], win, variance)
    out.setflags(write=False)
    return out, n_t


def _check_bound(block, n_t, slack=0.0):
    """|out| <= sqrt(n_t) with variance normalisation: the row is a member of its own window."""
    assert (np.abs(block) <= np.sqrt(n_t)[:, None] * (1.0 + slack)).all()


# ---------------------------------------------------------------- CPU ---------------------------------------------------------

def test_symbols_are_declared_exported_and_prototyped(sslib):
    from speechsauce_amd import _lib

    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "speechsauce_amd.h")).read(), flags=re.S)
    for name in NAMES:
        assert re.search(r"^int %s\(" % name, header, flags=re.M), name
        assert name in _lib.PROTOTYPES, name
        fn = getattr(sslib, name)
        assert fn.restype is C.c_int and len(fn.argtypes) == len(_lib.PROTOTYPES[name][1])
    assert len(_lib.PROTOTYPES["ss_cmvn_stream_state_len"][1]) == 3
    assert len(_lib.PROTOTYPES["ss_cmvn_stream_packed_device"][1]) == 12
    assert len(_lib.PROTOTYPES["ss_cmvn_stream_packed"][1]) == 10
    assert sslib.ss_abi_version() == 7  # entry points only: the version stays


def _state_len(sslib, cols, win):
    L = C.c_size_t(12345)
    return sslib.ss_cmvn_stream_state_len(cols, win, C.byref(L)), L.value


def test_state_len_formula_and_rejections(sslib):
    for cols in COLS + (1,):
        for win in WINS:
            assert _state_len(sslib, cols, win) == (0, (win - 1) * cols + 1)
    assert _state_len(sslib, 13, 1) == (0, 1)
    assert _state_len(sslib, 0, 301) == (3, 12345)  # SS_ERR_ARG, the output untouched
    assert _state_len(sslib, 13, 0) == (3, 12345)
    assert _state_len(sslib, 1 << 20, (1 << 11) + 1)[0] == 3  # L = 2^31 + 1
    assert _state_len(sslib, 1 << 20, 1 << 11) == (0, ((1 << 11) - 1) * (1 << 20) + 1)  # just below
    assert _state_len(sslib, 1 << 31, 1)[0] == 3
    assert sslib.ss_cmvn_stream_state_len(13, 301, None) == 3


def _host_buffers(cols=13, win=4, rows=6, pool_streams=4):
    L = (win - 1) * cols + 1
    vec = np.ones((rows, cols), np.float32)
    out = np.full((rows, cols), -5.0, np.float32)
    pool = np.full((pool_streams, L), -7.0, np.float32)
    return vec, out, pool


def test_argument_errors_are_decided_before_the_device_is_touched(sslib):
    """Every call here is rejected (or has nothing to do) on the host: none of the pointers is ever handed to the device, so host
    arrays stand in for device buffers."""
    cols, win, rows, P = 13, 4, 6, 4
    vec, out, pool = _host_buffers(cols, win, rows, P)
    ro = np.array([0, 2, 6], np.int64)
    sl = np.array([1, 3], np.int32)
    v, o, p, r, s = vec.ctypes.data, out.ctypes.data, pool.ctypes.data, ro.ctypes.data, sl.ctypes.data

    def dev(vec=v, n=2, ro=r, total=rows, sl=s, P=P, cols=cols, win=win, pool=p, out=o):
        return sslib.ss_cmvn_stream_packed_device(vec, n, ro, total, sl, P, cols, win, 1, pool, out, None)

    def host(vec=v, n=2, ro=r, sl=s, P=P, cols=cols, win=win, pool=p, out=o):
        return sslib.ss_cmvn_stream_packed(vec, n, ro, sl, P, cols, win, 1, pool, out)

    # an empty call is SS_OK with nothing launched, also without a device and whatever else is passed
    assert dev(n=0) == 0 and host(n=0) == 0
    assert sslib.ss_cmvn_stream_packed_device(None, 0, None, 0, None, 0, 0, 0, 0, None, None, None) == 0
    assert sslib.ss_cmvn_stream_packed(None, 0, None, None, 0, 0, 0, 0, None, None) == 0
    for call in (dev, host):
        for name in ("vec", "ro", "sl", "pool", "out"):
            assert call(**{name: None}) == 3, (call.__name__, name)  # null buffers
        assert call(cols=0) == 3 and call(win=0) == 3
        assert call(n=1 << 31) == 3 and call(P=1 << 31) == 3 and call(cols=1 << 31) == 3
        assert call(cols=1 << 20, win=(1 << 11) + 1) == 3  # L >= 2^31
        assert call(P=0) == 3
        assert call(out=v) == 3  # in place is not offered
        assert b"in place" in sslib.ss_last_error_string()
        assert call(out=v + 4 * cols) == 3  # out overlapping vec one row along
        assert call(pool=v) == 3 and call(pool=o) == 3 and call(pool=o + 4 * (rows * cols - 1)) == 3  # the pool overlapping vec / out
    assert dev(total=1 << 31) == 3
    # win_size == 1: L = 1, and the pool may still not be NULL (one rule)
    assert dev(win=1, pool=None) == 3 and host(win=1, pool=None) == 3
    # the host form's table errors name the first bad entry
    for bad_ro, entry in (([1, 2, 6], b"entry 0"), ([0, 4, 3], b"entry 1")):
        b = np.array(bad_ro, np.int64)
        assert host(ro=b.ctypes.data) == 3 and entry in sslib.ss_last_error_string(), bad_ro
    b3 = np.array([0, 1, 3, 2, 6], np.int64)
    s4 = np.array([0, 1, 2, 3], np.int32)
    assert host(n=4, ro=b3.ctypes.data, sl=s4.ctypes.data) == 3 and b"entry 2" in sslib.ss_last_error_string()
    for bad_sl, entry in (([1, 4], b"entry 1"), ([-1, 3], b"entry 0"), ([3, 3], b"entry 1")):
        b = np.array(bad_sl, np.int32)
        assert host(sl=b.ctypes.data) == 3 and entry in sslib.ss_last_error_string(), bad_sl
    # entries without rows only: nothing to do, no device needed
    z = np.zeros(3, np.int64)
    assert host(ro=z.ctypes.data) == 0
    assert (out == -5.0).all() and (pool == -7.0).all() and (vec == 1.0).all()  # nothing was written by any of it


def _has_gpu():
    try:
        import torch

        return torch.cuda.is_available()
    except Exception:
        return False


@pytest.mark.skipif(_has_gpu(), reason="checks the no-device failure mode")
def test_python_class_fails_loudly_without_a_device(sslib):
    import speechsauce_amd as ss
    from speechsauce_amd import SpeechSauceError

    m = ss.CmvnStreamPool(4, 13, win_size=4)
    with pytest.raises(SpeechSauceError) as e:
        m(np.zeros((3, 13), np.float32), [0, 2, 3], [2, 0])
    assert e.value.status == 4
    assert m.state is None


def test_python_argument_rules(sslib):
    import speechsauce_amd as ss

    m = ss.CmvnStreamPool(4, 13)
    assert (m.pool_streams, m.cols, m.win_size, m.variance_normalization, m.state_len) == (4, 13, 301, False, 300 * 13 + 1)
    assert m.state is None
    z = lambda r, c=13, dt=np.float32: np.zeros((r, c), dt)  # noqa: E731
    with pytest.raises(TypeError):
        m(z(3, dt=np.float64), [0, 3], [0])  # wrong dtype
    with pytest.raises(ValueError):
        m(np.zeros(39, np.float32), [0, 3], [0])  # not 2-D
    with pytest.raises(ValueError):
        m(z(3, 12), [0, 3], [0])  # wrong number of columns
    with pytest.raises(ValueError):
        m(z(3), [0, 2, 3], [0])  # table length
    with pytest.raises(ValueError):
        m(z(3), [0, 3], [4])  # a slot outside the pool
    with pytest.raises(ValueError):
        m(z(3), [0, 3], [-1])
    with pytest.raises(ValueError):
        m(z(3), [0, 2, 3], [1, 1])  # a slot named twice
    with pytest.raises(ValueError):
        m(z(3), [1, 3], [0])  # ro[0] != 0
    with pytest.raises(ValueError):
        m(z(3), [0, 2, 1], [0, 1])  # a decreasing pair
    with pytest.raises(ValueError):
        m(z(3), [0, 4], [0])  # past the block
    with pytest.raises(TypeError):
        m(z(3), np.array([0.0, 3.0]), [0])  # a float table
    assert m.state is None  # nothing was created by the rejected calls
    m.reset()
    m.reset(slots=[1])  # no state yet: nothing to do
    for bad in (dict(pool_streams=0, cols=13), dict(pool_streams=4, cols=0), dict(pool_streams=4, cols=13, win_size=0)):
        with pytest.raises(ValueError):
            ss.CmvnStreamPool(**bad)
    with pytest.raises(ss.SpeechSauceError) as e:
        ss.CmvnStreamPool(1, 1 << 20, win_size=(1 << 11) + 1)
    assert e.value.status == 3
    assert ss.CmvnStreamPool(2, 40, win_size=1, variance_normalization=True).state_len == 1
    assert "CmvnStreamPool" in ss.__all__


@pytest.mark.parametrize("cols", COLS)
def test_the_restatement_itself(cols):
    T = 340
    x = _streams(cols)[0, :T]
    for win in WINS:
        mean_only, n_t = restate(x, win, False)
        both, _ = restate(x, win, True)
        assert n_t[0] == 1 and n_t[-1] == min(T, win)
        _check_bound(both, n_t)
        assert (mean_only[:, CONST_COL] == 0).all() and (both[:, CONST_COL] == 0).all()  # a constant column: exact zeros
        assert (mean_only[0] == 0).all() and (both[0] == 0).all()  # the first row is alone in its window
        if win == 1:
            assert (mean_only == 0).all() and (both == 0).all()
        else:
            assert np.abs(mean_only).max() > 1.0 and np.abs(both).max() > 0.5
        # against the definition written out for one late element
        t, c = T - 1, cols - 1
        W = x[t - n_t[t] + 1:t + 1, c].astype(np.float64)
        assert abs(mean_only[t, c] - (W[-1] - W.mean())) < 1e-12
        assert abs(both[t, c] - (W[-1] - W.mean()) / (W.std() + EPS)) < 1e-9


# ---------------------------------------------------------------- GPU ---------------------------------------------------------

def _raw_call(torch, lib, x, n_active, d_ro, total_rows, d_sl, pool_streams, cols, win, variance, pool, out, stream=None):
    """The device entry on device tables as they are; returns its status."""
    st = C.c_void_p(stream if stream is not None else torch.cuda.current_stream().cuda_stream)
    return lib.ss_cmvn_stream_packed_device(x.data_ptr(), n_active, d_ro.data_ptr(), total_rows, d_sl.data_ptr(), pool_streams, cols, win,
                                            int(variance), pool.data_ptr(), out.data_ptr(), st)


def _pool_call(torch, lib, chunks, slots, pool, cols, win, variance):
    """One call on a list of [R_i, cols] device blocks; returns (out [total_rows, cols], ro) with ro the host row offsets."""
    ro = np.zeros(len(chunks) + 1, np.int64)
    np.cumsum([int(c.shape[0]) for c in chunks], out=ro[1:])
    R = int(ro[-1])
    x = torch.cat(list(chunks)) if R else torch.zeros((1, cols), device="cuda")
    out = torch.full((max(R, 1), cols), float("nan"), device="cuda")
    d_ro = torch.from_numpy(ro).cuda()
    d_sl = torch.tensor(list(slots), dtype=torch.int32, device="cuda")
    rc = _raw_call(torch, lib, x, len(chunks), d_ro, R, d_sl, pool.shape[0], cols, win, variance, pool, out)
    assert rc == 0, lib.ss_last_error_string()
    return out[:R], ro


def _feed(torch, lib, s, cuts, order, pool, slots, win, variance):
    """Feed streams s [B, T, cols] (device) through the schedule cuts[k][b] (rows of stream b in call k, -1: absent), the entries of
    call k standing in order[k]; returns the rows per stream [B, T_fed, cols]."""
    B, cols = s.shape[0], s.shape[2]
    fed = [sum(max(c[b], 0) for c in cuts) for b in range(B)]
    got = [torch.full((fed[b], cols), float("nan"), device="cuda") for b in range(B)]
    at = [0] * B
    for k, cut in enumerate(cuts):
        entries = [b for b in order[k] if cut[b] >= 0]
        chunks = [s[b, at[b]:at[b] + cut[b]] for b in entries]
        out, ro = _pool_call(torch, lib, chunks, [slots[b] for b in entries], pool, cols, win, variance)
        for i, b in enumerate(entries):
            got[b][at[b]:at[b] + cut[b]] = out[ro[i]:ro[i + 1]]
            at[b] += cut[b]
    assert at == fed
    return got


def _bits(t):
    import torch

    return t.contiguous().view(torch.int32)


@pytest.mark.gpu
@pytest.mark.parametrize("variance", [False, True])
@pytest.mark.parametrize("win", WINS)
@pytest.mark.parametrize("cols", COLS)
def test_parity_with_the_restatement_over_three_ticks(sslib, cols, win, variance):
    import torch

    L = (win - 1) * cols + 1
    s = torch.from_numpy(_streams(cols).copy()).cuda()
    pool = torch.zeros((POOL, L), device="cuda")
    order = [[4, 0, 6, 2, 5, 1, 3], [6, 5, 4, 3, 2, 1, 0], [1, 3, 5, 0, 2, 4, 6]]
    got = _feed(torch, sslib, s, TICKS, order, pool, SLOTS, win, variance)
    torch.cuda.synchronize()
    worst = 0.0
    for b in range(POOL):
        T = sum(t[b] for t in TICKS)
        want, n_t = _want(cols, win, variance, b, T)
        g = got[b].cpu().numpy()
        assert np.isfinite(g).all()
        if variance:
            _check_bound(want, n_t)
            _check_bound(g, n_t, slack=1e-6)
        assert (g[want == 0] == 0).all()  # win = 1, the first row, the constant column: exact zeros
        assert (want[:, CONST_COL] == 0).all() and (want[0] == 0).all() and (win > 1 or (want == 0).all())
        at = 0
        for tick in TICKS:  # per entry
            r = tick[b]
            if r:
                e = rel(g[at:at + r], want[at:at + r])
                worst = max(worst, e)
                assert e <= RTOL, (b, at, r, e)
            at += r
        assert rel(g, want) <= RTOL, (b, rel(g, want))  # per block
        # the pool row afterwards: the last min(T, win - 1) raw rows right-aligned, zeros in front, their count
        row = pool[SLOTS[b]].cpu().numpy()
        keep = min(T, win - 1)
        assert row[-1] == keep
        hist = row[:-1].reshape(win - 1, cols)
        assert np.array_equal(hist[win - 1 - keep:], _streams(cols)[b, T - keep:T]) and not hist[:win - 1 - keep].any()
    print(f"cols {cols} win {win} variance {variance}: worst per-entry rel {worst:.3g}")


# (cols, win): every window kind against every tile kind, without the full product
CUT_SHAPES = [(13, 301), (40, 31), (80, 4), (13, 2), (40, 1), (80, 301)]


@pytest.mark.gpu
@pytest.mark.parametrize("variance", [False, True])
@pytest.mark.parametrize("cols,win", CUT_SHAPES)
def test_rows_and_state_do_not_depend_on_how_the_stream_was_cut(sslib, cols, win, variance):
    import torch

    B, T = 3, 340  # 340 > 301: the window slides fully in every cutting
    L = (win - 1) * cols + 1
    s = torch.from_numpy(_streams(cols)[:B, :T].copy()).cuda()
    slots = [5, 0, 3]
    rng = np.random.default_rng(7)
    cuttings = {"one_call": [[T] * B], "row_by_row": [[1] * B] * T}
    cuts = []
    left = np.full(B, T)
    while left.any():
        c = np.minimum(rng.integers(0, 60, B) * (rng.random(B) < 0.7), left)  # zero-row entries in between
        absent = (c == 0) & (rng.random(B) < 0.3)
        cuts.append([-1 if a else int(v) for v, a in zip(c, absent)])
        left -= c
    assert any(0 in c for c in cuts) and any(-1 in c for c in cuts) and len(cuts) > 8
    cuttings["random"] = cuts
    rows, pools = {}, {}
    for key, cut in cuttings.items():
        pool = torch.zeros((POOL, L), device="cuda")
        order = [list(rng.permutation(B)) for _ in cut]
        rows[key] = torch.stack(_feed(torch, sslib, s, cut, order, pool, slots, win, variance))
        pools[key] = pool
    torch.cuda.synchronize()
    want = np.stack([_want(cols, win, variance, b, T)[0] for b in range(B)])
    assert rel(rows["one_call"].cpu().numpy(), want) <= RTOL
    for key in ("row_by_row", "random"):
        assert torch.equal(_bits(rows[key]), _bits(rows["one_call"])), key
        assert torch.equal(_bits(pools[key]), _bits(pools["one_call"])), key
    others = [r for r in range(POOL) if r not in slots]
    assert not pools["random"][others].any()


@pytest.mark.gpu
@pytest.mark.parametrize("cols,win", [(13, 301), (40, 31), (80, 4)])
def test_an_entry_does_not_depend_on_its_place_slot_or_neighbours(sslib, cols, win):
    import torch

    L = (win - 1) * cols + 1
    s = torch.from_numpy(_streams(cols).copy()).cuda()
    P = 12
    base = torch.zeros((P, L), device="cuda")
    warm = [s[b, :20] for b in range(4)]
    _pool_call(torch, sslib, warm, [7, 0, 1, 2], base, cols, win, True)  # some history everywhere
    base[9] = base[7]  # the same stream state in another slot
    mine = s[0, 20:25]
    other = [s[b, 20:20 + r] for b, r in ((1, 1), (2, 37), (3, 2), (4, 9))]
    empty = mine[:0]
    layouts = {"first": ([mine] + other, [7, 0, 1, 2, 3]),
               "last": (other + [mine], [0, 1, 2, 3, 7]),
               "other_slot": (other[:2] + [mine] + other[2:], [0, 1, 9, 2, 3]),
               "between_empties": (other[:2] + [empty, mine, empty] + other[2:], [0, 1, 10, 7, 11, 2, 3]),
               "alone": ([mine], [7])}
    rows, states = {}, {}
    for key, (chunks, slots) in layouts.items():
        pool = base.clone()
        out, ro = _pool_call(torch, sslib, chunks, slots, pool, cols, win, True)
        slot = 9 if key == "other_slot" else 7
        i = slots.index(slot)
        rows[key] = out[ro[i]:ro[i + 1]].clone()
        states[key] = pool[slot].clone()
        if key == "between_empties":
            assert torch.equal(_bits(pool[10]), _bits(base[10])) and torch.equal(_bits(pool[11]), _bits(base[11]))
    torch.cuda.synchronize()
    want, _ = _want(cols, win, True, 0, 25)
    assert rel(rows["alone"].cpu().numpy(), want[20:25]) <= RTOL
    for key in layouts:
        assert torch.equal(_bits(rows[key]), _bits(rows["alone"])), key
        assert torch.equal(_bits(states[key]), _bits(states["alone"])), key


@pytest.mark.gpu
def test_memory_the_call_does_not_own_is_left_as_it_was(sslib):
    import torch

    cols, win, P, FILL = 40, 31, 9, -777.0
    L = (win - 1) * cols + 1
    s = torch.from_numpy(_streams(cols).copy()).cuda()
    pool = torch.full((P, L), FILL, device="cuda")
    named, empties = [4, 1, 7], [2, 6]
    pool[named] = 0.0
    before = pool.clone()
    chunks = [s[0, :3], s[1, :0], s[2, :40], s[3, :0], s[4, :1]]
    slots = [4, 2, 1, 6, 7]
    ro = np.zeros(6, np.int64)
    np.cumsum([c.shape[0] for c in chunks], out=ro[1:])
    R, EXTRA = int(ro[-1]), 5
    x = torch.cat(chunks + [s[5, :EXTRA]])
    out = torch.full((R + EXTRA, cols), FILL, device="cuda")
    rc = _raw_call(torch, sslib, x, 5, torch.from_numpy(ro).cuda(), R + EXTRA, torch.tensor(slots, dtype=torch.int32, device="cuda"), P, cols,
                   win, True, pool, out)
    assert rc == 0, sslib.ss_last_error_string()
    torch.cuda.synchronize()
    assert (out[R:] == FILL).all()  # rows past ro[n_active]
    assert torch.isfinite(out[:R]).all() and not (out[:R] == FILL).any()
    for r in range(P):
        if r in named:
            assert not torch.equal(pool[r], before[r]), r
        else:  # never named, or named by an entry without rows
            assert torch.equal(_bits(pool[r]), _bits(before[r])), r
    for b, i in ((0, 0), (2, 2), (4, 4)):
        want, _ = _want(cols, win, True, b, int(chunks[i].shape[0]))
        assert rel(out[ro[i]:ro[i + 1]].cpu().numpy(), want) <= RTOL


@pytest.mark.gpu
def test_bad_device_tables_and_count_words_are_contained(sslib):
    """A contract check, run once.  The entry decoder bounds every access before it happens: a bad entry is skipped, a bad count
    word is read as a fresh stream, nothing outside the buffers is touched and the good entries of the same call are still exact."""
    import torch

    cols, win, P, GUARD, FILL = 13, 31, 8, 4, -777.0
    H = win - 1
    L = H * cols + 1
    s = torch.from_numpy(_streams(cols).copy()).cuda()

    def single(chunk, state_row):
        """The expected rows and pool row of one entry: the same call on that entry alone."""
        p = state_row[None, :].clone()
        o, _ = _pool_call(torch, sslib, [chunk], [0], p, cols, win, True)
        return o.clone(), p[0].clone()

    # ---- bad tables: entry i owns ro[i] .. ro[i+1] ----
    ro = np.array([0, 3, 5, 4, 6, 9, -2, 11, 13, 16], np.int64)
    total_rows = 14
    slots = [1, P, 2, 3, -1, 4, 6, 5, 7]
    #        e0 good | e1 slot = pool_streams | e2 decreasing | e3 good | e4 slot = -1 | e5 decreasing, below 0 | e6 starts below 0 |
    #        e7 good | e8 ends past total_rows
    good = {0: (0, 3), 3: (4, 6), 7: (11, 13)}
    x_g = torch.full((total_rows + 2 * GUARD, cols), FILL, device="cuda")
    x = x_g[GUARD:GUARD + total_rows]
    x.copy_(s[6, 100:100 + total_rows])
    x_before = x_g.clone()
    out_g = torch.full((total_rows + 2 * GUARD, cols), FILL, device="cuda")
    out = out_g[GUARD:GUARD + total_rows]
    pool_g = torch.full((P + 2 * GUARD, L), FILL, device="cuda")
    pool = pool_g[GUARD:GUARD + P]
    _pool_call(torch, sslib, [s[b % POOL, :40] for b in range(P)], list(range(P)), pool.zero_(), cols, win, True)  # valid states everywhere
    before = pool.clone()
    want = {i: single(x[a:b], before[slots[i]]) for i, (a, b) in good.items()}
    rc = _raw_call(torch, sslib, x, len(slots), torch.from_numpy(ro).cuda(), total_rows, torch.tensor(slots, dtype=torch.int32, device="cuda"),
                   P, cols, win, True, pool, out)
    assert rc == 0, sslib.ss_last_error_string()  # the tables are device data: the call itself cannot know
    torch.cuda.synchronize()
    written = np.zeros(total_rows, bool)
    for i, (a, b) in good.items():
        assert torch.equal(_bits(out[a:b]), _bits(want[i][0])), i
        assert torch.equal(_bits(pool[slots[i]]), _bits(want[i][1])), i
        written[a:b] = True
    assert (out[torch.from_numpy(~written).cuda()] == FILL).all()  # what the skipped entries claimed keeps its pre-fill
    for r in set(range(P)) - {slots[i] for i in good}:
        assert torch.equal(_bits(pool[r]), _bits(before[r])), r
    assert (out_g[:GUARD] == FILL).all() and (out_g[GUARD + total_rows:] == FILL).all()
    assert (pool_g[:GUARD] == FILL).all() and (pool_g[GUARD + P:] == FILL).all()
    assert torch.equal(_bits(x_g), _bits(x_before))

    # ---- bad count words: read as 0, a fresh stream, whatever the history floats hold ----
    words = [float("nan"), -1.0, float(win), 1e9, 1.5, float("inf")]
    gen = torch.Generator(device="cuda")
    gen.manual_seed(9)
    pool.copy_(torch.randn((P, L), generator=gen, device="cuda") * 50)  # garbage history
    for r, w in enumerate(words):
        pool[r, -1] = w
    control = before[6].clone()
    pool[6] = control  # one valid state beside them
    assert control[-1] == H
    chunks = [s[r, 200:200 + n] for r, n in zip(range(len(words)), (2, 1, 5, 35, 3, 2))] + [s[6, 40:44]]
    ro2 = np.zeros(len(chunks) + 1, np.int64)
    np.cumsum([c.shape[0] for c in chunks], out=ro2[1:])
    R = int(ro2[-1])
    x2_g = torch.full((R + 2 * GUARD, cols), FILL, device="cuda")
    x2_g[GUARD:GUARD + R] = torch.cat(chunks)
    out2_g = torch.full((R + 2 * GUARD, cols), FILL, device="cuda")
    fresh = torch.zeros(L, device="cuda")
    want2 = [single(c, fresh) for c in chunks[:-1]] + [single(chunks[-1], control)]
    rc = _raw_call(torch, sslib, x2_g[GUARD:GUARD + R], len(chunks), torch.from_numpy(ro2).cuda(), R,
                   torch.tensor(list(range(len(words))) + [6], dtype=torch.int32, device="cuda"), P, cols, win, True, pool, out2_g[GUARD:GUARD + R])
    assert rc == 0, sslib.ss_last_error_string()
    torch.cuda.synchronize()
    for i, c in enumerate(chunks):
        slot = i if i < len(words) else 6
        assert torch.equal(_bits(out2_g[GUARD + ro2[i]:GUARD + ro2[i + 1]]), _bits(want2[i][0])), i
        assert torch.equal(_bits(pool[slot]), _bits(want2[i][1])), i
        if i < len(words):  # and a fresh stream is what the definition says
            ref, _ = restate(c.cpu().numpy(), win, True)
            assert rel(want2[i][0].cpu().numpy(), ref) <= RTOL, i
    assert (out2_g[:GUARD] == FILL).all() and (out2_g[GUARD + R:] == FILL).all()
    assert (pool_g[:GUARD] == FILL).all() and (pool_g[GUARD + P:] == FILL).all()


@pytest.mark.gpu
@pytest.mark.parametrize("variance", [False, True])
def test_zeroing_a_pool_row_gives_a_fresh_stream(sslib, variance):
    import torch

    cols, win = 40, 31
    L = (win - 1) * cols + 1
    s = torch.from_numpy(_streams(cols).copy()).cuda()
    pool = torch.zeros((POOL, L), device="cuda")
    _pool_call(torch, sslib, [s[0, :50], s[1, :50]], [2, 5], pool, cols, win, variance)
    pool[2] = 0.0  # reset mid-stream
    out, ro = _pool_call(torch, sslib, [s[0, 50:90], s[1, 50:90]], [2, 5], pool, cols, win, variance)
    torch.cuda.synchronize()
    fresh, _ = restate(_streams(cols)[0, 50:90], win, variance)
    cont, _ = _want(cols, win, variance, 1, 90)
    assert rel(out[:40].cpu().numpy(), fresh) <= RTOL and (out[0] == 0).all()
    assert rel(out[40:].cpu().numpy(), cont[50:]) <= RTOL
    p2 = torch.zeros((1, L), device="cuda")
    alone, _ = _pool_call(torch, sslib, [s[0, 50:90]], [0], p2, cols, win, variance)
    assert torch.equal(_bits(out[:40]), _bits(alone)) and torch.equal(_bits(pool[2]), _bits(p2[0]))


@pytest.mark.gpu
@pytest.mark.parametrize("variance", [False, True])
@pytest.mark.parametrize("cols", COLS)
def test_anchor_on_the_reference_cmvn(ss, sslib, cols, variance):
    """With win >= G the window of row G - 1 is the stream's first G rows: the row equals row G - 1 of ss_cmvn on them (another
    summation order, so not bit for bit)."""
    import torch

    G = 50
    s = torch.from_numpy(_streams(cols)[:2, :G].copy()).cuda()
    whole = ss.cmvn(s, variance_normalization=variance)  # [2, G, cols]: the one-shot call per clip
    for win in (G, 64, 301):
        pool = torch.zeros((2, (win - 1) * cols + 1), device="cuda")
        a, _ = _pool_call(torch, sslib, [s[0, :20], s[1, :G]], [1, 0], pool, cols, win, variance)
        b, _ = _pool_call(torch, sslib, [s[0, 20:G]], [1], pool, cols, win, variance)
        torch.cuda.synchronize()
        for got, want in ((b[-1], whole[0, -1]), (a[-1], whole[1, -1])):
            assert rel(got.cpu().numpy(), want.cpu().numpy()) <= RTOL, (win, rel(got.cpu().numpy(), want.cpu().numpy()))


@pytest.mark.gpu
@pytest.mark.parametrize("variance", [False, True])
def test_host_form_and_python_class_equal_the_device_form(ss, sslib, variance):
    import torch

    cols, win, P = 13, 31, 9
    L = (win - 1) * cols + 1
    s = torch.from_numpy(_streams(cols).copy()).cuda()
    calls = [([s[0, :3], s[1, :0], s[2, :40]], [4, 1, 7]),
             ([s[2, 40:45], s[0, 3:4]], [7, 4]),
             ([s[1, :37], s[0, 4:6], s[3, :0]], [1, 4, 0])]
    pool_d = torch.zeros((P, L), device="cuda")
    pool_h = np.zeros((P, L), np.float32)
    m_np = ss.CmvnStreamPool(P, cols, win_size=win, variance_normalization=variance)
    m_t = ss.CmvnStreamPool(P, cols, win_size=win, variance_normalization=variance)
    for chunks, slots in calls:
        dev, ro = _pool_call(torch, sslib, chunks, slots, pool_d, cols, win, variance)
        torch.cuda.synchronize()
        dev = dev.cpu().numpy()
        R = int(ro[-1])
        xh = torch.cat(chunks).cpu().numpy()
        FILL = np.float32(-3.0)
        outh = np.full((R, cols), FILL)
        sl = np.asarray(slots, np.int32)
        before = pool_h.copy()
        dup = np.full(len(slots), slots[0], np.int32)
        rc = sslib.ss_cmvn_stream_packed(xh.ctypes.data, len(slots), ro.ctypes.data, dup.ctypes.data, P, cols, win, int(variance),
                                         pool_h.ctypes.data, outh.ctypes.data)
        assert rc == 3 and b"entry 1" in sslib.ss_last_error_string()  # a slot named twice: rejected, nothing written
        assert np.array_equal(pool_h, before) and (outh == FILL).all()
        rc = sslib.ss_cmvn_stream_packed(xh.ctypes.data, len(slots), ro.ctypes.data, sl.ctypes.data, P, cols, win, int(variance),
                                         pool_h.ctypes.data, outh.ctypes.data)
        assert rc == 0, sslib.ss_last_error_string()
        assert np.array_equal(outh.view(np.uint32), dev.view(np.uint32))
        assert np.array_equal(pool_h.view(np.uint32), pool_d.cpu().numpy().view(np.uint32))
        changed = {int(r) for r in np.flatnonzero((pool_h != before).any(axis=1))}
        assert changed <= {int(v) for v, c in zip(slots, chunks) if c.shape[0] > 0}  # only named rows with new rows moved
        got_np = m_np(xh, ro, slots)
        got_t = m_t(torch.cat(chunks), ro, slots)
        assert isinstance(got_np, np.ndarray) and torch.is_tensor(got_t)
        assert np.array_equal(got_np.view(np.uint32), dev.view(np.uint32))
        assert np.array_equal(got_t.cpu().numpy().view(np.uint32), dev.view(np.uint32))
    torch.cuda.synchronize()
    assert m_np.state.shape == (P, L) and np.array_equal(m_np.state, pool_h)
    assert torch.equal(_bits(m_t.state), _bits(pool_d))
    with pytest.raises(ValueError):
        m_np(torch.cat(calls[0][0]), [0, 3, 3, 43], [4, 1, 7])  # the pool lives on the host
    # reset(slots=[...]) makes exactly those streams fresh
    for m, to in ((m_np, lambda t: t.cpu().numpy()), (m_t, lambda t: t)):
        m.reset(slots=[4])
        st = m.state if isinstance(m.state, np.ndarray) else m.state.cpu().numpy()
        assert not st[4].any() and np.array_equal(st[7], pool_h[7])
        rows = m(to(s[0, 6:16].contiguous()), [0, 10], [4])
        rows = rows if isinstance(rows, np.ndarray) else rows.cpu().numpy()
        fresh, _ = restate(_streams(cols)[0, 6:16], win, variance)
        assert rel(rows, fresh) <= RTOL and (rows[0] == 0).all()
        m.reset()
        st = m.state if isinstance(m.state, np.ndarray) else m.state.cpu().numpy()
        assert not st.any()


def _hip_runtime():
    """The HIP runtime this process has loaded (torch's), for the stream-capture calls the graph-shape check needs."""
    with open("/proc/self/maps") as f:
        paths = {line.split()[-1] for line in f if "libamdhip64" in line}
    assert paths, "no HIP runtime loaded"
    return C.CDLL(sorted(paths)[0])


@pytest.mark.gpu
def test_graph_of_the_feature_call_and_the_normalisation_on_the_same_tables(ss, sslib):
    import torch

    from speechsauce_amd import _lib

    cfg = ss.SpeechConfig(_lib.make_params())  # the default 512-point shape
    N, CAP, P, STEP, COLS_, WIN, NORM = 5, 24, 8, 160, 13, 31, 100
    L = (WIN - 1) * COLS_ + 1
    x = torch.zeros(CAP * STEP, device="cuda")
    d_so = torch.zeros(N + 1, dtype=torch.int64, device="cuda")
    d_ro = torch.zeros(N + 1, dtype=torch.int64, device="cuda")
    d_sl = torch.arange(N, dtype=torch.int32, device="cuda")
    feat = torch.zeros((CAP, COLS_), device="cuda")
    out = torch.zeros((CAP, COLS_), device="cuda")
    fpool_g, fpool_e = torch.zeros((P, STEP), device="cuda"), torch.zeros((P, STEP), device="cuda")
    cpool_g, cpool_e = torch.zeros((P, L), device="cuda"), torch.zeros((P, L), device="cuda")

    def both(fpool, cpool, stream=None, n=N):
        st = C.c_void_p(stream if stream is not None else torch.cuda.current_stream().cuda_stream)
        rc = sslib.ss_mfcc_stream_packed_device(cfg.handle, x.data_ptr(), n, d_so.data_ptr(), d_ro.data_ptr(), CAP, d_sl.data_ptr(), P, NORM,
                                                fpool.data_ptr(), feat.data_ptr(), st)
        assert rc == 0, sslib.ss_last_error_string()
        rc = _raw_call(torch, sslib, feat, n, d_ro, CAP, d_sl, P, COLS_, WIN, True, cpool, out, stream=st.value)
        assert rc == 0, sslib.ss_last_error_string()

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up outside the capture (the zero tables are N entries without rows)
        both(fpool_g.clone(), cpool_g.clone(), stream=side.cuda_stream)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    # the shape of the captured normalisation alone: kernel nodes only, as many for 3 entries as for 5
    hip = _hip_runtime()
    hip.hipGraphGetNodes.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_size_t)]
    hip.hipGraphNodeGetType.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
    counts = []
    for n in (N, 3):
        raw, graph = torch.cuda.Stream(), C.c_void_p()
        assert hip.hipStreamBeginCapture(C.c_void_p(raw.cuda_stream), 2) == 0  # hipStreamCaptureModeRelaxed
        rc = _raw_call(torch, sslib, feat, n, d_ro, CAP, d_sl, P, COLS_, WIN, True, cpool_g, out, stream=raw.cuda_stream)
        assert hip.hipStreamEndCapture(C.c_void_p(raw.cuda_stream), C.byref(graph)) == 0
        assert rc == 0, sslib.ss_last_error_string()
        n_nodes = C.c_size_t()
        assert hip.hipGraphGetNodes(graph, None, C.byref(n_nodes)) == 0
        nodes = (C.c_void_p * n_nodes.value)()
        assert hip.hipGraphGetNodes(graph, nodes, C.byref(n_nodes)) == 0
        for node in nodes:
            kind = C.c_int(-1)
            assert hip.hipGraphNodeGetType(node, C.byref(kind)) == 0
            assert kind.value == 0  # hipGraphNodeTypeKernel
        assert hip.hipGraphDestroy(graph) == 0
        counts.append(n_nodes.value)
    assert counts[0] == counts[1] and 1 <= counts[0] <= 2, counts
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        both(fpool_g, cpool_g)
    rng = np.random.default_rng(44)
    for k in range(3):
        hops = rng.integers(0, 5, N)
        hops[rng.integers(0, N)] = 0  # an entry without rows
        slots = rng.permutation(P)[:N].astype(np.int32)
        so = np.zeros(N + 1, np.int64)
        np.cumsum(hops * STEP, out=so[1:])
        ro = so // STEP
        gen = torch.Generator(device="cuda")
        gen.manual_seed(45 + k)
        xs = torch.randn(int(so[-1]), generator=gen, device="cuda").mul_(0.1)
        x.zero_()
        x[:xs.numel()] = xs
        d_so.copy_(torch.from_numpy(so))
        d_ro.copy_(torch.from_numpy(ro))
        d_sl.copy_(torch.from_numpy(slots))
        feat.fill_(float("nan"))
        out.fill_(float("nan"))
        both(fpool_e, cpool_e)  # eager, on the other pools
        torch.cuda.synchronize()
        want_feat, want_out = feat.clone(), out.clone()
        feat.fill_(float("nan"))
        out.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        R = int(ro[-1])
        assert R > 0 and torch.isfinite(out[:R]).all()
        assert torch.equal(_bits(feat), _bits(want_feat)) and torch.equal(_bits(out), _bits(want_out)), k
        assert torch.isnan(out[R:]).all()  # rows past the last entry are left alone
        assert torch.equal(_bits(fpool_g), _bits(fpool_e)) and torch.equal(_bits(cpool_g), _bits(cpool_e)), k
    assert sslib.ss_config_device_status(cfg.handle) == 0
