"""Frame splicing and subsampling on the device: ss_splice_packed* on packed clips, ss_splice_stream_packed* / ss_splice_stream_flush*
over a pool of stream states, and the Python front's splice, splice_packed, lfr and SpliceStreamPool.

The stage copies bits, so every comparison is on uint32 views against the numpy restatement of the header (tests/splice_model.py).
The inputs are salted with NaNs of distinct payloads (quiet and signalling), -0.0, +-inf and denormals; outputs sit between guard
rows of a sentinel bit pattern that no input holds.
"""
import ctypes as C

import numpy as np
import pytest

from splice_model import PARAMS, SENTINEL, StreamModel, clip, delay_hist, splice_ref, u32, want

pytestmark = pytest.mark.gpu

ALL = PARAMS + ((32, 32, 1), (0, 32, 32))
COLS = (1, 13, 33, 80)
TILE = 64       # kSpliceTile, mfcc-rust_amd/csrc/ss_splice.hip: "constexpr unsigned kSpliceTile = 64;  // output rows per tile"
SPLIT_ALL = 8192  # packed_split, mfcc-rust_amd/csrc/ss_device.h: "want = std::max<unsigned long long>(1, 8192 / n_clips)"
GUARD = 3


def _fill(torch, shape):
    """a device block of the sentinel"""
    return torch.full(shape, int(SENTINEL) - (1 << 32), dtype=torch.int32, device="cuda").view(torch.float32)


def _bits(t):
    import torch

    return t.contiguous().view(torch.int32)


def _is_sentinel(t):
    return (_bits(t) == int(SENTINEL) - (1 << 32)).all()


def _host(t):
    return t.cpu().numpy()


def _stream():
    import torch

    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _offsets(lens, stride):
    ro = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    oo = np.concatenate([[0], np.cumsum([-(-int(n) // stride) for n in lens])]).astype(np.int64)
    return ro, oo


def _packed(torch, lib, clips, cols, left, right, stride, empties=0):
    """ss_splice_packed_device on a list of host clips [T_b, cols], `empties` clips without rows behind them; the output sits between
    guard rows.  -> (out [sum T_out, W * cols] on the host, oo)"""
    lens = [c.shape[0] for c in clips] + [0] * empties
    ro, oo = _offsets(lens, stride)
    R, RO, ocols = int(ro[-1]), int(oo[-1]), (left + 1 + right) * cols
    x = torch.from_numpy(np.concatenate(list(clips) + [np.zeros((1, cols), np.float32)])).cuda()
    out = _fill(torch, (RO + 2 * GUARD, ocols))
    d_ro, d_oo = torch.from_numpy(ro).cuda(), torch.from_numpy(oo).cuda()
    rc = lib.ss_splice_packed_device(x.data_ptr(), len(lens), d_ro.data_ptr(), R, d_oo.data_ptr(), RO, cols, left, right, stride,
                                     out[GUARD:].data_ptr(), _stream())
    assert rc == 0, lib.ss_last_error_string()
    torch.cuda.synchronize()
    assert _is_sentinel(out[:GUARD]) and _is_sentinel(out[GUARD + RO:])
    return _host(out[GUARD:GUARD + RO]), oo


@pytest.mark.parametrize("left,right,stride", ALL)
@pytest.mark.parametrize("cols", COLS)
def test_packed_is_the_restatement_bit_for_bit(sslib, cols, left, right, stride):
    """One block: the short lengths around the parameters, T_out one row below, at and one row above a tile of TILE output rows, and
    a clip of more than three tiles.  The block is padded with clips without rows up to SPLIT_ALL + 1 clips: packed_split then gives
    every clip ONE workgroup, which takes all of the long clip's tiles (test_a_clip_does_not_depend_on_its_place runs the other
    case, a clip's tiles shared among workgroups)."""
    import torch

    lens = [0, 1, 2, left, right + 1, stride - 1, stride, stride + 1, (TILE - 1) * stride, TILE * stride, TILE * stride + 1,
            (3 * TILE + 5) * stride - (stride // 2)]
    clips = [clip(cols, T, seed=i) for i, T in enumerate(lens)]
    got, oo = _packed(torch, sslib, clips, cols, left, right, stride, empties=SPLIT_ALL + 1 - len(lens))
    assert [int(b - a) for a, b in zip(oo[:len(lens)], oo[1:])][-4:] == [TILE - 1, TILE, TILE + 1, 3 * TILE + 5]
    ocols = (left + 1 + right) * cols
    if ocols % 2:  # odd rows: the clips start at every 16-byte phase
        assert {int(oo[i]) * ocols % 4 for i, T in enumerate(lens) if T} == {0, 1, 2, 3}
    for i, T in enumerate(lens):
        w = want(cols, T, left, right, stride, seed=i)
        g = got[oo[i]:oo[i + 1]]
        assert g.shape == w.shape, T
        bad = np.flatnonzero((u32(g) != u32(w)).any(axis=1))
        assert bad.size == 0, (T, bad[:8])


@pytest.mark.parametrize("cols,left,right,stride", [(13, 5, 5, 1), (33, 3, 3, 6), (80, 4, 7, 3), (1, 0, 32, 32), (13, 0, 0, 1)])
def test_a_clip_does_not_depend_on_its_place(sslib, cols, left, right, stride):
    """The same clip (three tiles, shared among workgroups here: few clips) in other places, behind other neighbours, at other output
    offsets and 16-byte phases."""
    import torch

    T = (2 * TILE + 22) * stride - (stride - 1)
    mine = clip(cols, T, seed=40)
    a, b, c = clip(cols, 7, seed=41), clip(cols, 300, seed=42), clip(cols, 1, seed=43)
    w = want(cols, T, left, right, stride, seed=40)
    starts = set()
    for clips, i in (([mine, a, b], 0), ([a, b, mine], 2), ([a, mine, b], 1), ([b, c, mine[:0], mine, a], 3), ([mine], 0), ([c, c, mine], 2)):
        got, oo = _packed(torch, sslib, clips, cols, left, right, stride)
        assert np.array_equal(u32(got[oo[i]:oo[i + 1]]), u32(w)), i
        starts.add(int(oo[i]))
    assert len(starts) >= 4


def _served(ro, oo, total_rows, total_out, stride):
    """the header's rule, clip by clip"""
    ok = []
    for b in range(len(ro) - 1):
        ok.append(bool(0 <= ro[b] <= ro[b + 1] <= total_rows and oo[b] >= 0 and oo[b + 1] - oo[b] == -(-(ro[b + 1] - ro[b]) // stride)
                       and oo[b + 1] <= total_out))
    return ok


# the last clip of the block: (ro entries appended behind 36, oo entries appended behind 17, total_out_rows, is the last clip served)
LAST = {"good": ([45], [20], 20, True), "reversed": ([30], [17], 17, False), "negative": ([-5, 3], [17, 20], 20, False),
        "past_the_end": ([51], [22], 22, False), "one_too_few": ([45], [19], 19, False), "one_too_many": ([45], [21], 21, False),
        "out_past_the_end": ([45], [20], 19, False)}


@pytest.mark.parametrize("last", sorted(LAST))
def test_bad_packed_segments_are_contained(sslib, last):
    """A reversed, negative or past-the-end row pair and an output pair with one row too few, one too many or ending past
    total_out_rows, in the interior and as the last clip: that clip is skipped whole, its rows of out keep the sentinel, the other
    clips are exact.  vec and out are allocated exactly to size."""
    import torch

    cols, left, right, stride, total_rows = 13, 4, 7, 3, 50
    ocols = (left + 1 + right) * cols
    #     b0 good | b1 reversed | b2 good | b3 reversed | b4 negative | b5 one too few | b6 one too many | b7 good |
    #     b8 ends past total_out_rows (a wrong count with it; LAST has the right count) | b9 no rows | b10 good | the last clip
    ro = [0, 7, 4, 10, -2, 6, 12, 19, 25, 31, 31, 36]
    oo = [0, 3, 3, 5, 5, 8, 9, 13, 15, 30, 15, 17]
    add_ro, add_oo, total_out, last_ok = LAST[last]
    ro, oo = np.array(ro + add_ro, np.int64), np.array(oo + add_oo, np.int64)
    n = len(ro) - 1
    ok = _served(ro, oo, total_rows, total_out, stride)
    assert ok[:11] == [True, False, True, False, False, False, False, True, False, False, True] and ok[-1] == last_ok and not any(ok[11:-1])
    src = clip(cols, total_rows, seed=50)
    x = torch.from_numpy(src.copy()).cuda()
    out = _fill(torch, (total_out, ocols))
    d_ro, d_oo = torch.from_numpy(ro).cuda(), torch.from_numpy(oo).cuda()
    rc = sslib.ss_splice_packed_device(x.data_ptr(), n, d_ro.data_ptr(), total_rows, d_oo.data_ptr(), total_out, cols, left, right, stride,
                                       out.data_ptr(), _stream())
    assert rc == 0, sslib.ss_last_error_string()  # the tables are device data: the call itself cannot know
    torch.cuda.synchronize()
    got = _host(out)
    written = np.zeros(total_out, bool)
    for b in range(n):
        if ok[b] and ro[b + 1] > ro[b]:
            assert np.array_equal(u32(got[oo[b]:oo[b + 1]]), u32(splice_ref(src[ro[b]:ro[b + 1]], left, right, stride))), b
            written[oo[b]:oo[b + 1]] = True
    assert written.sum() == 3 + 2 + 2 + 2 + (3 if last_ok else 0)
    assert (u32(got[~written]) == SENTINEL).all()  # rows of no served clip keep the sentinel
    assert np.array_equal(u32(_host(x)), u32(src)) and np.array_equal(_host(d_ro), ro) and np.array_equal(_host(d_oo), oo)


# ---------------------------------------------------------------- the pool ----------------------------------------------------

def _stream_raw(torch, lib, x, n_active, d_ro, total_rows, d_sl, pool_streams, cols, p, pool, out, stream=None):
    st = C.c_void_p(stream) if stream is not None else _stream()
    return lib.ss_splice_stream_packed_device(x.data_ptr(), n_active, d_ro.data_ptr(), total_rows, d_sl.data_ptr(), pool_streams, cols, *p,
                                              pool.data_ptr(), out.data_ptr(), st)


def _stream_call(torch, lib, chunks, slots, pool, cols, p, slack=2):
    """One pool call on a list of [R_i, cols] device blocks (whole periods) plus `slack` periods that no entry owns -> (out [total_rows
    / stride, W * cols], ro); the slack rows of out are checked here."""
    left, right, stride = p
    ro = np.concatenate([[0], np.cumsum([int(c.shape[0]) for c in chunks])]).astype(np.int64)
    R = int(ro[-1])
    x = torch.cat(list(chunks) + [torch.zeros((slack * stride + 1, cols), device="cuda")])
    out = _fill(torch, (R // stride + slack, (left + 1 + right) * cols))
    rc = _stream_raw(torch, lib, x, len(chunks), torch.from_numpy(ro).cuda(), R + slack * stride, torch.tensor(list(slots), dtype=torch.int32, device="cuda"),
                     pool.shape[0], cols, p, pool, out)
    assert rc == 0, lib.ss_last_error_string()
    torch.cuda.synchronize()
    assert _is_sentinel(out[R // stride:])
    return out[:R // stride], ro


def _flush_call(torch, lib, slots, pool, cols, p):
    left, right, stride = p
    D = right // stride
    out = _fill(torch, (len(slots) * D + GUARD, (left + 1 + right) * cols))
    d_sl = torch.tensor(list(slots), dtype=torch.int32, device="cuda")
    rc = lib.ss_splice_stream_flush_device(len(slots), d_sl.data_ptr(), pool.shape[0], cols, *p, pool.data_ptr(), out.data_ptr() if D else None, _stream())
    assert rc == 0, lib.ss_last_error_string()
    torch.cuda.synchronize()
    assert _is_sentinel(out[len(slots) * D:])
    return out[:len(slots) * D]


PERIODS = [4, 3, 6, 5, 2, 7, 1, 9, 4]           # per stream, in all
CUTS = (([0, 1, 1, 3, 0, 0, 0, 5, 2], [2, 0, 3, 1, 2, 3, 0, 4, 0], [2, 2, 2, 1, 0, 4, 1, 0, 2]),
        ([1, 0, 2, 0, 1, 0, 0, 3, 4], [3, 3, 4, 5, 1, 7, 1, 6, 0], [0, 0, 0, 0, 0, 0, 0, 0, 0]),
        ([2, 2, 2, 2, 2, 2, 1, 2, 2], [1, 1, 2, 2, 0, 3, 0, 3, 1], [1, 0, 2, 1, 0, 2, 0, 4, 1]))
SLOTS = [11, 3, 14, 0, 7, 9, 2, 12, 5]          # non-monotone, in a pool of 16 rows


@pytest.mark.parametrize("cols,left,right,stride", [(13,) + p for p in ALL] + [(c, 5, 5, 1) for c in (1, 33, 80)] + [(33, 4, 7, 3), (80, 3, 3, 6)])
def test_pool_rows_plus_flush_are_the_packed_call_however_the_streams_are_cut(sslib, cols, left, right, stride):
    """Nine streams in a 16-row pool, cut three ways into three calls (entries without rows in every call, the entry order reversed
    in the third cut), then the flush: per stream the rows after the first D are ss_splice_packed_device on the whole clip bit for
    bit, the first D are +0.0, the final pool rows agree between the cuts and with the model, rows of the pool that no entry names
    and rows of out that no entry owns keep the sentinel, and an entry without rows leaves its pool row bit for bit."""
    import torch

    p = (left, right, stride)
    D, H = delay_hist(*p)
    assert all(sum(c[i] for c in cut) == k for cut in CUTS for i, k in enumerate(PERIODS))
    clips = [clip(cols, k * stride, seed=70 + b) for b, k in enumerate(PERIODS)]
    dev = [torch.from_numpy(c.copy()).cuda() for c in clips]
    whole, off = _packed(torch, sslib, clips, cols, *p)
    finals = []
    for ci, cut in enumerate(CUTS):
        order = list(range(9)) if ci < 2 else list(range(8, -1, -1))
        pool = _fill(torch, (16, H * cols + 1))
        pool[SLOTS] = 0.0
        at, got = [0] * 9, [[] for _ in range(9)]
        for call in cut:
            before = pool.clone()
            chunks = [dev[b][at[b]:at[b] + call[b] * stride] for b in order]
            out, ro = _stream_call(torch, sslib, chunks, [SLOTS[b] for b in order], pool, cols, p)
            for i, b in enumerate(order):
                got[b].append(out[ro[i] // stride:ro[i + 1] // stride])
                at[b] += call[b] * stride
                if call[b] == 0:
                    assert torch.equal(_bits(pool[SLOTS[b]]), _bits(before[SLOTS[b]])), (ci, b)
        for b in range(9):
            m = StreamModel(cols, *p)
            m.push(clips[b])
            assert np.array_equal(u32(_host(pool[SLOTS[b]])), u32(m.pool_row())), (ci, b)
        finals.append(pool.clone())
        tail = _flush_call(torch, sslib, SLOTS[::-1], pool, cols, p)  # in another order
        for b in range(9):
            j = 8 - b
            rows = _host(torch.cat(got[b] + [tail[j * D:(j + 1) * D]]))
            assert rows.shape == (PERIODS[b] + D, (left + 1 + right) * cols)
            assert not u32(rows[:D]).any(), (ci, b)  # warm-up rows: +0.0
            w = whole[off[b]:off[b + 1]]
            assert np.array_equal(u32(rows[D:]), u32(w)), (ci, b)
            assert np.array_equal(u32(w), u32(want(cols, PERIODS[b] * stride, *p, seed=70 + b)))
        unnamed = [r for r in range(16) if r not in SLOTS]
        assert _is_sentinel(pool[unnamed]) and not _bits(pool[SLOTS]).any()  # flushed streams are fresh
    assert torch.equal(_bits(finals[0]), _bits(finals[1])) and torch.equal(_bits(finals[0]), _bits(finals[2]))


@pytest.mark.parametrize("cols,left,right,stride", [(13, 5, 5, 1), (33, 3, 3, 6), (80, 4, 7, 3), (13, 0, 0, 3)])
def test_an_entry_does_not_depend_on_its_place_slot_or_neighbours(sslib, cols, left, right, stride):
    import torch

    p = (left, right, stride)
    D, H = delay_hist(*p)
    T0, R = 12 * stride, 3 * stride
    host = [clip(cols, T0 + 40 * stride, seed=80 + b) for b in range(5)]
    s = [torch.from_numpy(h.copy()).cuda() for h in host]
    base = torch.zeros((12, H * cols + 1), device="cuda")
    _stream_call(torch, sslib, [s[b][:T0] for b in range(4)], [7, 0, 1, 2], base, cols, p)  # full histories
    base[9] = base[7]  # the same stream state in another slot
    mine = s[0][T0:T0 + R]
    other = [s[b][T0:T0 + r * stride] for b, r in ((1, 1), (2, 37), (3, 2), (4, 9))]
    empty = mine[:0]
    layouts = {"first": ([mine] + other, [7, 0, 1, 2, 3]),
               "last": (other + [mine], [0, 1, 2, 3, 7]),
               "other_slot": (other[:2] + [mine] + other[2:], [0, 1, 9, 2, 3]),
               "between_empties": (other[:2] + [empty, mine, empty] + other[2:], [0, 1, 10, 7, 11, 2, 3]),
               "alone": ([mine], [7])}
    rows, states, tails = {}, {}, {}
    for key, (chunks, slots) in layouts.items():
        pool = base.clone()
        out, ro = _stream_call(torch, sslib, chunks, slots, pool, cols, p)
        slot = 9 if key == "other_slot" else 7
        i = slots.index(slot)
        rows[key] = out[ro[i] // stride:ro[i + 1] // stride].clone()
        states[key] = pool[slot].clone()
        fl = [v for v in slots if v not in (10, 11)][::-1]
        tail = _flush_call(torch, sslib, fl, pool, cols, p)
        j = fl.index(slot)
        tails[key] = tail[j * D:(j + 1) * D].clone()
    m = StreamModel(cols, *p)
    m.push(host[0][:T0])
    assert np.array_equal(u32(_host(rows["alone"])), u32(m.push(host[0][T0:T0 + R])))
    assert np.array_equal(u32(_host(states["alone"])), u32(m.pool_row()))
    assert np.array_equal(u32(_host(tails["alone"])), u32(m.flush()))
    for key in layouts:
        assert torch.equal(_bits(rows[key]), _bits(rows["alone"])), key
        assert torch.equal(_bits(states[key]), _bits(states["alone"])), key
        assert torch.equal(_bits(tails[key]), _bits(tails["alone"])), key


def test_zeroing_a_pool_row_and_flush_both_give_a_fresh_stream(sslib):
    import torch

    cols, p = 33, (4, 7, 3)
    D, H = delay_hist(*p)
    host = [clip(cols, 30 * 3, seed=120 + b) for b in range(3)]
    s = [torch.from_numpy(h.copy()).cuda() for h in host]
    pool = torch.zeros((5, H * cols + 1), device="cuda")
    _stream_call(torch, sslib, [s[0][:45], s[1][:45], s[2][:45]], [2, 4, 0], pool, cols, p)
    pool[2] = 0.0                                      # reset mid-stream
    _flush_call(torch, sslib, [4], pool, cols, p)      # flushed mid-stream
    out, ro = _stream_call(torch, sslib, [s[0][45:], s[1][45:], s[2][45:]], [2, 4, 0], pool, cols, p)
    out = _host(out)
    for i in (0, 1):
        fresh = StreamModel(cols, *p).push(host[i][45:])
        assert np.array_equal(u32(out[ro[i] // 3:ro[i + 1] // 3]), u32(fresh)), i
        assert not u32(out[ro[i] // 3:ro[i] // 3 + D]).any()
    cont = want(cols, 90, *p, seed=122)
    assert np.array_equal(u32(out[ro[2] // 3:ro[3] // 3]), u32(cont[15 - D:30 - D]))  # the untouched stream goes on


# the last entry of the call: (ro entries appended behind 9 periods, in rows for stride s; its slot; total_rows in periods; served)
LAST_ENTRY = {"good": (lambda s: [11 * s], 6, 11, True), "past_the_end": (lambda s: [11 * s], 6, 10, False),
              "reversed": (lambda s: [8 * s], 6, 11, False), "part_of_a_period": (lambda s: [10 * s - 1], 6, 11, False),
              "slot_past_the_pool": (lambda s: [11 * s], 8, 11, False), "slot_below_zero": (lambda s: [11 * s], -1, 11, False)}


@pytest.mark.parametrize("last", sorted(LAST_ENTRY))
@pytest.mark.parametrize("left,right,stride", [(0, 0, 3), (3, 3, 6), (4, 7, 3)])  # H = 0; D = 0 with left > 0; both > 0
def test_bad_pool_entries_are_contained(sslib, left, right, stride, last):
    """An entry that does not start at a period, is not whole periods, is reversed, ends past total_rows or names a slot outside the
    pool is skipped -- no row written, its pool row untouched -- in the interior and as the last entry; the good entries of the
    same call are what they are alone; nothing outside the blocks is touched."""
    import torch

    cols, P, s = 13, 8, stride
    p = (left, right, stride)
    D, H = delay_hist(*p)
    ocols = (left + 1 + right) * cols
    add, last_slot, total_periods, last_ok = LAST_ENTRY[last]
    #     e0 good | e1 not whole periods | e2 does not start at a period | e3 reversed | e4 good | e5 slot = P | e6 slot = -1 | e7 good
    ro = np.array([0, 2 * s, 3 * s + 1, 5 * s + 1, 4 * s, 6 * s, 7 * s, 8 * s, 9 * s] + add(s), np.int64)
    slots = [1, 0, 3, 4, 2, P, -1, 5, last_slot]
    good = {0: (0, 2 * s), 4: (4 * s, 6 * s), 7: (8 * s, 9 * s)}
    if last_ok:
        good[8] = (9 * s, 11 * s)
    total_rows = total_periods * s
    host = clip(cols, total_rows, seed=110)
    x_g = _fill(torch, (total_rows + 2 * GUARD, cols))
    x = x_g[GUARD:GUARD + total_rows]
    x.copy_(torch.from_numpy(host.copy()).cuda())
    x_before = x_g.clone()
    out_g = _fill(torch, (total_periods + 2 * GUARD, ocols))
    out = out_g[GUARD:GUARD + total_periods]
    pool_g = _fill(torch, (P + 2 * GUARD, H * cols + 1))
    pool = pool_g[GUARD:GUARD + P]
    pool.zero_()
    prime = [torch.from_numpy(clip(cols, 20 * s, seed=111 + r).copy()).cuda() for r in range(P)]
    _stream_call(torch, sslib, prime, list(range(P)), pool, cols, p)  # valid states everywhere
    before = pool.clone()

    def single(chunk, state_row):
        q = state_row[None, :].clone()
        o, _ = _stream_call(torch, sslib, [chunk], [0], q, cols, p)
        return o.clone(), q[0].clone()

    expect = {i: single(x[a:b], before[slots[i]]) for i, (a, b) in good.items()}
    rc = _stream_raw(torch, sslib, x, len(slots), torch.from_numpy(ro).cuda(), total_rows, torch.tensor(slots, dtype=torch.int32, device="cuda"), P,
                     cols, p, pool, out)
    assert rc == 0, sslib.ss_last_error_string()  # the tables are device data: the call itself cannot know
    torch.cuda.synchronize()
    written = np.zeros(total_periods, bool)
    for i, (a, b) in good.items():
        assert torch.equal(_bits(out[a // s:b // s]), _bits(expect[i][0])), i
        assert torch.equal(_bits(pool[slots[i]]), _bits(expect[i][1])), i
        m = StreamModel(cols, *p)
        m.push(clip(cols, 20 * s, seed=111 + slots[i]))
        assert np.array_equal(u32(_host(out[a // s:b // s])), u32(m.push(host[a:b]))), i
        written[a // s:b // s] = True
    assert _is_sentinel(out[torch.from_numpy(~written).cuda()])  # what the skipped entries claimed keeps the sentinel
    for r in set(range(P)) - {slots[i] for i in good}:
        assert torch.equal(_bits(pool[r]), _bits(before[r])), r
    assert _is_sentinel(out_g[:GUARD]) and _is_sentinel(out_g[GUARD + total_periods:])
    assert _is_sentinel(pool_g[:GUARD]) and _is_sentinel(pool_g[GUARD + P:])
    assert torch.equal(_bits(x_g), _bits(x_before))
    # the flush with slots outside the pool, interior and last: those entries' D rows keep the sentinel, the others are flushed
    fl_g = _fill(torch, (4 * D + 2 * GUARD, ocols))
    kept = pool.clone()
    d_sl = torch.tensor([2, P, 5, -1], dtype=torch.int32, device="cuda")
    rc = sslib.ss_splice_stream_flush_device(4, d_sl.data_ptr(), P, cols, *p, pool.data_ptr(), fl_g[GUARD:].data_ptr(), _stream())
    assert rc == 0, sslib.ss_last_error_string()
    torch.cuda.synchronize()
    fl = fl_g[GUARD:GUARD + 4 * D]
    for j, slot in ((0, 2), (2, 5)):
        m = StreamModel(cols, *p)
        m.hist = _host(kept[slot])[:-1].reshape(H, cols)[H - int(kept[slot][-1]):]
        assert np.array_equal(u32(_host(fl[j * D:(j + 1) * D])), u32(m.flush())), slot
        assert not _bits(pool[slot]).any()
    assert _is_sentinel(fl[D:2 * D]) and _is_sentinel(fl[3 * D:]) and _is_sentinel(fl_g[:GUARD]) and _is_sentinel(fl_g[GUARD + 4 * D:])
    for r in set(range(P)) - {2, 5}:
        assert torch.equal(_bits(pool[r]), _bits(kept[r])), r
    assert _is_sentinel(pool_g[:GUARD]) and _is_sentinel(pool_g[GUARD + P:])


@pytest.mark.parametrize("left,right,stride", [(0, 0, 3), (3, 3, 6), (4, 7, 3), (5, 5, 1)])
def test_bad_count_words_are_read_as_a_fresh_stream(sslib, left, right, stride):
    """Count words NaN, -1, 0.5, 1e9, H + 1 and inf over garbage history, in the interior and last: read as 0 whatever the history
    floats hold, beside one valid state."""
    import torch

    cols, P = 13, 8
    p = (left, right, stride)
    D, H = delay_hist(*p)
    words = [float("nan"), -1.0, 0.5, 1e9, float(H + 1), float("inf")]
    gen = torch.Generator(device="cuda")
    gen.manual_seed(9)
    pool_g = _fill(torch, (P + 2 * GUARD, H * cols + 1))
    pool = pool_g[GUARD:GUARD + P]
    pool.copy_(torch.randn((P, H * cols + 1), generator=gen, device="cuda") * 50)  # garbage history
    host = [clip(cols, 25 * stride, seed=140 + r) for r in range(P)]
    valid = StreamModel(cols, *p)
    valid.push(host[6][:20 * stride])
    pool[6] = torch.from_numpy(valid.pool_row()).cuda()
    for r, w in enumerate(words):
        pool[r, -1] = w
    entries = [0, 1, 2, 6, 3, 4, 5]  # the valid state in the interior, a bad word last
    periods = [2, 1, 5, 3, 4, 1, 2]
    chunks = [torch.from_numpy(host[r][20 * stride:(20 + k) * stride].copy()).cuda() for r, k in zip(entries, periods)]
    out, ro = _stream_call(torch, sslib, chunks, entries, pool, cols, p)
    for i, (r, k) in enumerate(zip(entries, periods)):
        m = valid if r == 6 else StreamModel(cols, *p)
        assert np.array_equal(u32(_host(out[ro[i] // stride:ro[i + 1] // stride])), u32(m.push(host[r][20 * stride:(20 + k) * stride]))), r
        assert np.array_equal(u32(_host(pool[r])), u32(m.pool_row())), r
    assert _is_sentinel(pool_g[:GUARD]) and _is_sentinel(pool_g[GUARD + P:])


@pytest.mark.parametrize("left,right,stride", [(5, 5, 1), (3, 3, 6), (4, 7, 3)])
def test_host_forms_and_python_front_equal_the_device_forms(ss, sslib, left, right, stride):
    import torch

    cols, P = 13, 9
    p = (left, right, stride)
    D, H = delay_hist(*p)
    len_, ocols = H * cols + 1, (left + 1 + right) * cols
    # packed: device form, host form, splice_packed on numpy and on tensors, splice of a matrix and of a batch, lfr
    lens = [0, 1, stride + 1, 2 * TILE * stride + 3, 7]
    clips = [clip(cols, T, seed=150 + i) for i, T in enumerate(lens)]
    dev, oo = _packed(torch, sslib, clips, cols, *p)
    block = np.concatenate(clips)
    ro = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    host = np.full((int(oo[-1]) + 1, ocols), -3.0, np.float32)
    assert sslib.ss_splice_packed(block.ctypes.data, len(lens), ro.ctypes.data, len(block), cols, *p, host.ctypes.data) == 0, sslib.ss_last_error_string()
    assert np.array_equal(u32(host[:-1]), u32(dev)) and (host[-1] == -3.0).all()
    got_np, oo_np = ss.splice_packed(block, ro, *p)
    got_t, oo_t = ss.splice_packed(torch.from_numpy(block).cuda(), torch.from_numpy(ro).cuda(), *p)
    assert isinstance(got_np, np.ndarray) and torch.is_tensor(got_t) and torch.is_tensor(oo_t) and oo_t.is_cuda
    assert np.array_equal(oo_np, oo) and np.array_equal(_host(oo_t), oo)
    assert np.array_equal(u32(got_np), u32(dev)) and np.array_equal(u32(_host(got_t)), u32(dev))
    one = ss.splice(torch.from_numpy(clips[3].copy()).cuda(), *p)
    assert np.array_equal(u32(_host(one)), u32(dev[oo[3]:oo[4]]))
    batch = ss.splice(np.stack([clips[4], clips[4][::-1]]), *p)
    assert batch.shape == (2, -(-7 // stride), ocols)
    assert np.array_equal(u32(batch[0]), u32(dev[oo[4]:oo[5]])) and np.array_equal(u32(batch[1]), u32(splice_ref(clips[4][::-1], *p)))
    m_lfr = left + 1 + right
    if left == (m_lfr - 1) // 2:
        assert np.array_equal(u32(ss.lfr(clips[3], m_lfr, stride)), u32(dev[oo[3]:oo[4]]))
        assert np.array_equal(u32(ss.lfr_packed(block, ro, m_lfr, stride)[0]), u32(dev))
    # the pool: three calls, then reset and flush
    hosts = [clip(cols, 60 * stride, seed=160 + b) for b in range(4)]
    s = [torch.from_numpy(h.copy()).cuda() for h in hosts]
    k = stride
    calls = [([s[0][:3 * k], s[1][:0], s[2][:40 * k]], [4, 1, 7]),
             ([s[2][40 * k:45 * k], s[0][3 * k:4 * k]], [7, 4]),
             ([s[1][:50 * k], s[0][4 * k:6 * k], s[3][:0]], [1, 4, 0])]
    pool_d = torch.zeros((P, len_), device="cuda")
    pool_h = np.zeros((P, len_), np.float32)
    m_np, m_t = ss.SpliceStreamPool(P, cols, *p), ss.SpliceStreamPool(P, cols, *p)
    seen = np.zeros(P, np.int64)
    for chunks, slots in calls:
        d, ro = _stream_call(torch, sslib, chunks, slots, pool_d, cols, p, slack=0)
        d = _host(d)
        R = int(ro[-1])
        xh = _host(torch.cat(chunks))
        outh = np.full((R // stride, ocols), -3.0, np.float32)
        sl = np.asarray(slots, np.int32)
        before = pool_h.copy()
        dup = np.full(len(slots), slots[0], np.int32)
        rc = sslib.ss_splice_stream_packed(xh.ctypes.data, len(slots), ro.ctypes.data, dup.ctypes.data, P, cols, *p, pool_h.ctypes.data, outh.ctypes.data)
        assert rc == 3 and b"entry 1" in sslib.ss_last_error_string()  # a slot named twice: rejected, nothing written
        assert np.array_equal(u32(pool_h), u32(before)) and (outh == -3.0).all()
        rc = sslib.ss_splice_stream_packed(xh.ctypes.data, len(slots), ro.ctypes.data, sl.ctypes.data, P, cols, *p, pool_h.ctypes.data, outh.ctypes.data)
        assert rc == 0, sslib.ss_last_error_string()
        assert np.array_equal(u32(outh), u32(d)) and np.array_equal(u32(pool_h), u32(_host(pool_d)))
        changed = {int(r) for r in np.flatnonzero((u32(pool_h) != u32(before)).any(axis=1))}
        assert changed <= {int(v) for v, c in zip(slots, chunks) if c.shape[0] > 0}  # only named rows with new rows moved
        got_np, got_t = m_np(xh, ro, slots), m_t(torch.cat(chunks), ro, slots)
        assert isinstance(got_np, np.ndarray) and torch.is_tensor(got_t)
        assert np.array_equal(u32(got_np), u32(d)) and np.array_equal(u32(_host(got_t)), u32(d))
        seen[sl] += np.diff(ro)
        assert np.array_equal(m_np.rows_seen, seen) and np.array_equal(m_t.rows_seen, seen)
    torch.cuda.synchronize()
    assert m_np.state.shape == (P, len_) and np.array_equal(u32(m_np.state), u32(pool_h)) and torch.equal(_bits(m_t.state), _bits(pool_d))
    with pytest.raises(ValueError):
        m_np(torch.cat(calls[1][0]), [0, 5 * k, 6 * k], [7, 4])  # the pool lives on the host
    for m in (m_np, m_t):
        m.reset(slots=[7])
        st = m.state if isinstance(m.state, np.ndarray) else _host(m.state)
        assert not st[7].any() and np.array_equal(u32(st[4]), u32(pool_h[4])) and m.rows_seen[7] == 0 and m.rows_seen[4] == seen[4]
    pool_d[7] = 0.0
    pool_h[7] = 0.0
    seen[7] = 0
    fl = [1, 7, 4, 3]  # a long stream, a fresh one, a short one (6 periods) and a never-named one
    tail_d = _host(_flush_call(torch, sslib, fl, pool_d, cols, p))
    tail_h = np.full((len(fl) * D, ocols), -3.0, np.float32)
    before = pool_h.copy()
    rc = sslib.ss_splice_stream_flush(len(fl), np.array([1, 7, 1, 3], np.int32).ctypes.data, P, cols, *p, pool_h.ctypes.data, tail_h.ctypes.data)
    assert rc == 3 and b"entry 2" in sslib.ss_last_error_string() and np.array_equal(u32(pool_h), u32(before)) and (tail_h == -3.0).all()
    rc = sslib.ss_splice_stream_flush(len(fl), np.array(fl, np.int32).ctypes.data, P, cols, *p, pool_h.ctypes.data, tail_h.ctypes.data if D else None)
    assert rc == 0, sslib.ss_last_error_string()
    assert np.array_equal(u32(tail_h), u32(tail_d)) and np.array_equal(u32(pool_h), u32(_host(pool_d))) and not pool_h[fl].any()
    whole1 = splice_ref(hosts[1][:50 * k], *p)
    assert np.array_equal(u32(tail_d[:D]), u32(whole1[50 - D:]))
    assert not u32(tail_d[D:2 * D]).any() and not u32(tail_d[3 * D:]).any()  # fresh streams flush to zero rows
    t_np, t_t = m_np.flush(fl), m_t.flush(fl)
    assert isinstance(t_np, np.ndarray) and torch.is_tensor(t_t)
    assert np.array_equal(u32(t_np), u32(tail_d)) and np.array_equal(u32(_host(t_t)), u32(tail_d))
    seen[fl] = 0
    assert np.array_equal(m_np.rows_seen, seen) and np.array_equal(m_t.rows_seen, seen)
    assert np.array_equal(u32(m_np.state), u32(pool_h)) and torch.equal(_bits(m_t.state), _bits(pool_d))


def _captured_node_kinds(torch, record):
    """the node kinds of what `record(stream)` puts on a capturing stream (the HIP runtime this process has loaded: torch's)"""
    with open("/proc/self/maps") as f:
        paths = {line.split()[-1] for line in f if "libamdhip64" in line}
    assert paths, "no HIP runtime loaded"
    hip = C.CDLL(sorted(paths)[0])
    hip.hipGraphGetNodes.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_size_t)]
    hip.hipGraphNodeGetType.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
    raw, graph = torch.cuda.Stream(), C.c_void_p()
    assert hip.hipStreamBeginCapture(C.c_void_p(raw.cuda_stream), 2) == 0  # hipStreamCaptureModeRelaxed
    try:
        assert record(raw.cuda_stream) == 0
    finally:
        assert hip.hipStreamEndCapture(C.c_void_p(raw.cuda_stream), C.byref(graph)) == 0
    n_nodes = C.c_size_t()
    assert hip.hipGraphGetNodes(graph, None, C.byref(n_nodes)) == 0
    nodes = (C.c_void_p * n_nodes.value)()
    assert hip.hipGraphGetNodes(graph, nodes, C.byref(n_nodes)) == 0
    kinds = []
    for node in nodes:
        kind = C.c_int(-1)
        assert hip.hipGraphNodeGetType(node, C.byref(kind)) == 0
        kinds.append(kind.value)
    assert hip.hipGraphDestroy(graph) == 0
    return kinds


def test_graph_of_the_kaldi_pool_the_normalisation_and_the_splice_on_the_same_tables(ss, sslib):
    """ss_kstream_fbank_packed_device -> ss_cmvn_stream_packed_device -> ss_splice_stream_packed_device on one set of row_offsets /
    slots, captured once and replayed over three table contents (entries of 0 / 3 / 6 hops, stride 3): the eager calls' bits, and the
    splice call alone is one kernel node."""
    import torch

    from test_kaldi_cpu import gpu_case_signal
    from test_kaldi_stream import FBANK, KINDS, Rig

    rig = Rig(ss, sslib, False, **FBANK)
    N, CAP, P, sh, WIN, p = 6, 30, 10, rig.shift, 7, (4, 7, 3)
    M, stride = rig.cols, p[2]
    D, H = delay_hist(*p)
    ocols = (p[0] + 1 + p[1]) * M
    x = torch.zeros(CAP * sh, device="cuda")
    d_so, d_ro = torch.zeros(N + 1, dtype=torch.int64, device="cuda"), torch.zeros(N + 1, dtype=torch.int64, device="cuda")
    d_sl = torch.arange(N, dtype=torch.int32, device="cuda")
    feat, en = rig.outs(torch, CAP)
    norm = torch.zeros((CAP, M), device="cuda")
    out = _fill(torch, (CAP // stride, ocols))
    sizes = (rig.S, (WIN - 1) * M + 1, H * M + 1)
    pools_g = [torch.zeros((P, n), device="cuda") for n in sizes]
    pools_e = [torch.zeros((P, n), device="cuda") for n in sizes]

    def chain(pools, stream=None):
        stream = stream if stream is not None else torch.cuda.current_stream().cuda_stream
        assert rig.raw(torch, x, d_so, d_ro, CAP, d_sl, P, pools[0], feat, en, stream=stream) == 0, sslib.ss_last_error_string()
        rc = sslib.ss_cmvn_stream_packed_device(feat.data_ptr(), N, d_ro.data_ptr(), CAP, d_sl.data_ptr(), P, M, WIN, 1, pools[1].data_ptr(),
                                                norm.data_ptr(), C.c_void_p(stream))
        assert rc == 0, sslib.ss_last_error_string()
        assert _stream_raw(torch, sslib, norm, N, d_ro, CAP, d_sl, P, M, p, pools[2], out, stream=stream) == 0, sslib.ss_last_error_string()

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up outside the capture (the zero tables are N entries without rows)
        chain([q.clone() for q in pools_g], stream=side.cuda_stream)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for n in (N, 2):  # the splice call alone: ONE kernel node, for 2 entries as for 6
        kinds = _captured_node_kinds(torch, lambda st, n=n: _stream_raw(torch, sslib, norm, n, d_ro, CAP, d_sl, P, M, p, pools_g[2], out, stream=st))
        assert kinds == [0], (n, kinds)  # hipGraphNodeTypeKernel
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        chain(pools_g)
    rng = np.random.default_rng(44)
    for k, hops in enumerate(([3, 0, 6, 3, 0, 6], [6, 6, 0, 3, 3, 0], [0, 3, 3, 6, 6, 3])):
        slots = rng.permutation(P)[:N].astype(np.int32)
        so = np.concatenate([[0], np.cumsum(np.asarray(hops) * sh)]).astype(np.int64)
        ro = so // sh
        xs = torch.from_numpy(gpu_case_signal(60 + k, int(so[-1]), KINDS[k])).cuda()
        x.zero_()
        x[:xs.numel()] = xs
        d_so.copy_(torch.from_numpy(so))
        d_ro.copy_(torch.from_numpy(ro))
        d_sl.copy_(torch.from_numpy(slots))
        for t in (feat, norm, out):
            t.view(torch.int32).fill_(int(SENTINEL) - (1 << 32))
        chain(pools_e)  # eager, on the other pools
        torch.cuda.synchronize()
        eager = [t.clone() for t in (feat, norm, out)]
        for t in (feat, norm, out):
            t.view(torch.int32).fill_(int(SENTINEL) - (1 << 32))
        g.replay()
        torch.cuda.synchronize()
        R = int(ro[-1])
        assert R > 0 and not (_bits(out[:R // stride]) == int(SENTINEL) - (1 << 32)).any()
        for got_t, want_t in zip((feat, norm, out), eager):
            assert torch.equal(_bits(got_t), _bits(want_t)), k
        assert _is_sentinel(out[R // stride:])  # rows past the last entry are left alone
        for a, b in zip(pools_g, pools_e):
            assert torch.equal(_bits(a), _bits(b)), k
        # and the splice rows are the model's on the normalised rows of this tick
        if k == 0:
            nh = _host(norm)
            for i, h in enumerate(hops):
                fresh = StreamModel(M, *p).push(nh[ro[i]:ro[i + 1]])
                assert np.array_equal(u32(_host(out[ro[i] // stride:ro[i + 1] // stride])), u32(fresh)), i
    assert rig.status() == 0


def test_chain_of_the_python_pools_equals_the_stages_fed_the_dense_rows(ss):
    """KaldiFbankStreamPool -> CmvnStreamPool -> SpliceStreamPool on one set of row_offsets / slots (entries of 0 / 3 / 6 hops, stride
    3), new streams primed as documented: the result equals the two side stages fed the dense call's rows, and with the flush it is
    splice of the whole normalised clip."""
    import torch

    from test_kaldi_cpu import gpu_case_signal
    from test_kaldi_stream import KINDS

    M, sh, P, p = 23, 160, 8, (4, 7, 3)
    D, _ = delay_hist(*p)
    slots = [5, 0, 7, 2]
    calls = ([3, 0, 6, 3], [6, 3, 0, 3], [0, 6, 3, 6])
    totals = [sum(c[i] for c in calls) for i in range(4)]
    kpool = ss.KaldiFbankStreamPool(P, num_mel_bins=M)
    KD = kpool.delay_rows
    cm_a, cm_b = ss.CmvnStreamPool(P, M, win_size=5), ss.CmvnStreamPool(P, M, win_size=5)
    sp_a, sp_b = ss.SpliceStreamPool(P, M, *p), ss.SpliceStreamPool(P, M, *p)
    streams = [torch.from_numpy(gpu_case_signal(20 + i, (KD + k) * sh, KINDS[i % 3])).cuda() for i, k in enumerate(totals)]
    kpool([s[:KD * sh] for s in streams], None, slots)  # priming: the first KD hops go through a call whose rows are discarded
    at = [KD * sh] * 4
    dense = [ss.kaldi_fbank(s, num_mel_bins=M) for s in streams]
    done = [0] * 4
    got, normed = [[] for _ in range(4)], [[] for _ in range(4)]
    for hops in calls:
        chunks = [s[a:a + h * sh] for s, a, h in zip(streams, at, hops)]
        at = [a + h * sh for a, h in zip(at, hops)]
        rows, ro = kpool(chunks, None, slots)
        out = sp_a(cm_a(rows, ro, slots), ro, slots)
        want_rows = torch.cat([dense[i][done[i]:done[i] + h] for i, h in enumerate(hops)])
        done = [d + h for d, h in zip(done, hops)]
        assert torch.equal(rows, want_rows)
        nb = cm_b(want_rows, ro, slots)
        assert torch.equal(_bits(out), _bits(sp_b(nb, ro, slots)))
        ro = np.asarray(ro.cpu() if torch.is_tensor(ro) else ro)
        for i in range(4):
            got[i].append(out[ro[i] // 3:ro[i + 1] // 3])
            normed[i].append(nb[ro[i]:ro[i + 1]])
    tail = sp_a.flush(slots)
    for i in range(4):
        rows = _host(torch.cat(got[i] + [tail[i * D:(i + 1) * D]]))
        assert np.array_equal(u32(rows[D:]), u32(splice_ref(_host(torch.cat(normed[i])), *p))), i
