"""Energy VAD and voiced-row selection on the device: ss_vad_energy_packed* and ss_select_rows_packed* on packed clips,
ss_vad_energy_stream_packed* / ss_vad_energy_stream_flush* over a pool of stream states, and the Python front's vad_energy,
vad_energy_packed, select_rows, select_rows_packed and VadEnergyStreamPool.

Every comparison is exact: mask bytes and counts against the numpy restatement of the header (tests/vad_model.py), selected rows on
uint32 views (the selection copies bits; the inputs are salted with NaNs of distinct payloads, -0.0, +-inf and denormals).  Outputs sit
between guard regions of a sentinel that no result holds.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from splice_model import SENTINEL, clip, u32
from vad_model import KALDI_DEFAULT, MASK_SENTINEL, PARAMS, XVECTOR, VadStreamModel, causal_ref, energies, feature_clip, select_ref, vad_ref

pytestmark = pytest.mark.gpu

TILE = 256        # kVadTile / kSelTile, mfcc-rust_amd/csrc/ss_vad.hip: "constexpr unsigned kSelTile = 256;  // rows per tile"
SPLIT_ROWS = 2048  # kVadSplitRows: a clip gets one workgroup per 2048 rows
SPLIT_ALL = 8192  # packed_split, mfcc-rust_amd/csrc/ss_device.h: "want = std::max<unsigned long long>(1, 8192 / n_clips)"
GUARD = 64
ISENT = int(SENTINEL) - (1 << 32)


def _fill(torch, shape):
    return torch.full(shape, ISENT, dtype=torch.int32, device="cuda").view(torch.float32)


def _bytes(torch, n):
    return torch.full((n,), MASK_SENTINEL, dtype=torch.uint8, device="cuda")


def _bits(t):
    import torch

    return t.contiguous().view(torch.int32)


def _is_sentinel(t):
    return bool((_bits(t) == ISENT).all())


def _host(t):
    return t.cpu().numpy()


def _stream():
    import torch

    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _table(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


@functools.lru_cache(maxsize=None)
def _want_mask(T, seed, params):
    """vad_ref of energies(T, seed) (the decision looks at nothing else), computed once"""
    w = vad_ref(energies(T, seed)[:, None], 0, *params)
    w.setflags(write=False)
    return w


def _vad_raw(torch, lib, x, n, d_off, total, cols, col, params, mask, counts, stream=None):
    thr, scale, L, p = params
    return lib.ss_vad_energy_packed_device(x.data_ptr(), n, d_off.data_ptr(), total, cols, col, thr, scale, L, p, mask.data_ptr(),
                                           counts.data_ptr() if counts is not None else None, stream if stream is not None else _stream())


def _vad(torch, lib, clips, cols, col, params, empties=0):
    """ss_vad_energy_packed_device on a list of host clips, `empties` clips without rows behind them; mask and counts sit between
    guards.  -> (mask [sum T] , counts [n]) on the host"""
    lens = [c.shape[0] for c in clips] + [0] * empties
    off = _table(lens)
    R, n = int(off[-1]), len(lens)
    x = torch.from_numpy(np.concatenate(list(clips) + [np.zeros((1, cols), np.float32)])).cuda()
    mask = _bytes(torch, R + 2 * GUARD)
    counts = torch.full((n + 2 * GUARD,), -77, dtype=torch.int64, device="cuda")
    d_off = torch.from_numpy(off).cuda()
    rc = _vad_raw(torch, lib, x, n, d_off, R, cols, col, params, mask[GUARD:], counts[GUARD:])
    assert rc == 0, lib.ss_last_error_string()
    torch.cuda.synchronize()
    assert (mask[:GUARD] == MASK_SENTINEL).all() and (mask[GUARD + R:] == MASK_SENTINEL).all()
    assert (counts[:GUARD] == -77).all() and (counts[GUARD + n:] == -77).all()
    assert np.array_equal(_host(d_off), off)
    return _host(mask[GUARD:GUARD + R]), _host(counts[GUARD:GUARD + n])


@pytest.mark.parametrize("params", PARAMS)
@pytest.mark.parametrize("cols,col", [(1, 0), (13, 0), (13, 12), (80, 0), (80, 79)])
def test_packed_vad_is_the_model_byte_for_byte(sslib, cols, col, params):
    """One block of the lengths around the parameters, around the 32-row chunks of the mean, around a workgroup's share of 2048 rows and
    a clip of more than three shares -- once padded with clips without rows to SPLIT_ALL + 1 clips (one workgroup per clip, which walks
    every tile), once as it is (the long clips shared among workgroups)."""
    import torch

    L = params[2]
    lens = [0, 1, 2, L, L + 1, 2 * L + 1, 31, 32, 33, TILE - 1, TILE, TILE + 1, SPLIT_ROWS - 1, SPLIT_ROWS, SPLIT_ROWS + 1, 3 * SPLIT_ROWS + 463]
    clips = [feature_clip(cols, T, col, seed=i) for i, T in enumerate(lens)]
    off = _table(lens)
    for empties in (SPLIT_ALL + 1 - len(lens), 0):
        mask, counts = _vad(torch, sslib, clips, cols, col, params, empties=empties)
        assert set(np.unique(mask)) <= {0, 1}
        for i, T in enumerate(lens):
            w = _want_mask(T, i, params)
            g = mask[off[i]:off[i + 1]]
            bad = np.flatnonzero(g != w)
            assert bad.size == 0, (empties, T, bad[:8])
            assert counts[i] == int(w.sum()), (empties, T)
        assert not counts[len(lens):].any()  # a valid clip without rows: count 0
    assert 0 < sum(int(_want_mask(T, i, params).sum()) for i, T in enumerate(lens)) < off[-1]  # both decisions occur


def test_packed_vad_on_energies_that_straddle_the_threshold_and_without_counts(sslib):
    """Energies exactly on, one float below and one float above the threshold (scale 0: the threshold is the float itself), NaN and
    +-inf rows; and the call without a count table."""
    import torch

    thr = np.float32(5.0)
    e = np.array([thr, np.nextafter(thr, np.float32(9)), np.nextafter(thr, np.float32(0)), np.nan, np.inf, -np.inf, 5.5, 4.5] * 40, np.float32)
    x = np.stack([e, np.full_like(e, np.nan)], axis=1)
    for params in ((5.0, 0.0, 0, 0.6), (5.0, 0.0, 2, 0.5), (5.0, 0.5, 1, 0.5)):
        mask, counts = _vad(torch, sslib, [x, x[:37]], 2, 0, params)
        w = np.concatenate([vad_ref(x, 0, *params), vad_ref(x[:37], 0, *params)])
        assert np.array_equal(mask, w) and counts.tolist() == [int(w[:320].sum()), int(w[320:].sum())]
    assert vad_ref(x, 0, 5.0, 0.0, 0, 0.6)[:8].tolist() == [0, 1, 0, 0, 1, 0, 1, 0] and not vad_ref(x, 0, 5.0, 0.5, 1, 0.5).any()  # a NaN mean
    d = torch.from_numpy(x).cuda()
    mask = _bytes(torch, 320 + 2 * GUARD)
    d_off = torch.tensor([0, 100, 320], dtype=torch.int64, device="cuda")
    assert _vad_raw(torch, sslib, d, 2, d_off, 320, 2, 0, XVECTOR[:1] + (0.0,) + XVECTOR[2:], mask[GUARD:], None) == 0
    torch.cuda.synchronize()
    p = (XVECTOR[0], 0.0) + XVECTOR[2:]
    assert np.array_equal(_host(mask[GUARD:-GUARD]), np.concatenate([vad_ref(x[:100], 0, *p), vad_ref(x[100:], 0, *p)]))
    assert (mask[:GUARD] == MASK_SENTINEL).all() and (mask[-GUARD:] == MASK_SENTINEL).all()


def test_packed_vad_on_real_log_energy_rows(ss, sslib):
    """Rows of ss_kaldi_mfcc with use_energy (column 0 is the frame's log energy) of a signal with loud and quiet stretches."""
    import torch

    from test_kaldi_cpu import gpu_case_signal

    n = 16000 * 4
    env = np.repeat(np.where(np.random.default_rng(3).random(n // 1600 + 1) < 0.5, 1.0, 1e-3), 1600)[:n].astype(np.float32)
    sig = gpu_case_signal(5, n, "int16") * env
    feat = ss.kaldi_mfcc(torch.from_numpy(sig).cuda(), use_energy=True)
    rows = _host(feat)
    assert rows.shape == (398, 13)
    clips = [rows[:150], rows[150:151], rows[151:]]
    off = _table([len(c) for c in clips])
    for params in (KALDI_DEFAULT, XVECTOR):
        mask, counts = _vad(torch, sslib, clips, 13, 0, params)
        w = np.concatenate([vad_ref(c, 0, *params) for c in clips])
        assert np.array_equal(mask, w) and counts.tolist() == [int(w[off[i]:off[i + 1]].sum()) for i in range(3)]
        assert 0 < w.sum() < len(w)  # both decisions occur on such a signal


@pytest.mark.parametrize("cols,col,params", [(13, 0, XVECTOR), (80, 79, KALDI_DEFAULT), (1, 0, PARAMS[4])])
def test_a_clips_mask_does_not_depend_on_its_place(sslib, cols, col, params):
    """The same clip (more than two shares: workgroups share it here) in other places and behind other neighbours."""
    import torch

    T = 2 * SPLIT_ROWS + 300
    mine = feature_clip(cols, T, col, seed=40)
    a, b, c = feature_clip(cols, 7, col, seed=41), feature_clip(cols, 300, col, seed=42, centre=50.0), feature_clip(cols, 1, col, seed=43)
    w = _want_mask(T, 40, params)
    for clips, i in (([mine, a, b], 0), ([a, b, mine], 2), ([b, c, mine[:0], mine, a], 3), ([mine], 0)):
        mask, counts = _vad(torch, sslib, clips, cols, col, params)
        off = _table([len(k) for k in clips])
        assert np.array_equal(mask[off[i]:off[i + 1]], w) and counts[i] == int(w.sum()), i


# a table over a block of 45 rows: clips (0, 9) and (9, 9) are served, (9, 5) is reversed, (5, 50) ends past the block, (50, 12) is
# reversed, (12, 20) is served, (20, -3) is reversed, (-3, 20) starts below 0, (20, 36) is served; then the last clip(s), from 36
BAD_TABLE = [0, 9, 9, 5, 50, 12, 20, -3, 20, 36]
BAD = {"reversed": [30], "negative": [-5, 3], "past_the_end": [51], "good": [45]}


@pytest.mark.parametrize("last", sorted(BAD))
def test_bad_vad_segments_are_contained(sslib, last):
    """Reversed, negative and past-the-end pairs in the interior and as the last clip: their mask bytes and count words keep the
    sentinel, the other clips are exact, vec (allocated exactly to size) and the table are unchanged."""
    import torch

    cols, params, total = 13, XVECTOR, 45
    off = np.array(BAD_TABLE + BAD[last], np.int64)
    n = len(off) - 1
    xh = feature_clip(cols, total, 0, seed=50)
    x = torch.from_numpy(xh.copy()).cuda()
    mask, counts = _bytes(torch, total + 2 * GUARD), torch.full((n + 2 * GUARD,), -77, dtype=torch.int64, device="cuda")
    d_off = torch.from_numpy(off).cuda()
    assert _vad_raw(torch, sslib, x, n, d_off, total, cols, 0, params, mask[GUARD:], counts[GUARD:]) == 0
    torch.cuda.synchronize()
    want = np.full(total, MASK_SENTINEL, np.uint8)
    want_counts = np.full(n, -77, np.int64)
    for b in range(n):
        lo, hi = int(off[b]), int(off[b + 1])
        if 0 <= lo <= hi <= total:
            want[lo:hi] = vad_ref(xh[lo:hi], 0, *params)
            want_counts[b] = int(want[lo:hi].sum())
    assert (want_counts == -77).sum() >= 5 and want_counts[1] == 0 and (want[9:12] == MASK_SENTINEL).all()
    assert np.array_equal(_host(mask[GUARD:-GUARD]), want) and np.array_equal(_host(counts[GUARD:-GUARD]), want_counts)
    assert (mask[:GUARD] == MASK_SENTINEL).all() and (mask[-GUARD:] == MASK_SENTINEL).all()
    assert (counts[:GUARD] == -77).all() and (counts[-GUARD:] == -77).all()
    assert np.array_equal(u32(_host(x)), u32(xh)) and np.array_equal(_host(d_off), off)


# ---- the selection ----

def _masks(R, seed):
    rng = np.random.default_rng(seed)
    alt = (np.arange(R) % 2).astype(np.uint8)
    out = {"zero": np.zeros(R, np.uint8), "one": np.ones(R, np.uint8), "alternating": alt}
    for p in (0.12, 0.5, 0.9):
        out[f"random{p}"] = (rng.random(R) < p).astype(np.uint8)
    out["bytes_1_2_255"] = np.where(rng.random(R) < 0.5, rng.choice(np.array([1, 2, 255], np.uint8), R), 0).astype(np.uint8)
    return out


def _select_raw(torch, lib, x, n, d_ro, total, cols, mask, oo, out, stream=None):
    return lib.ss_select_rows_packed_device(x.data_ptr(), n, d_ro.data_ptr(), total, cols, mask.data_ptr(), oo.data_ptr(), out.data_ptr(),
                                            stream if stream is not None else _stream())


def _select(torch, lib, xh, ro, mask_h):
    """ss_select_rows_packed_device with out and the table between guards -> (the whole capacity of out as bits, oo) on the host"""
    R, cols, n = xh.shape[0], xh.shape[1], len(ro) - 1
    x = torch.from_numpy(np.array(xh)).cuda()  # (a copy: the cached clips are read-only)
    out = _fill(torch, (R + 2 * GUARD, cols))
    oo = torch.full((n + 1 + 2 * GUARD,), -77, dtype=torch.int64, device="cuda")
    d_ro, d_m = torch.from_numpy(np.asarray(ro, np.int64)).cuda(), torch.from_numpy(mask_h).cuda()
    rc = _select_raw(torch, lib, x, n, d_ro, R, cols, d_m, oo[GUARD:], out[GUARD:])
    assert rc == 0, lib.ss_last_error_string()
    torch.cuda.synchronize()
    assert _is_sentinel(out[:GUARD]) and _is_sentinel(out[GUARD + R:])
    assert (oo[:GUARD] == -77).all() and (oo[GUARD + n + 1:] == -77).all()
    assert np.array_equal(u32(_host(x)), u32(xh)) and np.array_equal(_host(d_m), mask_h) and np.array_equal(_host(d_ro), ro)
    return u32(_host(out[GUARD:GUARD + R])), _host(oo[GUARD:GUARD + n + 1])


@pytest.mark.parametrize("empties", [0, SPLIT_ALL + 1])
@pytest.mark.parametrize("cols", (1, 13, 33, 80))
def test_selection_is_numpy_bit_for_bit(sslib, cols, empties):
    """x[mask != 0] and cumsum(counts), for every kind of mask, on clips of the lengths around one tile of TILE rows and of several
    tiles -- as few clips (a clip's tiles shared among workgroups) and padded with clips without rows to more clips than one
    workgroup of the scan has lanes for (8193 and more).  Rows past oo[n] keep the sentinel."""
    import torch

    lens = [0, 1, 2, 3, TILE - 1, TILE, TILE + 1, 2 * TILE - 1, 2 * TILE + 1, 5, 4 * TILE + 77, 7]
    seq = lens[:6] + [0] * (empties // 2) + lens[6:] + [0] * (empties - empties // 2)
    assert empties == 0 or len(seq) - 1 > 8192
    ro = _table(seq)
    xh = np.concatenate([clip(cols, T, seed=i) for i, T in enumerate(lens)])
    phases = set()
    for kind, m in _masks(len(xh), 60 + cols).items():
        got, oo = _select(torch, sslib, xh, ro, m)
        w, woo = select_ref(xh, ro, m)
        assert np.array_equal(oo, woo), kind
        K = int(woo[-1])
        assert K == int((m != 0).sum())
        bad = np.flatnonzero((got[:K] != u32(w)).any(axis=1)) if K else np.zeros(0, int)
        assert bad.size == 0, (kind, bad[:8])
        assert (got[K:] == SENTINEL).all(), kind  # rows at and past oo[n] are left unwritten
        phases |= {int(o) * cols % 4 for o in woo[:-1]}
    if cols % 2:  # odd rows: the clips' outputs start at every 16-byte phase
        assert phases == {0, 1, 2, 3}


def test_a_clips_selected_rows_do_not_depend_on_its_place(sslib):
    import torch

    cols, T = 13, 3 * TILE + 41
    mine, m_mine = clip(cols, T, seed=70), _masks(T, 71)["random0.5"]
    w = u32(mine[m_mine != 0])
    a, b = clip(cols, 11, seed=72), clip(cols, 300, seed=73)
    starts = set()
    for front in ([], [a], [b, a], [b[:150], mine[:0]], [a[:5]]):  # every row in front is kept: the clip starts at 0, 11, 311, 150, 5
        clips, i = front + [mine, a], len(front)
        ro = _table([len(k) for k in clips])
        m = np.concatenate([m_mine if k is mine else np.ones(len(k), np.uint8) for k in clips])
        got, oo = _select(torch, sslib, np.concatenate(clips), ro, m)
        assert np.array_equal(got[oo[i]:oo[i + 1]], w), i
        starts.add(int(oo[i]) * cols % 4)
    assert starts == {0, 1, 2, 3}  # at every 16-byte phase


@pytest.mark.parametrize("last", sorted(BAD))
def test_bad_selection_segments_contribute_no_rows(sslib, last):
    import torch

    cols, total = 13, 45
    ro = np.array(BAD_TABLE + BAD[last], np.int64)
    n = len(ro) - 1
    xh = clip(cols, total, seed=80)
    m = _masks(total, 81)["random0.9"]
    got, oo = _select(torch, sslib, xh, ro, m)
    rows, counts = [], []
    for b in range(n):
        lo, hi = int(ro[b]), int(ro[b + 1])
        ok = 0 <= lo <= hi <= total
        keep = np.flatnonzero(m[lo:hi] != 0) + lo if ok else np.zeros(0, int)
        rows.append(xh[keep])
        counts.append(len(keep))
    assert counts.count(0) >= 6 and sum(counts) > 20 and np.array_equal(oo, np.concatenate([[0], np.cumsum(counts)]))
    K = int(oo[-1])
    assert np.array_equal(got[:K], u32(np.concatenate(rows))) and (got[K:] == SENTINEL).all()


def test_clips_that_overlap_cannot_outgrow_the_block(sslib):
    """A device table may name the same rows twice; the kept rows then number more than the block holds.  The table still counts them,
    the clips that would end past total_rows have no row written, nothing outside the block is touched."""
    import torch

    cols, total = 5, 40
    ro = np.array([0, 40, 0, 40, 10], np.int64)  # clips: all rows, (reversed), all rows again, (reversed)
    xh = clip(cols, total, seed=82)
    m = np.ones(total, np.uint8)
    got, oo = _select(torch, sslib, xh, ro, m)
    assert oo.tolist() == [0, 40, 40, 80, 80]
    assert np.array_equal(got, u32(xh))  # clip 0's rows; clip 2 (rows 40 .. 80 of a block of 40) was not written


def _node_kinds(torch, record):
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
        assert record(C.c_void_p(raw.cuda_stream)) == 0
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


KERNEL, MEMSET = 0, 2  # hipGraphNodeTypeKernel, hipGraphNodeTypeMemset


def test_the_chain_runs_without_a_host_sync_and_replays_as_a_graph(ss, sslib):
    """ss_vad_energy_packed_device -> ss_select_rows_packed_device -> ss_cmvn_packed_device on d_out_offsets with total_rows as the
    bound, captured once and replayed over three inputs: the graph's bits are the eager bits and numpy's selection followed by
    ss_cmvn_packed_device on the host-made table.  The selection alone is at most three kernel / memset nodes, for 2 clips as for 8193."""
    import torch

    cols, params = 13, XVECTOR
    lens = [300, 0, 1, 700, 45, TILE + 3]
    off = _table(lens)
    R, n = int(off[-1]), len(lens)
    x = torch.zeros((R, cols), device="cuda")
    d_off = torch.from_numpy(off).cuda()

    def buffers():
        return (_bytes(torch, R), torch.full((n,), -77, dtype=torch.int64, device="cuda"), torch.full((n + 1,), -77, dtype=torch.int64, device="cuda"),
                _fill(torch, (R, cols)), _fill(torch, (R, cols)))

    def chain(bufs, stream=None):
        mask, counts, oo, sel, norm = bufs
        st = stream if stream is not None else _stream()
        assert _vad_raw(torch, sslib, x, n, d_off, R, cols, 0, params, mask, counts, stream=st) == 0, sslib.ss_last_error_string()
        assert _select_raw(torch, sslib, x, n, d_off, R, cols, mask, oo, sel, stream=st) == 0, sslib.ss_last_error_string()
        assert sslib.ss_cmvn_packed_device(sel.data_ptr(), n, oo.data_ptr(), R, cols, 1, norm.data_ptr(), st) == 0, sslib.ss_last_error_string()

    g_bufs, e_bufs = buffers(), buffers()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up outside the capture
        chain(buffers(), stream=C.c_void_p(side.cuda_stream))
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    big = SPLIT_ALL + 1
    big_ro = torch.from_numpy(_table([5] * 40 + [0] * (big - 40))).cuda()
    big_oo = torch.zeros(big + 1, dtype=torch.int64, device="cuda")
    for n_clips, table, oo in ((2, d_off, g_bufs[2]), (big, big_ro, big_oo)):
        kinds = _node_kinds(torch, lambda st, k=n_clips, t=table, o=oo: _select_raw(torch, sslib, x, k, t, 200, cols, g_bufs[0], o, g_bufs[3], stream=st))
        assert 1 <= sum(k in (KERNEL, MEMSET) for k in kinds) <= 3, (n_clips, kinds)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        chain(g_bufs)
    for k in range(3):
        xh = np.concatenate([feature_clip(cols, T, 0, seed=90 + 10 * k + i) for i, T in enumerate(lens)])
        xh = np.where(np.isfinite(xh), xh, np.float32(1.5)).astype(np.float32)  # cmvn behind it is arithmetic: finite rows
        x.copy_(torch.from_numpy(xh))
        for bufs in (g_bufs, e_bufs):
            bufs[0].fill_(MASK_SENTINEL)
            bufs[1].fill_(-77)
            bufs[2].fill_(-77)
            for t in bufs[3:]:
                t.view(torch.int32).fill_(ISENT)
        chain(e_bufs)
        g.replay()
        torch.cuda.synchronize()
        for a, b in zip(g_bufs, e_bufs):
            assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), k
        mask = np.concatenate([vad_ref(xh[off[i]:off[i + 1]], 0, *params) for i in range(n)])
        sel, oo = select_ref(xh, off, mask)
        K = int(oo[-1])
        assert 0 < K < R and np.array_equal(_host(g_bufs[0]), mask) and np.array_equal(_host(g_bufs[2]), oo)
        assert np.array_equal(u32(_host(g_bufs[3][:K])), u32(sel)) and _is_sentinel(g_bufs[3][K:]) and _is_sentinel(g_bufs[4][K:])
        d_sel, ref = torch.from_numpy(sel).cuda(), torch.empty((K, cols), device="cuda")
        d_oo = torch.from_numpy(oo).cuda()
        assert sslib.ss_cmvn_packed_device(d_sel.data_ptr(), n, d_oo.data_ptr(), K, cols, 1, ref.data_ptr(), _stream()) == 0
        torch.cuda.synchronize()
        assert torch.equal(_bits(g_bufs[4][:K]), _bits(ref)), k


# ---- the pool ----

def _pool_raw(torch, lib, x, n, d_ro, total, d_sl, P, cols, col, params, pool, mask, stream=None):
    thr, scale, L, p = params
    return lib.ss_vad_energy_stream_packed_device(x.data_ptr(), n, d_ro.data_ptr(), total, d_sl.data_ptr(), P, cols, col, thr, scale, L, p,
                                                  pool.data_ptr(), mask.data_ptr(), stream if stream is not None else _stream())


def _flush_raw(torch, lib, n, d_sl, P, params, pool, mask, stream=None):
    thr, scale, L, p = params
    return lib.ss_vad_energy_stream_flush_device(n, d_sl.data_ptr(), P, thr, scale, L, p, pool.data_ptr(), mask.data_ptr(),
                                                 stream if stream is not None else _stream())


def _pool_call(torch, lib, entries, slots, P, cols, col, params, pool):
    """one call on a list of host entries -> the entries' bytes (a list), the mask between guards"""
    lens = [len(e) for e in entries]
    ro = _table(lens)
    R = int(ro[-1])
    x = torch.from_numpy(np.concatenate(list(entries) + [np.zeros((1, cols), np.float32)])).cuda()
    mask = _bytes(torch, R + 2 * GUARD)
    d_ro, d_sl = torch.from_numpy(ro).cuda(), torch.tensor(list(slots), dtype=torch.int32, device="cuda")
    rc = _pool_raw(torch, lib, x, len(lens), d_ro, R, d_sl, P, cols, col, params, pool, mask[GUARD:])
    assert rc == 0, lib.ss_last_error_string()
    torch.cuda.synchronize()
    assert (mask[:GUARD] == MASK_SENTINEL).all() and (mask[GUARD + R:] == MASK_SENTINEL).all()
    got = _host(mask[GUARD:GUARD + R])
    return [got[ro[i]:ro[i + 1]] for i in range(len(lens))]


def _pool_flush(torch, lib, slots, P, params, pool):
    L, n = params[2], len(slots)
    mask = _bytes(torch, n * L + 2 * GUARD)
    d_sl = torch.tensor(list(slots), dtype=torch.int32, device="cuda")
    assert _flush_raw(torch, lib, n, d_sl, P, params, pool, mask[GUARD:]) == 0, lib.ss_last_error_string()
    torch.cuda.synchronize()
    assert (mask[:GUARD] == MASK_SENTINEL).all() and (mask[GUARD + n * L:] == MASK_SENTINEL).all()
    got = _host(mask[GUARD:GUARD + n * L])
    return [got[i * L:(i + 1) * L] for i in range(n)]


STREAM_LENS = (0, 1, 2, 3, 5, 40, 257, 600, 4)  # nine streams


@pytest.mark.parametrize("params", [XVECTOR, (5.0, 0.0, 3, 0.6), KALDI_DEFAULT, (4.0, 0.5, 32, 0.3), (5.5, 0.0, 0, 0.5)])
def test_pool_over_three_cuts_equals_the_packed_call_and_the_model(sslib, params):
    """Nine streams in a pool of 16 rows, cut three ways into three calls (entries without rows, the entries in reversed order in the
    second call), then the flush in another order.  scale == 0: all bytes, the first L dropped, are ss_vad_energy_packed_device on the
    whole clips; scale != 0: the causal model's bytes.  The final pool rows agree between the cuts and with the model; rows of the pool
    that no entry names keep the sentinel; an entry without rows leaves its pool row bit for bit."""
    import torch

    cols, col, P = 13, 4, 16
    thr, scale, L, p = params
    slots = [11, 3, 0, 15, 7, 8, 2, 5, 12]
    streams = [feature_clip(cols, T, col, seed=100 + i) for i, T in enumerate(STREAM_LENS)]
    if scale == 0:
        whole, _ = _vad(torch, sslib, streams, cols, col, params)
        off = _table(STREAM_LENS)
        want = [whole[off[i]:off[i + 1]] for i in range(9)]
    else:
        want = [causal_ref(s[:, col], *params) for s in streams]
    rng = np.random.default_rng(7)
    finals = []
    for cut in range(3):
        pool = _fill(torch, (P, 2 * L + 4))
        pool[slots] = 0
        models = [VadStreamModel(col, *params) for _ in streams]
        got = [[] for _ in streams]
        marks = [sorted(rng.integers(0, T + 1, 2).tolist()) if cut else [T // 3, T // 2] for T in STREAM_LENS]
        for call in range(3):
            order = list(range(9))[::-1] if call == 1 else list(range(9))
            pieces = [streams[i][([0] + marks[i] + [len(streams[i])])[call]:([0] + marks[i] + [len(streams[i])])[call + 1]] for i in order]
            before = pool.clone()
            outs = _pool_call(torch, sslib, pieces, [slots[i] for i in order], P, cols, col, params, pool)
            for i, piece, o in zip(order, pieces, outs):
                assert np.array_equal(o, models[i].push(piece)), (cut, call, i)
                got[i].append(o)
                if len(piece) == 0:
                    assert torch.equal(_bits(pool[slots[i]]), _bits(before[slots[i]]))
                assert np.array_equal(u32(_host(pool[slots[i]])), u32(models[i].pool_row())), (cut, call, i)
        finals.append(_host(pool).copy())
        forder = [4, 0, 8, 1, 7, 2, 6, 3, 5]
        tails = _pool_flush(torch, sslib, [slots[i] for i in forder], P, params, pool)
        for i, tail in zip(forder, tails):
            assert np.array_equal(tail, models[i].flush()), (cut, i)
            allb = np.concatenate(got[i] + [tail])
            assert allb.shape == (STREAM_LENS[i] + L,) and not allb[:L].any()
            assert np.array_equal(allb[L:], want[i]), (cut, i)
        assert not _bits(pool[slots]).any()  # flushed: fresh streams
        rest = sorted(set(range(P)) - set(slots))
        assert _is_sentinel(pool[rest])
    assert np.array_equal(u32(finals[0]), u32(finals[1])) and np.array_equal(u32(finals[0]), u32(finals[2]))


def test_a_pool_entry_does_not_depend_on_its_place_slot_or_neighbours(sslib):
    import torch

    cols, col, P, params = 13, 0, 8, XVECTOR
    L = params[2]
    mine = feature_clip(cols, 300, col, seed=120)
    a, b = feature_clip(cols, 7, col, seed=121), feature_clip(cols, 50, col, seed=122, centre=60.0)
    ref = None
    for entries, i, slots in (([mine[200:], a, b], 0, [0, 1, 2]), ([a, b, mine[200:]], 2, [5, 6, 7]), ([b, mine[200:]], 1, [3, 0]), ([mine[200:]], 0, [4])):
        pool = torch.zeros((P, 2 * L + 4), device="cuda")
        first = _pool_call(torch, sslib, [mine[:200]], [slots[i]], P, cols, col, params, pool)[0]
        got = _pool_call(torch, sslib, entries, slots, P, cols, col, params, pool)[i]
        row = u32(_host(pool[slots[i]]))
        tail = _pool_flush(torch, sslib, [slots[i]], P, params, pool)[0]
        allb = np.concatenate([first, got, tail])
        if ref is None:
            ref = (allb, row)
            assert np.array_equal(allb[L:], causal_ref(mine[:, col], *params))
        assert np.array_equal(allb, ref[0]) and np.array_equal(row, ref[1])


def test_bad_entries_slots_and_count_words_are_contained(sslib):
    """Bad row pairs and slots outside the pool, interior and last, in the call and in the flush: no byte written, no pool row touched.
    A count word that is not an integer in [0, 2 L], or rows seen below the count, reads as a fresh stream, beside one valid state."""
    import torch

    cols, col, P, params = 13, 2, 6, XVECTOR
    L, total = params[2], 40
    xh = feature_clip(cols, total, col, seed=130)
    x = torch.from_numpy(xh.copy()).cuda()
    # entries: (0, 8) slot 1 served; (8, 5) reversed; (5, 12) slot -1; (12, -3) reversed; (-3, 0) starts below 0; (0, 20) slot 6, outside
    # the pool; (20, 33) slot 4 served; (33, 41) ends past the block, the last
    ro = np.array([0, 8, 5, 12, -3, 0, 20, 33, 41], np.int64)
    sl = np.array([1, 2, -1, 3, 0, 6, 4, 5], np.int32)
    n = len(sl)
    pool = _fill(torch, (P, 2 * L + 4))
    pool[[1, 4]] = 0
    mask = _bytes(torch, total + 2 * GUARD)
    d_ro, d_sl = torch.from_numpy(ro).cuda(), torch.from_numpy(sl).cuda()
    assert _pool_raw(torch, sslib, x, n, d_ro, total, d_sl, P, cols, col, params, pool, mask[GUARD:]) == 0
    torch.cuda.synchronize()
    want = np.full(total, MASK_SENTINEL, np.uint8)
    m1, m4 = VadStreamModel(col, *params), VadStreamModel(col, *params)
    want[20:33] = m4.push(xh[20:33])  # (entry 0's bytes 0 .. 8 lie under the skipped entries' ranges too: nobody else writes them)
    want[0:8] = m1.push(xh[0:8])
    assert np.array_equal(_host(mask[GUARD:-GUARD]), want)
    assert (mask[:GUARD] == MASK_SENTINEL).all() and (mask[-GUARD:] == MASK_SENTINEL).all()
    assert np.array_equal(u32(_host(pool[1])), u32(m1.pool_row())) and np.array_equal(u32(_host(pool[4])), u32(m4.pool_row()))
    assert _is_sentinel(pool[[0, 2, 3, 5]])
    assert np.array_equal(u32(_host(x)), u32(xh)) and np.array_equal(_host(d_ro), ro) and np.array_equal(_host(d_sl), sl)
    # the flush: slots outside the pool, interior and last
    fmask = _bytes(torch, 4 * L + 2 * GUARD)
    fsl = torch.tensor([1, -1, 4, 6], dtype=torch.int32, device="cuda")
    assert _flush_raw(torch, sslib, 4, fsl, P, params, pool, fmask[GUARD:]) == 0
    torch.cuda.synchronize()
    wantf = np.full(4 * L, MASK_SENTINEL, np.uint8)
    wantf[0:L], wantf[2 * L:3 * L] = m1.flush(), m4.flush()
    assert np.array_equal(_host(fmask[GUARD:-GUARD]), wantf) and (fmask[:GUARD] == MASK_SENTINEL).all() and (fmask[-GUARD:] == MASK_SENTINEL).all()
    assert not _bits(pool[[1, 4]]).any() and _is_sentinel(pool[[0, 2, 3, 5]])
    # bad count words, and rows seen below the count, beside one valid state (slot 0)
    good = VadStreamModel(col, *params)
    good.push(xh[:9])
    rows = np.tile(good.pool_row(), (P, 1))
    rows[1, -1], rows[2, -1], rows[3, -1], rows[4, -1] = 2 * L + 1, 1.5, np.nan, -1.0
    rows.view(np.uint32)[5, 2] = 2 * L - 1  # rows seen below the count 2 L
    pool = torch.from_numpy(rows).cuda()
    piece = xh[9:30]
    outs = _pool_call(torch, sslib, [piece] * P, list(range(P)), P, cols, col, params, pool)
    fresh = VadStreamModel(col, *params)
    wf, wg = fresh.push(piece), good.push(piece)
    assert not np.array_equal(u32(fresh.pool_row()), u32(good.pool_row()))
    assert np.array_equal(outs[0], wg) and np.array_equal(u32(_host(pool[0])), u32(good.pool_row()))
    for s in range(1, P):
        assert np.array_equal(outs[s], wf) and np.array_equal(u32(_host(pool[s])), u32(fresh.pool_row())), s


def test_zeroing_a_pool_row_and_the_flush_both_give_a_fresh_stream_and_the_call_is_one_kernel_node(sslib):
    import torch

    cols, col, P, params = 13, 0, 4, (5.0, 0.5, 2, 0.3)
    L = params[2]
    a, b = feature_clip(cols, 30, col, seed=140), feature_clip(cols, 25, col, seed=141)
    pool = torch.zeros((P, 2 * L + 4), device="cuda")
    _pool_call(torch, sslib, [a, a], [0, 1], P, cols, col, params, pool)
    pool[0] = 0
    _pool_flush(torch, sslib, [1], P, params, pool)
    outs = _pool_call(torch, sslib, [b, b, b], [0, 1, 2], P, cols, col, params, pool)
    m = VadStreamModel(col, *params)
    w = m.push(b)
    for s in range(3):
        assert np.array_equal(outs[s], w) and np.array_equal(u32(_host(pool[s])), u32(m.pool_row()))
    x = torch.from_numpy(np.concatenate([a, b])).cuda()
    mask = _bytes(torch, 55)
    d_sl = torch.tensor([2, 3, 0], dtype=torch.int32, device="cuda")
    for n, table in ((2, [0, 30, 55]), (3, [0, 30, 30, 55])):  # ONE kernel node, for two entries as for three
        d_ro = torch.tensor(table, dtype=torch.int64, device="cuda")
        kinds = _node_kinds(torch, lambda st, n=n, d_ro=d_ro: _pool_raw(torch, sslib, x, n, d_ro, 55, d_sl, P, cols, col, params, pool, mask, stream=st))
        assert kinds == [KERNEL], (n, kinds)
    kinds = _node_kinds(torch, lambda st: _flush_raw(torch, sslib, 3, d_sl, P, params, pool, mask, stream=st))
    assert kinds == [KERNEL], kinds


# ---- host forms and the Python front ----

def test_host_forms_and_the_python_front_equal_the_device_forms(ss, sslib):
    import torch

    cols, col, params = 13, 12, XVECTOR
    thr, scale, L, p = params
    lens = [40, 0, 300, 1, TILE + 9]
    off = _table(lens)
    clips = [feature_clip(cols, T, col, seed=150 + i) for i, T in enumerate(lens)]
    xh = np.concatenate(clips)
    R, n = len(xh), len(lens)
    mask_d, counts_d = _vad(torch, sslib, clips, cols, col, params)
    assert np.array_equal(mask_d, np.concatenate([vad_ref(c, col, *params) for c in clips]))
    # the C host form
    mask_h, counts_h = np.full(R, MASK_SENTINEL, np.uint8), np.full(n, -77, np.int64)
    assert sslib.ss_vad_energy_packed(xh.ctypes.data, n, off.ctypes.data, R, cols, col, thr, scale, L, p, mask_h.ctypes.data, counts_h.ctypes.data) == 0
    assert np.array_equal(mask_h, mask_d) and np.array_equal(counts_h, counts_d)
    # the Python front, numpy and tensors
    m_np, c_np = ss.vad_energy_packed(xh, off, col, *params)
    m_t, c_t = ss.vad_energy_packed(torch.from_numpy(xh).cuda(), torch.from_numpy(off).cuda(), col, *params)
    assert isinstance(m_np, np.ndarray) and m_np.dtype == np.uint8 and c_np.dtype == np.int64 and torch.is_tensor(m_t) and m_t.is_cuda
    assert np.array_equal(m_np, mask_d) and np.array_equal(c_np, counts_d) and np.array_equal(_host(m_t), mask_d) and np.array_equal(_host(c_t), counts_d)
    batch = np.stack([feature_clip(cols, 70, col, seed=160 + i) for i in range(6)]).reshape(2, 3, 70, cols)
    wb = np.stack([vad_ref(m, col, *params) for m in batch.reshape(6, 70, cols)]).reshape(2, 3, 70).astype(bool)
    b_np, b_t = ss.vad_energy(batch, col, *params), ss.vad_energy(torch.from_numpy(batch).cuda(), col, *params)
    assert b_np.dtype == bool and b_t.dtype == torch.bool and np.array_equal(b_np, wb) and np.array_equal(_host(b_t), wb)
    assert np.array_equal(ss.vad_energy(clips[2], col, *params), vad_ref(clips[2], col, *params).astype(bool))
    # the selection
    w, woo = select_ref(xh, off, mask_d)
    K = int(woo[-1])
    out_h, oo_h = np.full((R, cols), -5.0, np.float32), np.full(n + 1, -77, np.int64)
    assert sslib.ss_select_rows_packed(xh.ctypes.data, n, off.ctypes.data, R, cols, mask_d.ctypes.data, oo_h.ctypes.data, out_h.ctypes.data) == 0
    assert np.array_equal(oo_h, woo) and np.array_equal(u32(out_h[:K]), u32(w)) and (out_h[K:] == -5.0).all()
    s_np, o_np = ss.select_rows_packed(xh, off, mask_d)
    s_t, o_t = ss.select_rows_packed(torch.from_numpy(xh).cuda(), off, torch.from_numpy(mask_d).cuda())
    f_t, fo_t = ss.select_rows_packed(torch.from_numpy(xh).cuda(), torch.from_numpy(off).cuda(), torch.from_numpy(mask_d.astype(bool)).cuda(), trim=False)
    assert s_np.shape == (K, cols) and np.array_equal(u32(s_np), u32(w)) and np.array_equal(o_np, woo)
    assert s_t.shape == (K, cols) and np.array_equal(u32(_host(s_t)), u32(w)) and o_t.is_cuda and np.array_equal(_host(o_t), woo)
    assert f_t.shape == (R, cols) and np.array_equal(u32(_host(f_t[:K])), u32(w)) and np.array_equal(_host(fo_t), woo)
    assert np.array_equal(u32(ss.select_rows(clips[2], mask_d[off[2]:off[3]])), u32(clips[2][mask_d[off[2]:off[3]] != 0]))
    assert np.array_equal(u32(_host(ss.select_rows(torch.from_numpy(np.array(clips[2])).cuda(), mask_d[off[2]:off[3]].astype(bool)))),
                          u32(clips[2][mask_d[off[2]:off[3]] != 0]))
    # the pool: the C host forms and the class equal the device forms
    P, slots = 6, [4, 1, 5]
    pieces = [clips[0], clips[2][:0], clips[2][:100]]
    pool_d = torch.zeros((P, 2 * L + 4), device="cuda")
    outs_d = _pool_call(torch, sslib, pieces, slots, P, cols, col, params, pool_d)
    pool_h = np.zeros((P, 2 * L + 4), np.float32)
    ro = _table([len(k) for k in pieces])
    sl = np.array(slots, np.int32)
    xs = np.concatenate(pieces)
    got_h = np.full(len(xs), MASK_SENTINEL, np.uint8)
    assert sslib.ss_vad_energy_stream_packed(xs.ctypes.data, 3, ro.ctypes.data, sl.ctypes.data, P, cols, col, thr, scale, L, p, pool_h.ctypes.data,
                                             got_h.ctypes.data) == 0
    assert np.array_equal(got_h, np.concatenate(outs_d)) and np.array_equal(u32(pool_h), u32(_host(pool_d)))
    m_np, m_t = ss.VadEnergyStreamPool(P, cols, col, *params), ss.VadEnergyStreamPool(P, cols, col, *params)
    g_np, g_t = m_np(xs, ro, slots), m_t(torch.from_numpy(xs).cuda(), ro, slots)
    assert np.array_equal(g_np, got_h) and np.array_equal(_host(g_t), got_h) and g_t.dtype == torch.uint8
    seen = np.zeros(P, np.int64)
    seen[slots] = [40, 0, 100]
    assert np.array_equal(m_np.rows_seen, seen) and np.array_equal(m_t.rows_seen, seen)
    assert np.array_equal(u32(m_np.state), u32(pool_h)) and np.array_equal(u32(_host(m_t.state)), u32(pool_h))
    before = pool_h.copy()
    dup = np.array([1, 1, 4], np.int32)
    assert sslib.ss_vad_energy_stream_packed(xs.ctypes.data, 3, ro.ctypes.data, dup.ctypes.data, P, cols, col, thr, scale, L, p, pool_h.ctypes.data,
                                             got_h.ctypes.data) == 3 and b"named twice" in sslib.ss_last_error_string()
    assert np.array_equal(u32(pool_h), u32(before))  # a slot named twice: rejected with nothing written
    with pytest.raises(ValueError):
        m_np(xs, ro, [1, 1, 4])
    assert np.array_equal(m_np.rows_seen, seen)
    fl = [5, 4, 0]
    tails_d = np.concatenate(_pool_flush(torch, sslib, fl, P, params, pool_d))
    tail_h = np.full(3 * L, MASK_SENTINEL, np.uint8)
    fsl = np.array(fl, np.int32)
    assert sslib.ss_vad_energy_stream_flush(3, fsl.ctypes.data, P, thr, scale, L, p, pool_h.ctypes.data, tail_h.ctypes.data) == 0
    assert np.array_equal(tail_h, tails_d) and np.array_equal(u32(pool_h), u32(_host(pool_d))) and not pool_h[fl].any()
    t_np, t_t = m_np.flush(fl), m_t.flush(fl)
    assert np.array_equal(t_np, tails_d) and np.array_equal(_host(t_t), tails_d)
    seen[fl] = 0
    assert np.array_equal(m_np.rows_seen, seen) and np.array_equal(m_t.rows_seen, seen)
    m_t.reset(slots=[1])
    assert not _bits(m_t.state[1]).any()
