"""Position independence of every packed entry point on blocks past 2^32 elements and buffers past 2^32 samples.

The header lets total_rows, n_clips and cols each reach 2^31 and checks no product of them, and sample offsets are int64: a feature
block of more than 2^32 floats and a sample buffer of more than 2^32 samples are inside the domain of every call.  It also promises
that a clip's bits depend on the clip and the scalars only, not on where the clip sits.  Each test here runs the same five clips
twice -- alone in a small block (`want`) and behind filler that pushes them past element 2^32 of a big block (`got`) -- and compares
the tail bit for bit, with the lengths, counts, offset tables and pool rows that belong to the tail clips as integers.

Every buffer is allocated in full, so that an index truncated to 32 bits lands inside the allocation, at the wrong place, and shows
as a mismatch.  Only the tail of a big output is prefilled (NaN, or all-ones bytes) and only tails come back to the host.  The
shapes, and the conditions they meet (past 2^32, below 2^31, at most 40 GiB per case), are tests/large_blocks_model.py's and are
checked without a device by tests/test_large_blocks_cpu.py.  One object holds the big input blocks, one at a time: asking for
another frees the one before.  Every test starts by handing what the one before left in torch's caching allocator back to the
device, and ends by holding the peak the allocator reserved during it, plus what the library allocates for itself in that case
(large_blocks_model's library_bytes), to the 40 GiB: the cap is checked for the whole file, not assumed.

cmvnw with variance normalisation keeps a scratch block as large as the block; three distinct blocks past 2^32 elements would be
48 GiB, so that case passes out == vec.  The header does not offer an in-place cmvnw: this rests on the implementation, whose first
launch writes only the scratch block and whose second reads only the scratch block (ss_cmvnw_packed_device in csrc/ss_post.hip).
So the write path of the second launch into a distinct out block is not walked past element 2^32 here; the call without variance
walks the same kernel template's store into a distinct block.  The filler of the shared block is zeros and stays zeros under it
(a clip of zeros normalises to +0.0)."""
import contextlib
import ctypes as C
import gc
import time

import numpy as np
import pytest

import large_blocks_model as M

pytestmark = pytest.mark.gpu

NAN = float("nan")
ROWS_T = sum(M.TAIL_ROWS)
PCM_SCALE = 2.0 ** -15


@pytest.fixture(scope="module")
def torch():
    import torch

    assert torch.cuda.is_available()
    return torch


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class Blocks:
    """The big input blocks of the file: one f32 and one int16 sample buffer of BIG samples, one row block per column count, the
    wide block of the dense strides.  One is alive at a time."""

    def __init__(self, torch):
        self.torch, self.key, self.big, self.tails = torch, None, None, {}

    def drop(self):
        self.big = self.key = None
        gc.collect()
        self.torch.cuda.empty_cache()

    def _hold(self, key, make):
        if self.key != key:
            self.drop()
            self.big, self.key = make(), key
        return self.big

    def tail_rows(self, cols, square=False):
        """the five tail clips alone: the small block [ROWS_T * cols] (square: the squares, a power spectrum for power_to_db)"""
        k = (cols, square)
        if k not in self.tails:
            t = _dev(self.torch, M.tail_rows_block(cols).reshape(-1))
            self.tails[k] = t * t if square else t
        return self.tails[k]

    def rows(self, cols, square=False):
        """filler clips of zeros, then the tail clips; the tail is written afresh on every request (a test may have masked it)"""
        lay = M.CASES["cmvn"].filler["layout"]
        x = self._hold(("rows", cols), lambda: self.torch.zeros(lay.total_rows * cols, dtype=self.torch.float32, device="cuda"))
        x[lay.tail_row0 * cols:] = self.tail_rows(cols, square)
        return x

    def samples(self, i16):
        torch = self.torch

        def make():
            x = torch.zeros(M.BIG, dtype=torch.int16 if i16 else torch.float32, device="cuda")
            x[M.BIG - M.N_TAIL:] = _dev(torch, M.sample_tail_i16() if i16 else M.sample_tail())
            return x

        return self._hold(("samples", i16), make)

    def custom(self, key, make):
        return self._hold(key, make)


@pytest.fixture(scope="module")
def blocks(torch):
    b = Blocks(torch)
    yield b
    b.drop()


@contextlib.contextmanager
def _report(torch, case):
    """Every test prints where its first tail element lies and its wall time, pass or fail.  What the test before left cached goes
    back to the device first; afterwards the peak that torch reserved during the test, plus the library's own allocations of the
    case, must be inside the cap."""
    gc.collect()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    try:
        yield
        torch.cuda.synchronize()
    finally:
        reserved = torch.cuda.max_memory_reserved()
        where = ", ".join(f"{b.name}: element {b.tail} byte {b.tail_byte}" for b in case.blocks if b.role != "small")
        print(f"{case.name}: first tail element of {where}; model peak {case.peak_bytes / 2 ** 30:.1f} GiB, reserved {reserved / 2 ** 30:.1f} GiB "
              f"+ library {case.library_bytes / 2 ** 30:.1f} GiB; wall {time.perf_counter() - t0:.2f} s")
    assert reserved + case.library_bytes <= M.CAP_BYTES, (case.name, reserved, case.library_bytes)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _same(want, got, what, per_row=1):
    """bit for bit, naming the first element that differs"""
    w, g = _bits(want).reshape(-1), _bits(got).reshape(-1)
    assert w.shape == g.shape, (what, w.shape, g.shape)
    bad = np.flatnonzero(w != g)
    assert bad.size == 0, f"{what}: {bad.size} of {w.size} tail elements differ, the first at {bad[0]} (row {bad[0] // per_row}): want {w[bad[0]]:#x} got {g[bad[0]]:#x}"


def _ok(sslib, rc):
    assert rc == 0, sslib.ss_last_error_string()


def _row_pair(torch, sslib, blocks, case, cols, out_cols, call, square=False, out_dtype=None, fill=NAN, in_place=False):
    """call(vec, n_clips, offsets, total_rows, out) on the five tail clips alone and on filler + tail; the tail rows of out must be
    the same bits.  in_place: the big call gets out == vec.  Returns the tail as a host array."""
    lay = case.filler["layout"]
    out_dtype = out_dtype or torch.float32
    small = blocks.tail_rows(cols, square)
    soff, boff = _dev(torch, lay.small_offsets()), _dev(torch, lay.offsets())
    want = torch.full((ROWS_T * out_cols,), fill, dtype=out_dtype, device="cuda")
    _ok(sslib, call(small.data_ptr(), len(M.TAIL_ROWS), soff.data_ptr(), ROWS_T, want.data_ptr()))
    big = blocks.rows(cols, square)
    t0 = lay.tail_row0 * out_cols
    if in_place:
        got = big
    else:
        got = torch.empty(lay.total_rows * out_cols, dtype=out_dtype, device="cuda")
        got[t0:] = fill
    _ok(sslib, call(big.data_ptr(), lay.n_clips, boff.data_ptr(), lay.total_rows, got.data_ptr()))
    torch.cuda.synchronize()
    w, g = want.cpu().numpy(), got[t0:].cpu().numpy()
    del got, big
    if out_dtype == torch.float32:
        assert not np.isnan(w).any(), case.name
    _same(w, g, case.name, out_cols)
    return w


# ---- section 2: the one-shot packed calls ----

@pytest.mark.parametrize("variance", [0, 1], ids=["mean", "var"])
def test_cmvn(torch, sslib, blocks, variance):
    case = M.CASES["cmvn_var" if variance else "cmvn"]
    with _report(torch, case):
        _row_pair(torch, sslib, blocks, case, 39, 39, lambda v, n, off, total, out: sslib.ss_cmvn_packed_device(v, n, off, total, 39, variance, out, None))


def test_cmvnw(torch, sslib, blocks):
    case = M.CASES["cmvnw"]
    with _report(torch, case):
        _row_pair(torch, sslib, blocks, case, 39, 39, lambda v, n, off, total, out: sslib.ss_cmvnw_packed_device(v, n, off, total, 39, 31, 0, out, None))


def test_cmvnw_with_variance_and_its_scratch_block(torch, sslib, blocks):
    """two launches through a stream-ordered scratch block of the block's size; the big call is in place (module docstring), the
    small one is not: the bits are the same"""
    case = M.CASES["cmvnw_var"]
    with _report(torch, case):
        _row_pair(torch, sslib, blocks, case, 39, 39, lambda v, n, off, total, out: sslib.ss_cmvnw_packed_device(v, n, off, total, 39, 31, 1, out, None),
                  in_place=True)


def test_power_to_db_with_the_per_clip_floor(torch, sslib, blocks):
    case = M.CASES["power_to_db"]
    with _report(torch, case):
        w = _row_pair(torch, sslib, blocks, case, 39, 39,
                      lambda v, n, off, total, out: sslib.ss_power_to_db_packed_device(v, n, off, total, 39, 1.0, 1e-10, 20.0, out, None), square=True)
        # top_db = 20 bites: every clip but the one-row one has elements on its floor
        lo = M.RowLayout(0).small_offsets()
        assert all((w[39 * lo[b]:39 * lo[b + 1]] == w[39 * lo[b]:39 * lo[b + 1]].min()).sum() > 1 for b in range(1, 5))


def _groups(lay, tail):
    return np.concatenate([np.full(lay.n_filler, -1, np.int32), np.asarray(tail, np.int32)])


GROUP_FORMS = {"speaker": (M.TAIL_GROUPS, M.TAIL_GROUPS, 2), "global": (None, (0,) * 5, 1)}  # small table, the tail's ids in the big table, n_groups


def _group_tables(torch, lay, form):
    small, tail, n_groups = GROUP_FORMS[form]
    d_small = None if small is None else _dev(torch, np.asarray(small, np.int32))
    return d_small, _dev(torch, _groups(lay, tail)), n_groups


def _stats(torch, sslib, vec, n, off, total, grp, n_groups):
    st = torch.zeros(n_groups * (2 * 39 + 1), dtype=torch.float64, device="cuda")
    _ok(sslib, sslib.ss_cmvn_stats_packed_device(vec.data_ptr(), n, off.data_ptr(), total, 39, grp.data_ptr() if grp is not None else None, n_groups,
                                                 st.data_ptr(), None))
    return st


@pytest.mark.parametrize("form", sorted(GROUP_FORMS))
def test_cmvn_group_stats(torch, sslib, blocks, form):
    """filler clips are of group -1 (left out); the global form's small run has no table at all"""
    case = M.CASES["cmvn_stats"]
    lay = case.filler["layout"]
    with _report(torch, case):
        g_small, g_big, n_groups = _group_tables(torch, lay, form)
        want = _stats(torch, sslib, blocks.tail_rows(39), 5, _dev(torch, lay.small_offsets()), ROWS_T, g_small, n_groups)
        got = _stats(torch, sslib, blocks.rows(39), lay.n_clips, _dev(torch, lay.offsets()), lay.total_rows, g_big, n_groups)
        torch.cuda.synchronize()
        w = want.cpu().numpy()
        assert w[0] == (sum(M.TAIL_ROWS[0::2]) if form == "speaker" else ROWS_T) and np.isfinite(w).all()
        _same(w, got.cpu().numpy(), case.name, 79)


@pytest.mark.parametrize("variance", [0, 1], ids=["mean", "var"])
def test_cmvn_group_apply(torch, sslib, blocks, variance):
    case = M.CASES["cmvn_apply"]
    lay = case.filler["layout"]
    with _report(torch, case):
        g_small, g_big, n_groups = _group_tables(torch, lay, "speaker")
        st = _stats(torch, sslib, blocks.tail_rows(39), 5, _dev(torch, lay.small_offsets()), ROWS_T, g_small, n_groups)

        def call(v, n, off, total, out):
            grp = g_small if n == 5 else g_big
            return sslib.ss_cmvn_apply_packed_device(v, n, off, total, 39, grp.data_ptr(), n_groups, st.data_ptr(), variance, out, None)

        _row_pair(torch, sslib, blocks, case, 39, 39, call)


@pytest.mark.parametrize("form", sorted(GROUP_FORMS))
def test_cmvn_grouped(torch, sslib, blocks, form):
    case = M.CASES["cmvn_grouped_global" if form == "global" else "cmvn_grouped"]
    lay = case.filler["layout"]
    with _report(torch, case):
        g_small, g_big, n_groups = _group_tables(torch, lay, form)

        def call(v, n, off, total, out):
            grp = g_small if n == 5 else g_big
            return sslib.ss_cmvn_grouped_packed_device(v, n, off, total, 39, grp.data_ptr() if grp is not None else None, n_groups, 1, out, None)

        _row_pair(torch, sslib, blocks, case, 39, 39, call)


def test_add_deltas(torch, sslib, blocks):
    case = M.CASES["add_deltas"]
    with _report(torch, case):
        _row_pair(torch, sslib, blocks, case, 13, 39, lambda v, n, off, total, out: sslib.ss_add_deltas_packed_device(v, n, off, total, 13, 2, 2, out, None))


def test_splice(torch, sslib, blocks):
    """left = right = 1, stride 1: the out offsets are the row offsets themselves"""
    case = M.CASES["splice"]
    with _report(torch, case):
        _row_pair(torch, sslib, blocks, case, 13, 39,
                  lambda v, n, off, total, out: sslib.ss_splice_packed_device(v, n, off, total, off, total, 13, 1, 1, 1, out, None))


VAD = (0, 0.02, 0.5, M.VAD_CONTEXT, 0.6)  # energy_col, threshold, mean scale, frames_context, proportion


def test_vad_energy(torch, sslib, blocks):
    case = M.CASES["vad_energy"]
    lay = case.filler["layout"]
    with _report(torch, case):
        counts = {n: torch.full((n,), -9, dtype=torch.int64, device="cuda") for n in (5, lay.n_clips)}
        w = _row_pair(torch, sslib, blocks, case, 39, 1,
                      lambda v, n, off, total, out: sslib.ss_vad_energy_packed_device(v, n, off, total, 39, *VAD, out, counts[n].data_ptr(), None),
                      out_dtype=torch.uint8, fill=255)
        small, big = counts[5].cpu().numpy(), counts[lay.n_clips][lay.n_filler:].cpu().numpy()
        assert np.array_equal(small, big) and set(np.unique(w)) == {0, 1}
        assert small.sum() == int(w.sum()) and 0 < small.sum() < ROWS_T


def test_select_rows(torch, sslib, blocks):
    """the filler's mask keeps every row, so the tail's kept rows lie past element 2^32 of out as well"""
    case = M.CASES["select_rows"]
    lay = case.filler["layout"]
    with _report(torch, case):
        tail_mask = np.random.default_rng(5).integers(0, 3, ROWS_T).astype(np.uint8)  # 0, 1 and another non-zero byte
        tail_mask[0] = 1
        kept = np.array([int((tail_mask[a:b] != 0).sum()) for a, b in zip(lay.small_offsets()[:-1], lay.small_offsets()[1:])])
        m_small = _dev(torch, tail_mask)
        m_big = torch.ones(lay.total_rows, dtype=torch.uint8, device="cuda")
        m_big[lay.tail_row0:] = m_small
        want = torch.full((ROWS_T * 39,), NAN, device="cuda")
        oo_s = torch.full((6,), -9, dtype=torch.int64, device="cuda")
        soff, boff = _dev(torch, lay.small_offsets()), _dev(torch, lay.offsets())  # (held: the calls are asynchronous)
        _ok(sslib, sslib.ss_select_rows_packed_device(blocks.tail_rows(39).data_ptr(), 5, soff.data_ptr(), ROWS_T, 39,
                                                      m_small.data_ptr(), oo_s.data_ptr(), want.data_ptr(), None))
        big = blocks.rows(39)
        got = torch.empty(lay.total_rows * 39, dtype=torch.float32, device="cuda")
        got[lay.tail_row0 * 39:] = NAN
        oo_b = torch.full((lay.n_clips + 1,), -9, dtype=torch.int64, device="cuda")
        _ok(sslib, sslib.ss_select_rows_packed_device(big.data_ptr(), lay.n_clips, boff.data_ptr(), lay.total_rows, 39,
                                                      m_big.data_ptr(), oo_b.data_ptr(), got.data_ptr(), None))
        torch.cuda.synchronize()
        oo_small, oo_big = oo_s.cpu().numpy(), oo_b[lay.n_filler:].cpu().numpy()
        assert np.array_equal(np.diff(oo_small), kept) and oo_small[0] == 0
        assert oo_big[0] == lay.tail_row0 and np.array_equal(oo_big - lay.tail_row0, oo_small)
        n_kept = int(kept.sum())
        w = want[:n_kept * 39].cpu().numpy()
        g = got[lay.tail_row0 * 39:(lay.tail_row0 + n_kept) * 39].cpu().numpy()
        rest = got[(lay.tail_row0 + n_kept) * 39:].cpu().numpy()
        del got, big, m_big
        assert not np.isnan(w).any() and np.isnan(rest).all()  # rows at and past oo[n_clips] are left unwritten
        _same(w, g, case.name, 39)


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
@pytest.mark.parametrize("layout", ["btc", "bct"])
def test_pad(torch, sslib, blocks, layout, dtype):
    import pad_model as PM

    case = M.CASES[f"pad_{layout}_{dtype}"]
    lay = case.filler["layout"]
    per = M.PAD_MAX_ROWS * 39
    tdt = torch.int32 if dtype == "float32" else torch.int16
    with _report(torch, case):
        def call(v, n, off, total, out, lengths):
            return sslib.ss_pad_packed_device(v, n, off, total, 39, M.PAD_MAX_ROWS, PM.LAYOUT_CODE[layout], PM.DTYPE_CODE[dtype], -2.5, out, lengths, None)

        want = torch.full((5 * per,), -1, dtype=tdt, device="cuda")  # all-ones: a NaN in either type
        wl = torch.full((5,), -9, dtype=torch.int32, device="cuda")
        soff, boff = _dev(torch, lay.small_offsets()), _dev(torch, lay.offsets())  # (held: the calls are asynchronous)
        _ok(sslib, call(blocks.tail_rows(39).data_ptr(), 5, soff.data_ptr(), ROWS_T, want.data_ptr(), wl.data_ptr()))
        big = blocks.rows(39)
        got = torch.empty(lay.n_clips * per, dtype=tdt, device="cuda")
        got[lay.n_filler * per:] = -1
        gl = torch.full((lay.n_clips,), -9, dtype=torch.int32, device="cuda")
        _ok(sslib, call(big.data_ptr(), lay.n_clips, boff.data_ptr(), lay.total_rows, got.data_ptr(), gl.data_ptr()))
        torch.cuda.synchronize()
        w, g = want.cpu().numpy(), got[lay.n_filler * per:].cpu().numpy()
        lengths = gl.cpu().numpy()
        del got, big
        assert wl.cpu().tolist() == list(M.TAIL_ROWS) and lengths[lay.n_filler:].tolist() == list(M.TAIL_ROWS)
        assert (lengths[:lay.n_filler] == M.FILLER_ROWS).all()
        assert not (w == -1).any()  # every element of out is written
        _same(w, g, case.name, 39)


SPEC = dict(n_time=2, max_time_width=40, time_ratio=1.0, n_freq=2, max_freq_width=8)
SEED, EPOCH = 2026, 3


def _rng_block(torch):
    return _dev(torch, np.array([SEED, EPOCH], np.uint64).view(np.int64))


@pytest.mark.parametrize("in_place", [False, True], ids=["copy", "inplace"])
def test_specaug(torch, sslib, blocks, in_place):
    """clip_base makes the tail clips' ids the same in both runs: n_filler + b.  In place the mask value is +0.0, which leaves the
    shared block's filler as it was."""
    import specaug_model as SM

    case = M.CASES["specaug_inplace" if in_place else "specaug"]
    lay = case.filler["layout"]
    n_masks = SPEC["n_time"] + SPEC["n_freq"]
    value = 0.0 if in_place else -7.5
    with _report(torch, case):
        def call(v, n, off, total, out, base, spans):
            rng = _rng_block(torch)
            rc = sslib.ss_specaug_packed_device(v, n, off, total, 39, rng.data_ptr(), base, SPEC["n_time"], SPEC["max_time_width"], SPEC["time_ratio"],
                                                SPEC["n_freq"], SPEC["max_freq_width"], value, out, spans.data_ptr(), None)
            return rc, rng

        sp_s = torch.full((5 * n_masks * 2,), -9, dtype=torch.int32, device="cuda")
        sp_b = torch.full((lay.n_clips * n_masks * 2,), -9, dtype=torch.int32, device="cuda")
        soff, boff = _dev(torch, lay.small_offsets()), _dev(torch, lay.offsets())
        small = blocks.tail_rows(39).clone()
        want = small if in_place else torch.full((ROWS_T * 39,), NAN, device="cuda")
        rc, rng_s = call(small.data_ptr(), 5, soff.data_ptr(), ROWS_T, want.data_ptr(), lay.n_filler, sp_s)
        _ok(sslib, rc)
        big = blocks.rows(39)
        t0 = lay.tail_row0 * 39
        if in_place:
            got = big
        else:
            got = torch.empty(lay.total_rows * 39, dtype=torch.float32, device="cuda")
            got[t0:] = NAN
        rc, rng_b = call(big.data_ptr(), lay.n_clips, boff.data_ptr(), lay.total_rows, got.data_ptr(), 0, sp_b)
        _ok(sslib, rc)
        torch.cuda.synchronize()
        w, g = want.cpu().numpy(), got[t0:].cpu().numpy()
        del got, big
        spans = sp_s.cpu().numpy().reshape(5, n_masks, 2)
        assert np.array_equal(spans, sp_b[lay.n_filler * n_masks * 2:].cpu().numpy().reshape(5, n_masks, 2))
        assert np.array_equal(spans, SM.spans_ref((SEED, EPOCH), lay.n_filler, lay.small_offsets(), ROWS_T, 39, **SPEC))
        assert rng_s.cpu().tolist() == [SEED, EPOCH + 1] == rng_b.cpu().tolist()
        src = M.tail_rows_block(39)
        ref = SM.apply_ref(SM.u32(src), lay.small_offsets(), ROWS_T, spans, SPEC["n_time"], SPEC["n_freq"], SM.u32(np.float32(value).reshape(1))[0])
        _same(ref, w, case.name + " (model)", 39)
        assert (SM.u32(w.reshape(-1, 39)) != SM.u32(src)).any()  # something was masked
        _same(w, g, case.name, 39)


def test_mask_spans(torch, sslib, blocks):
    import specaug_model as SM

    case = M.CASES["mask_spans"]
    lay = case.filler["layout"]
    n_masks = SPEC["n_time"] + SPEC["n_freq"]
    with _report(torch, case):
        tail = SM.spans_ref((SEED, EPOCH), lay.n_filler, lay.small_offsets(), ROWS_T, 39, **SPEC)
        filler = np.tile(np.array([[100, 7], [8000, 192], [3, 2], [30, 9]], np.int32)[None], (lay.n_filler, 1, 1))  # valid spans of a filler clip
        tables = {5: _dev(torch, tail.reshape(-1)), lay.n_clips: _dev(torch, np.concatenate([filler, tail]).reshape(-1))}
        _row_pair(torch, sslib, blocks, case, 39, 39,
                  lambda v, n, off, total, out: sslib.ss_mask_spans_packed_device(v, n, off, total, 39, tables[n].data_ptr(), SPEC["n_time"],
                                                                                  SPEC["n_freq"], -7.5, out, None))
        assert n_masks == 4


# ---- section 3: the pool calls, from fresh streams ----

def _pool_pair(torch, sslib, blocks, case, cols, out_cols, state_len, call, out_dtype=None, fill=NAN):
    """call(vec, n_active, row_offsets, total_rows, slots, pool_streams, pool, out): every entry owns its own slot of a zeroed pool;
    the tail entries' rows and pool rows are the bits of the small run"""
    lay = case.filler["layout"]
    assert state_len == case.counts["state_len"] and lay.n_clips == case.counts["pool_streams"]
    pools = {n: torch.zeros(n * state_len, dtype=torch.float32, device="cuda") for n in (5, lay.n_clips)}
    slots = {n: torch.arange(n, dtype=torch.int32, device="cuda") for n in (5, lay.n_clips)}
    _row_pair(torch, sslib, blocks, case, cols, out_cols,
              lambda v, n, off, total, out: call(v, n, off, total, slots[n].data_ptr(), n, pools[n].data_ptr(), out), out_dtype=out_dtype, fill=fill)
    w, g = pools[5].cpu().numpy(), pools[lay.n_clips][lay.n_filler * state_len:].cpu().numpy()
    assert np.any(w != 0)
    _same(w, g, case.name + " (pool rows)", state_len)


def _state_len(sslib, fn, *args):
    n = C.c_size_t()
    extra = [C.byref(C.c_size_t())] if fn == "ss_splice_stream_state_len" else []
    assert getattr(sslib, fn)(*args, C.byref(n), *extra) == 0
    return n.value


def test_cmvn_stream_pool(torch, sslib, blocks):
    case = M.CASES["cmvn_stream"]
    with _report(torch, case):
        L = _state_len(sslib, "ss_cmvn_stream_state_len", 39, M.CMVN_STREAM_WIN)
        _pool_pair(torch, sslib, blocks, case, 39, 39, L, lambda v, n, ro, total, sl, P, pool, out: sslib.ss_cmvn_stream_packed_device(
            v, n, ro, total, sl, P, 39, M.CMVN_STREAM_WIN, 1, pool, out, None))


def test_add_deltas_stream_pool(torch, sslib, blocks):
    case = M.CASES["add_deltas_stream"]
    with _report(torch, case):
        L = _state_len(sslib, "ss_add_deltas_stream_state_len", 13, 2, 2)
        _pool_pair(torch, sslib, blocks, case, 13, 39, L, lambda v, n, ro, total, sl, P, pool, out: sslib.ss_add_deltas_stream_packed_device(
            v, n, ro, total, sl, P, 13, 2, 2, pool, out, None))


def test_splice_stream_pool(torch, sslib, blocks):
    case = M.CASES["splice_stream"]
    with _report(torch, case):
        L = _state_len(sslib, "ss_splice_stream_state_len", 13, 1, 1, 1)
        _pool_pair(torch, sslib, blocks, case, 13, 39, L, lambda v, n, ro, total, sl, P, pool, out: sslib.ss_splice_stream_packed_device(
            v, n, ro, total, sl, P, 13, 1, 1, 1, pool, out, None))


def test_vad_energy_stream_pool(torch, sslib, blocks):
    case = M.CASES["vad_energy_stream"]
    with _report(torch, case):
        L = _state_len(sslib, "ss_vad_energy_stream_state_len", M.VAD_CONTEXT)
        _pool_pair(torch, sslib, blocks, case, 39, 1, L, lambda v, n, ro, total, sl, P, pool, out: sslib.ss_vad_energy_stream_packed_device(
            v, n, ro, total, sl, P, 39, *VAD, pool, out, None), out_dtype=torch.uint8, fill=255)


# ---- section 4: the sample side ----

def _sample_pair(torch, blocks, name, run):
    """run(x_ptr, base, total_in) -> device tensors, once on the clips alone in a small buffer (base 0) and once at the end of the
    buffer of BIG samples (device sample offsets are absolute; output offsets stay compact): the same bits, free of NaN"""
    case = M.CASES[name]
    lens, eb = M.SAMPLE_CASES[name]
    n, base = sum(lens), M.sample_base(name)
    with _report(torch, case):
        big = blocks.samples(eb == 2)
        small = big[base:base + n].clone()
        outs = []
        for ptr, b, total in ((small.data_ptr(), 0, n), (big.data_ptr(), base, M.BIG)):
            res = run(ptr, b, total)
            torch.cuda.synchronize()
            outs.append([t.view(torch.int16).cpu().numpy() if t.dtype == torch.bfloat16 else t.cpu().numpy() for t in res])
        assert base >= M.TWO32 and len(outs[0]) == len(outs[1]) > 0
        for i, (w, g) in enumerate(zip(*outs)):
            if w.dtype.kind == "f":
                assert not np.isnan(w).any(), (name, i)
            _same(w, g, f"{name} (output {i})")


# The kernel each sample-side case must run on, as (prefix, suffix) of ss_last_kernel_name(): a quiet change of dispatch would
# otherwise leave the named kernel untested past 2^32.  The names are those the families' own test files assert.
KERNELS = {
    "mfcc": (b"ss_mfcc_c256v<10,exact,bank421,sym>", b""), "mfcc_i16": (b"ss_mfcc_c256vi<10,exact,bank421,sym>", b""),
    "mfe_i16": (b"ss_front_generic_varleni<", b">"), "lmfe": (b"ss_front_generic_varlen<", b">"),
    "mel": (b"ss_mel_c1024v<w12,mel6321>", b""), "mel_i16": (b"ss_mel_c1024vi<w12,mel6321>", b""),
    "stft": (b"ss_front_generic_varrows<", b">"), "stft_i16": (b"ss_front_generic_varrowsi<", b">"),
    "log_mel_cfg3": (b"ss_mel_c1024v<w12,mel6321,db>", b""), "log_mel_chirpz400": (b"ss_front_generic_varrows<", b"chirpz,db>"),
    "kaldi_fbank": (b"ss_kaldi_c256<13,pow2,fbank,v>", b""), "kaldi_mfcc": (b"ss_kaldi_c256<13,pow2,mfcc,v>", b""),
    "kstream_fbank": (b"ss_kaldi_c256<13,pow2,fbank,sp>", b""), "kstream_fbank_i16": (b"ss_kaldi_c256<13,pow2,fbank,spi>", b""),
    "mfcc_stream": (b"ss_mfcc_c256sp<10,exact,bank421,sym>", b""), "mel_stream": (b"ss_mel_c1024sp<w12,mel6321>", b""),
    "whisper": (b"ss_whisper_c200", b""), "resample": (b"ss_resample_kernel<packed,f32>", b""), "resample_i16": (b"ss_resample_kernel<packed,i16>", b""),
    "resample_stream": (b"ss_resample_stream_kernel<f32>", b""), "resample_dense": (b"ss_resample_kernel<dense,f32>", b""),
    "kaldi_dense": (b"ss_kaldi_c256<13,pow2,fbank>", b""),
}


def _ran_on(sslib, key):
    name, (prefix, suffix) = sslib.ss_last_kernel_name(), KERNELS[key]
    assert name.startswith(prefix) and name.endswith(suffix) and (suffix or name == prefix), (key, name)


def _so(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


def _speech(ss, **kw):
    from speechsauce_amd import _lib

    return ss.SpeechConfig(_lib.make_params(**kw))


CFG3 = dict(sample_rate=16000, fft_points=2048, frame_length=0.032, frame_stride=0.032, num_filters=128, high_frequency=8000.0)
CHIRPZ400 = dict(fft_points=400, frame_length=0.01)


@pytest.mark.parametrize("name", ["mfcc", "mfcc_i16", "mfe_i16", "lmfe"])
def test_frame_path_packed_calls(torch, ss, sslib, blocks, name):
    """ss_mfcc_packed_device, ss_mfcc_packed_i16_device, ss_mfe_packed_i16_device, ss_lmfe_packed_device"""
    lens, eb = M.SAMPLE_CASES[name]
    cfg = _speech(ss)
    so, fo = ss._packed_offsets(cfg, np.asarray(lens, np.int64), sum(lens), name)
    rows, dfo = int(fo[-1]), _dev(torch, fo)
    sc = [PCM_SCALE] if eb == 2 else []

    def run(x, base, total):
        dso = _dev(torch, so + base)
        feat = torch.full((rows, cfg.params.num_cepstral if name.startswith("mfcc") else cfg.params.num_filters), NAN, device="cuda")
        outs = [feat]
        if name.startswith("mfcc"):
            rc = getattr(sslib, f"ss_{name.replace('_i16', '_packed_i16') if eb == 2 else 'mfcc_packed'}_device")(
                cfg.handle, x, 5, dso.data_ptr(), *sc, dfo.data_ptr(), rows, feat.data_ptr(), None)
        elif name == "mfe_i16":
            en = torch.full((rows,), NAN, device="cuda")
            outs.append(en)
            rc = sslib.ss_mfe_packed_i16_device(cfg.handle, x, 5, dso.data_ptr(), PCM_SCALE, dfo.data_ptr(), rows, feat.data_ptr(), en.data_ptr(), None)
        else:
            rc = sslib.ss_lmfe_packed_device(cfg.handle, x, 5, dso.data_ptr(), dfo.data_ptr(), rows, feat.data_ptr(), None, None)
        _ok(sslib, rc)
        _ran_on(sslib, name)
        torch.cuda.synchronize()
        cfg.device_status()
        return outs

    _sample_pair(torch, blocks, name, run)


@pytest.mark.parametrize("name", ["mel", "stft", "mel_i16", "stft_i16", "log_mel_cfg3", "log_mel_chirpz400"])
def test_spectrogram_packed_calls(torch, ss, sslib, blocks, name):
    """ss_mel_spectrogram_packed_device, ss_stft_packed_device, their _i16 forms, ss_log_mel_spectrogram_packed_device (the
    2048-point kernel and the chirp-z 400 build)"""
    lens, eb = M.SAMPLE_CASES[name]
    cfg = _speech(ss, **(CHIRPZ400 if name.endswith("chirpz400") else CFG3))
    so = _so(lens)
    ro = ss._row_offsets(cfg, so)
    rows, dro = int(ro[-1]), _dev(torch, ro)
    sc = [PCM_SCALE] if eb == 2 else []
    stft = name.startswith("stft")
    n_out = rows * (cfg.params.fft_points // 2 + 1) * 2 if stft else rows * cfg.params.num_filters

    def run(x, base, total):
        dso = _dev(torch, so + base)
        out = torch.full((n_out,), NAN, device="cuda")
        if name.startswith("log_mel"):
            rc = sslib.ss_log_mel_spectrogram_packed_device(cfg.handle, x, 5, dso.data_ptr(), dro.data_ptr(), rows, 1.0, 1e-10, 80.0, out.data_ptr(), None)
        else:
            fn = f"ss_{'stft' if stft else 'mel_spectrogram'}_packed{'_i16' if eb == 2 else ''}_device"
            rc = getattr(sslib, fn)(cfg.handle, x, 5, dso.data_ptr(), *sc, dro.data_ptr(), rows, out.data_ptr(), None)
        _ok(sslib, rc)
        _ran_on(sslib, name)
        torch.cuda.synchronize()
        cfg.device_status()
        return [out]

    _sample_pair(torch, blocks, name, run)


def _kaldi(ss, sslib, **kw):
    from test_kaldi_cpu import make_kaldi_params

    return ss.KaldiConfig(make_kaldi_params(sslib, **kw))


@pytest.mark.parametrize("name", ["kaldi_fbank", "kaldi_mfcc"])
def test_kaldi_packed_calls(torch, ss, sslib, blocks, name):
    lens, _ = M.SAMPLE_CASES[name]
    mfcc = name == "kaldi_mfcc"
    cfg = _kaldi(ss, sslib) if mfcc else _kaldi(ss, sslib, num_mel_bins=80)
    so = _so(lens)
    fo = np.empty_like(so)
    assert sslib.ss_kaldi_packed_frame_offsets(C.byref(cfg.params), 5, so.ctypes.data, fo.ctypes.data) == 0
    rows, dfo = int(fo[-1]), _dev(torch, fo)

    def run(x, base, total):
        dso = _dev(torch, so + base)
        out = torch.full((rows, cfg.params.num_ceps if mfcc else cfg.params.num_mel_bins), NAN, device="cuda")
        en = torch.full((rows,), NAN, device="cuda")
        if mfcc:
            rc = sslib.ss_kaldi_mfcc_packed_device(cfg.handle, x, 5, dso.data_ptr(), dfo.data_ptr(), rows, out.data_ptr(), None)
        else:
            rc = sslib.ss_kaldi_fbank_packed_device(cfg.handle, x, 5, dso.data_ptr(), dfo.data_ptr(), rows, out.data_ptr(), en.data_ptr(), None)
        _ok(sslib, rc)
        _ran_on(sslib, name)
        torch.cuda.synchronize()
        assert sslib.ss_kaldi_config_device_status(cfg.handle) == 0
        return [out] if mfcc else [out, en]

    _sample_pair(torch, blocks, name, run)


@pytest.mark.parametrize("name", ["kstream_fbank", "kstream_fbank_i16"])
def test_kaldi_pool_from_a_fresh_pool(torch, ss, sslib, blocks, name):
    lens, eb = M.SAMPLE_CASES[name]
    cfg = _kaldi(ss, sslib, num_mel_bins=80)
    S, D = C.c_size_t(), C.c_size_t()
    assert sslib.ss_kstream_state_len(C.byref(cfg.params), C.byref(S), C.byref(D)) == 0 and S.value == 320
    so = _so(lens)
    ro = so // 160
    rows, dro = int(ro[-1]), _dev(torch, ro)
    slots = torch.arange(5, dtype=torch.int32, device="cuda")
    sc = [PCM_SCALE] if eb == 2 else []

    def run(x, base, total):
        dso = _dev(torch, so + base)
        pool = torch.zeros(5 * S.value, dtype=torch.float32, device="cuda")
        out = torch.full((rows, 80), NAN, device="cuda")
        en = torch.full((rows,), NAN, device="cuda")
        fn = getattr(sslib, f"ss_kstream_fbank_packed{'_i16' if eb == 2 else ''}_device")
        _ok(sslib, fn(cfg.handle, x, 5, dso.data_ptr(), dro.data_ptr(), rows, slots.data_ptr(), 5, *sc, pool.data_ptr(), out.data_ptr(), en.data_ptr(), None))
        _ran_on(sslib, name)
        torch.cuda.synchronize()
        assert sslib.ss_kaldi_config_device_status(cfg.handle) == 0
        return [out, en, pool]

    _sample_pair(torch, blocks, name, run)


@pytest.mark.parametrize("name", ["mfcc_stream", "mel_stream"])
def test_front_end_pools_from_a_fresh_pool(torch, ss, sslib, blocks, name):
    """ss_mfcc_stream_packed_device (hop 160) and ss_mel_spectrogram_stream_packed_device (the 2048-point configuration, hop 512)"""
    lens, _ = M.SAMPLE_CASES[name]
    mel = name == "mel_stream"
    cfg = _speech(ss, **(CFG3 if mel else {}))
    S = C.c_size_t()
    assert getattr(sslib, "ss_stream_state_len" if mel else "ss_frame_stream_state_len")(C.byref(cfg.params), C.byref(S)) == 0 and S.value > 0
    so = _so(lens)
    ro = so // (512 if mel else 160)
    rows, dro = int(ro[-1]), _dev(torch, ro)
    slots = torch.arange(5, dtype=torch.int32, device="cuda")

    def run(x, base, total):
        dso = _dev(torch, so + base)
        pool = torch.zeros(5 * S.value, dtype=torch.float32, device="cuda")
        out = torch.full((rows * (cfg.params.num_filters if mel else cfg.params.num_cepstral),), NAN, device="cuda")
        if mel:
            rc = sslib.ss_mel_spectrogram_stream_packed_device(cfg.handle, x, 5, dso.data_ptr(), dro.data_ptr(), rows, slots.data_ptr(), 5, pool.data_ptr(),
                                                               out.data_ptr(), None)
        else:
            rc = sslib.ss_mfcc_stream_packed_device(cfg.handle, x, 5, dso.data_ptr(), dro.data_ptr(), rows, slots.data_ptr(), 5, 100, pool.data_ptr(),
                                                    out.data_ptr(), None)
        _ok(sslib, rc)
        _ran_on(sslib, name)
        torch.cuda.synchronize()
        cfg.device_status()
        return [out, pool]

    _sample_pair(torch, blocks, name, run)


WHISPER_FRAMES = 300  # 48000 / 160: the longest clip fills the window


@pytest.mark.parametrize("name", ["whisper_f32", "whisper_bf16"])
def test_whisper_packed(torch, ss, sslib, blocks, name):
    lens, _ = M.SAMPLE_CASES[name]
    bf16 = name.endswith("bf16")
    cfg = ss.WhisperConfig(80)
    so = _so(lens)
    n_out = 5 * 80 * WHISPER_FRAMES

    def run(x, base, total):
        dso = _dev(torch, so + base)
        out = torch.full((n_out,), -1, dtype=torch.int16, device="cuda") if bf16 else torch.full((n_out,), NAN, device="cuda")
        work = torch.empty(n_out, dtype=torch.float32, device="cuda") if bf16 else None
        lengths = torch.full((5,), -9, dtype=torch.int32, device="cuda")
        _ok(sslib, sslib.ss_whisper_log_mel_packed_device(cfg.handle, x, 5, dso.data_ptr(), WHISPER_FRAMES, 2 if bf16 else 0,
                                                          work.data_ptr() if bf16 else None, out.data_ptr(), lengths.data_ptr(), None))
        _ran_on(sslib, "whisper")
        torch.cuda.synchronize()
        assert sslib.ss_whisper_config_device_status(cfg.handle) == 0
        assert lengths.cpu().tolist() == [min(n // 160, WHISPER_FRAMES) for n in lens]
        all_written = not bf16 or not bool((out == -1).any())
        assert all_written
        return [out, lengths]

    _sample_pair(torch, blocks, name, run)


def test_whisper_output_block_past_two_to_the_32(torch, ss, sslib, blocks):
    """11200 clips x 128 mels x 3000 frames: all empty but the last five.  Empty clips cost no transform, so only the floor launch
    walks the block: clip 11195 + b is the five-clip call's clip b, and every empty clip's block is all -1.5 (one reduction on the
    device)."""
    case = M.CASES["whisper_output_block"]
    w_ = M.WHISPER_BLOCK
    n_clips, blk, nf = w_["n_clips"], w_["n_mels"] * w_["n_frames"], w_["n_frames"]
    lens = M.SAMPLE_LENS
    blocks.drop()
    with _report(torch, case):
        cfg = ss.WhisperConfig(w_["n_mels"])
        x = _dev(torch, M.sample_tail()[:sum(lens)])
        so5 = _so(lens)
        so_big = np.concatenate([np.zeros(n_clips - 5, np.int64), so5])

        def call(so, n, out, lengths):
            dso = _dev(torch, so)
            _ok(sslib, sslib.ss_whisper_log_mel_packed_device(cfg.handle, x.data_ptr(), n, dso.data_ptr(), nf, 0, None, out.data_ptr(),
                                                              lengths.data_ptr(), None))
            _ran_on(sslib, "whisper")
            torch.cuda.synchronize()
            assert sslib.ss_whisper_config_device_status(cfg.handle) == 0

        want = torch.full((5 * blk,), NAN, device="cuda")
        wl = torch.full((5,), -9, dtype=torch.int32, device="cuda")
        call(so5, 5, want, wl)
        got = torch.empty(n_clips * blk, dtype=torch.float32, device="cuda")
        got[(n_clips - 5) * blk:] = NAN
        gl = torch.full((n_clips,), -9, dtype=torch.int32, device="cuda")
        call(so_big, n_clips, got, gl)
        minus_1_5 = int(np.float32(-1.5).view(np.int32))
        # (the verdict first, as a plain bool: a failing assert must not have pytest describe a 17 GB tensor)
        empties_are_floor = bool((got[:(n_clips - 5) * blk].view(torch.int32) == minus_1_5).all())
        assert empties_are_floor
        lengths = gl.cpu().numpy()
        assert (lengths[:n_clips - 5] == 0).all() and lengths[n_clips - 5:].tolist() == wl.cpu().tolist() == [min(n // 160, nf) for n in lens]
        w, g = want.cpu().numpy(), got[(n_clips - 5) * blk:].cpu().numpy()
        del got
        assert not np.isnan(w).any()
        _same(w, g, case.name, nf)


RATES = {"441_160": (44100, 16000), "1_2": (8000, 16000)}


@pytest.mark.parametrize("name", ["resample_441_160", "resample_1_2", "resample_i16_441_160", "resample_i16_1_2"])
def test_resample_packed_input_side(torch, ss, sslib, blocks, name):
    lens, eb = M.SAMPLE_CASES[name]
    orig, new = RATES[name.split("_", 2)[2] if eb == 2 else name.split("_", 1)[1]]
    rs = ss.Resampler(orig, new)
    so = _so(lens)
    oo = np.empty_like(so)
    assert sslib.ss_resample_packed_offsets(orig, new, 5, so.ctypes.data, oo.ctypes.data) == 0
    doo, n_out = _dev(torch, oo), int(oo[-1])
    sc = [PCM_SCALE] if eb == 2 else []

    def run(x, base, total):
        dso = _dev(torch, so + base)
        out = torch.full((n_out,), NAN, device="cuda")
        fn = getattr(sslib, f"ss_resample_packed{'_i16' if eb == 2 else ''}_device")
        _ok(sslib, fn(rs.handle, x, 5, dso.data_ptr(), *sc, doo.data_ptr(), total, n_out, out.data_ptr(), None))
        _ran_on(sslib, "resample_i16" if eb == 2 else "resample")
        return [out]

    _sample_pair(torch, blocks, name, run)


def test_resample_packed_output_side(torch, ss, sslib, blocks):
    """8 kHz -> 16 kHz: filler clips of zeros in front put the tail clips' outputs past element 2^32 of out"""
    case = M.CASES["resample_output_side"]
    nf, fl = case.filler["n_filler"], M.RESAMPLE_FILLER
    lens = M.SAMPLE_LENS
    n = sum(lens)
    with _report(torch, case):
        rs = ss.Resampler(8000, 16000)
        src = _dev(torch, M.sample_tail()[:n])

        def make():
            x = torch.zeros(nf * fl + n, dtype=torch.float32, device="cuda")
            x[nf * fl:] = src
            return x

        big = blocks.custom("resample_output_side", make)
        so5 = _so(lens)
        so_big = np.concatenate([np.arange(nf, dtype=np.int64) * fl, nf * fl + so5])
        want = torch.full((2 * n,), NAN, device="cuda")
        tables = [_dev(torch, t) for t in (so5, 2 * so5, so_big, 2 * so_big)]  # (held: the calls are asynchronous)
        _ok(sslib, sslib.ss_resample_packed_device(rs.handle, src.data_ptr(), 5, tables[0].data_ptr(), tables[1].data_ptr(), n, 2 * n,
                                                   want.data_ptr(), None))
        total_out = 2 * (nf * fl + n)
        got = torch.empty(total_out, dtype=torch.float32, device="cuda")
        got[2 * nf * fl:] = NAN
        _ok(sslib, sslib.ss_resample_packed_device(rs.handle, big.data_ptr(), nf + 5, tables[2].data_ptr(), tables[3].data_ptr(),
                                                   nf * fl + n, total_out, got.data_ptr(), None))
        _ran_on(sslib, "resample")
        torch.cuda.synchronize()
        w, g = want.cpu().numpy(), got[2 * nf * fl:].cpu().numpy()
        del got, big
        assert not np.isnan(w).any()
        _same(w, g, case.name)


def test_resample_pool_from_a_fresh_pool(torch, ss, sslib, blocks):
    """44.1 kHz -> 16 kHz: entry i's outputs lie at so[i] / 441 * 160 of out [total_in / 441 * 160], so the output block follows the
    input's offsets: allocated in full, the tail prefilled"""
    name = "resample_stream"
    case = M.CASES[name]
    lens, _ = M.SAMPLE_CASES[name]
    o, n_ = M.RESAMPLE_STREAM_RATIO
    rs = ss.Resampler(44100, 16000)
    L = C.c_size_t()
    assert sslib.ss_resample_stream_state_len(rs.handle, C.byref(L)) == 0
    so = _so(lens)
    n_out = int(so[-1]) // o * n_
    slots = torch.arange(5, dtype=torch.int32, device="cuda")

    def run(x, base, total):
        assert base % o == 0
        total_in = total // o * o
        first = base // o * n_
        dso = _dev(torch, so + base)
        pool = torch.zeros(5 * L.value, dtype=torch.float32, device="cuda")
        out = torch.empty(total_in // o * n_, dtype=torch.float32, device="cuda")
        assert out.numel() == (case.block("out").elems if base else n_out) and first == (case.block("out").tail if base else 0)
        out[first:] = NAN
        _ok(sslib, sslib.ss_resample_stream_packed_device(rs.handle, x, 5, dso.data_ptr(), total_in, slots.data_ptr(), 5, pool.data_ptr(), out.data_ptr(), None))
        _ran_on(sslib, "resample_stream")
        torch.cuda.synchronize()
        rest_untouched = bool(torch.isnan(out[first + n_out:]).all())  # outputs behind the last entry are left alone
        assert rest_untouched
        return [out[first:first + n_out].clone(), pool]

    _sample_pair(torch, blocks, name, run)


# ---- section 5: dense strides of 2^32 + 2 ----

def _wide(torch, blocks, rows):
    """three rows at a stride of DENSE_LD floats, in a block allocated in full"""
    def make():
        x = torch.zeros(2 * M.DENSE_LD + M.DENSE_ROW, dtype=torch.float32, device="cuda")
        for b in range(3):
            x[b * M.DENSE_LD:b * M.DENSE_LD + M.DENSE_ROW] = rows[b]
        return x

    return blocks.custom("wide", make)


def _dense_rows(torch):
    return _dev(torch, (np.random.default_rng(21).standard_normal((3, M.DENSE_ROW)) * 0.1).astype(np.float32))


def _dense_pair(torch, blocks, case, run):
    """run(x_ptr, ld) -> device tensors: the rows at a small stride, then at DENSE_LD"""
    with _report(torch, case):
        rows = _dense_rows(torch)
        want = [t.cpu().numpy() for t in run(rows.data_ptr(), M.DENSE_ROW)]
        wide = _wide(torch, blocks, rows)
        got = [t.cpu().numpy() for t in run(wide.data_ptr(), M.DENSE_LD)]
        del wide
        for i, (w, g) in enumerate(zip(want, got)):
            assert not np.isnan(w).any()
            _same(w, g, f"{case.name} (output {i})")


def test_dense_stride_kaldi_fbank(torch, ss, sslib, blocks):
    cfg = _kaldi(ss, sslib, num_mel_bins=80)
    T = 1 + (M.DENSE_ROW - 400) // 160

    def run(x, ld):
        out, en = torch.full((3 * T, 80), NAN, device="cuda"), torch.full((3 * T,), NAN, device="cuda")
        _ok(sslib, sslib.ss_kaldi_fbank_device(cfg.handle, x, 3, M.DENSE_ROW, ld, out.data_ptr(), en.data_ptr(), None))
        _ran_on(sslib, "kaldi_dense")
        torch.cuda.synchronize()
        return [out, en]

    _dense_pair(torch, blocks, M.CASES["dense_kaldi_fbank"], run)


def test_dense_stride_whisper(torch, ss, sslib, blocks):
    cfg = ss.WhisperConfig(80)

    def run(x, ld):
        out = torch.full((3 * 80 * WHISPER_FRAMES,), NAN, device="cuda")
        _ok(sslib, sslib.ss_whisper_log_mel_device(cfg.handle, x, 3, M.DENSE_ROW, ld, WHISPER_FRAMES, 0, None, out.data_ptr(), None))
        _ran_on(sslib, "whisper")
        torch.cuda.synchronize()
        return [out]

    _dense_pair(torch, blocks, M.CASES["dense_whisper"], run)


def test_dense_stride_resample_ld(torch, ss, sslib, blocks):
    rs = ss.Resampler(44100, 16000)
    n_out = -(-M.DENSE_ROW * 160 // 441)

    def run(x, ld):
        out = torch.full((3 * n_out,), NAN, device="cuda")
        _ok(sslib, sslib.ss_resample_device(rs.handle, x, 3, M.DENSE_ROW, ld, out.data_ptr(), n_out, None))
        _ran_on(sslib, "resample_dense")
        torch.cuda.synchronize()
        return [out]

    _dense_pair(torch, blocks, M.CASES["dense_resample_in"], run)


def test_dense_stride_resample_ld_out(torch, ss, sslib, blocks):
    """8 kHz -> 16 kHz with ld_out = 2^32 + 2: the three out rows lie 2^32 + 2 floats apart in an out block allocated in full"""
    case = M.CASES["dense_resample_out"]
    rs = ss.Resampler(8000, 16000)
    n_out = 2 * M.DENSE_ROW
    blocks.drop()
    with _report(torch, case):
        rows = _dense_rows(torch)
        want = torch.full((3 * n_out,), NAN, device="cuda")
        _ok(sslib, sslib.ss_resample_device(rs.handle, rows.data_ptr(), 3, M.DENSE_ROW, M.DENSE_ROW, want.data_ptr(), n_out, None))
        got = torch.empty(case.block("wide").elems, dtype=torch.float32, device="cuda")
        for b in range(3):
            got[b * M.DENSE_LD:b * M.DENSE_LD + n_out] = NAN
        _ok(sslib, sslib.ss_resample_device(rs.handle, rows.data_ptr(), 3, M.DENSE_ROW, M.DENSE_ROW, got.data_ptr(), M.DENSE_LD, None))
        _ran_on(sslib, "resample_dense")
        torch.cuda.synchronize()
        w = want.cpu().numpy()
        g = np.concatenate([got[b * M.DENSE_LD:b * M.DENSE_LD + n_out].cpu().numpy() for b in range(3)])
        del got
        assert not np.isnan(w).any()
        _same(w, g, case.name)


# ---- section 6: one clip whose own element count passes 2^32 ----
# The clip repeats a seeded tile of LONG_TILE rows, so the rows near any position follow from the tile by the stage's model.  Three
# windows of 64 rows are compared bit for bit: the clip's start, across the row that holds element 2^32, its end.  The per-clip CMVN
# kernels, the grouped statistics and the VAD recompute a clip's statistics in every workgroup that shares it: they are not here.

def _long_block(torch, blocks, cols):
    def make():
        tile = _dev(torch, M.long_tile(cols).reshape(-1))
        per, full = M.LONG_TILE * cols, M.LONG_ROWS // M.LONG_TILE
        x = torch.empty(M.LONG_ROWS * cols, dtype=torch.float32, device="cuda")
        x[:full * per].view(full, per).copy_(tile.view(1, per).expand(full, per))
        x[full * per:] = tile[:M.LONG_ROWS * cols - full * per]
        return x

    return blocks.custom(("long", cols), make)


def _long_table(torch):
    return _dev(torch, np.array([0, M.LONG_ROWS], np.int64))


def _long_out(torch, rows=M.LONG_ROWS, dtype=None):
    return torch.full((rows * 39,), NAN, dtype=dtype or torch.float32, device="cuda")


def _windows_same(out, out_rows, expect, what):
    for lo, hi in M.long_windows(out_rows, 39):
        _same(expect(lo, hi), out[lo * 39:hi * 39].cpu().numpy(), f"{what} rows {lo}..{hi}", 39)


def _local(tile, lo, hi, halo, f):
    """rows lo .. hi of f(the long clip), from the rows within `halo` of them: f clamps at its argument's ends, and the argument ends
    where the clip does or `halo` rows away"""
    a, b = max(0, lo - halo), min(M.LONG_ROWS, hi + halo)
    return f(M.tiled_rows(tile, a, b))[lo - a:hi - a]


def _masked(tile, lo, hi, spans, n_time, value):
    w = M.tiled_rows(tile, lo, hi).copy()
    r = np.arange(lo, hi)
    for k, (start, width) in enumerate(spans):
        if k < n_time:
            w[(r >= start) & (r < start + width)] = value
        else:
            w[:, start:start + width] = value
    return w


def test_long_clip_mask_spans(torch, sslib, blocks):
    case = M.CASES["long_mask_spans"]
    mid = M.TWO32 // 39
    spans = np.array([[10, 30], [mid - 10, 25], [M.LONG_ROWS - 40, 40], [3, 2], [30, 9]], np.int32)  # three time spans in the windows, two of columns
    with _report(torch, case):
        x, ro, d_spans, out = _long_block(torch, blocks, 39), _long_table(torch), _dev(torch, spans.reshape(-1)), _long_out(torch)
        _ok(sslib, sslib.ss_mask_spans_packed_device(x.data_ptr(), 1, ro.data_ptr(), M.LONG_ROWS, 39, d_spans.data_ptr(), 3, 2, -7.5, out.data_ptr(), None))
        torch.cuda.synchronize()
        tile = M.long_tile(39)
        _windows_same(out, M.LONG_ROWS, lambda lo, hi: _masked(tile, lo, hi, spans, 3, np.float32(-7.5)), case.name)


LONG_SPEC = dict(n_time=2, max_time_width=2 ** 20, time_ratio=1.0, n_freq=2, max_freq_width=8)


@pytest.mark.parametrize("in_place", [False, True], ids=["copy", "inplace"])
def test_long_clip_specaug(torch, sslib, blocks, in_place):
    """the spans are the device's own draw, held to the host model; the mask value of the in-place form differs from every input"""
    import specaug_model as SM

    case = M.CASES["long_specaug_inplace" if in_place else "long_specaug"]
    with _report(torch, case):
        x, ro, rng = _long_block(torch, blocks, 39), _long_table(torch), _rng_block(torch)
        out = x if in_place else _long_out(torch)
        d_spans = torch.full((8,), -9, dtype=torch.int32, device="cuda")
        _ok(sslib, sslib.ss_specaug_packed_device(x.data_ptr(), 1, ro.data_ptr(), M.LONG_ROWS, 39, rng.data_ptr(), 0, LONG_SPEC["n_time"],
                                                  LONG_SPEC["max_time_width"], LONG_SPEC["time_ratio"], LONG_SPEC["n_freq"], LONG_SPEC["max_freq_width"],
                                                  -7.5, out.data_ptr(), d_spans.data_ptr(), None))
        torch.cuda.synchronize()
        spans = d_spans.cpu().numpy().reshape(4, 2)
        assert np.array_equal(spans[None], SM.spans_ref((SEED, EPOCH), 0, [0, M.LONG_ROWS], M.LONG_ROWS, 39, **LONG_SPEC))
        tile = M.long_tile(39)
        _windows_same(out, M.LONG_ROWS, lambda lo, hi: _masked(tile, lo, hi, spans, 2, np.float32(-7.5)), case.name)
        del out, x
        if in_place:
            blocks.drop()  # the block is masked now: the next test makes its own


def test_long_clip_power_to_db(torch, sslib, blocks):
    """top_db < 0: element-wise, so a row's bits are those of the same tile row in a clip of one tile"""
    case = M.CASES["long_power_to_db"]
    with _report(torch, case):
        x, ro, out = _long_block(torch, blocks, 39), _long_table(torch), _long_out(torch)
        small, sro = x[:M.LONG_TILE * 39], _dev(torch, np.array([0, M.LONG_TILE], np.int64))
        want = torch.full((M.LONG_TILE * 39,), NAN, device="cuda")
        _ok(sslib, sslib.ss_power_to_db_packed_device(small.data_ptr(), 1, sro.data_ptr(), M.LONG_TILE, 39, 1.0, 1e-10, -1.0, want.data_ptr(), None))
        _ok(sslib, sslib.ss_power_to_db_packed_device(x.data_ptr(), 1, ro.data_ptr(), M.LONG_ROWS, 39, 1.0, 1e-10, -1.0, out.data_ptr(), None))
        torch.cuda.synchronize()
        w = want.cpu().numpy().reshape(M.LONG_TILE, 39)
        assert not np.isnan(w).any()
        _windows_same(out, M.LONG_ROWS, lambda lo, hi: M.tiled_rows(w, lo, hi), case.name)


def test_long_clip_select_rows(torch, sslib, blocks):
    case = M.CASES["long_select_rows"]
    P, kept = M.LONG_SELECT_PERIOD, M.long_select_kept()
    with _report(torch, case):
        x, ro, out = _long_block(torch, blocks, 39), _long_table(torch), _long_out(torch)
        mask = torch.ones(M.LONG_ROWS, dtype=torch.uint8, device="cuda")
        mask[P - 1::P] = 0
        oo = torch.full((2,), -9, dtype=torch.int64, device="cuda")
        _ok(sslib, sslib.ss_select_rows_packed_device(x.data_ptr(), 1, ro.data_ptr(), M.LONG_ROWS, 39, mask.data_ptr(), oo.data_ptr(), out.data_ptr(), None))
        torch.cuda.synchronize()
        assert oo.cpu().tolist() == [0, kept]
        tile = M.long_tile(39)
        _windows_same(out, kept, lambda lo, hi: tile[M.long_select_source(np.arange(lo, hi)) % M.LONG_TILE], case.name)
        rest_untouched = bool(torch.isnan(out[kept * 39:]).all())  # rows at and past oo[n_clips] are left unwritten
        assert rest_untouched


@pytest.mark.parametrize("layout", ["btc", "bct"])
def test_long_clip_pad(torch, sslib, blocks, layout):
    """max_rows = the clip's rows + 3: the block ends in pad rows.  bct: column 38's run holds element 2^32 of out"""
    import pad_model as PM

    case = M.CASES["long_pad_" + layout]
    mr = M.LONG_ROWS + M.LONG_PAD_EXTRA
    with _report(torch, case):
        x, ro, out = _long_block(torch, blocks, 39), _long_table(torch), _long_out(torch, mr)
        lengths = torch.full((1,), -9, dtype=torch.int32, device="cuda")
        _ok(sslib, sslib.ss_pad_packed_device(x.data_ptr(), 1, ro.data_ptr(), M.LONG_ROWS, 39, mr, PM.LAYOUT_CODE[layout], 0, -2.5, out.data_ptr(),
                                              lengths.data_ptr(), None))
        torch.cuda.synchronize()
        assert lengths.cpu().tolist() == [M.LONG_ROWS]
        tile = M.long_tile(39)

        def rows(lo, hi):  # rows lo .. hi of the padded clip
            w = np.full((hi - lo, 39), np.float32(-2.5))
            live = min(hi, M.LONG_ROWS) - lo
            w[:live] = M.tiled_rows(tile, lo, lo + live)
            return w

        if layout == "btc":
            _windows_same(out, mr, rows, case.name)
        else:
            cross = M.TWO32 - 38 * mr  # t of column 38 at element 2^32
            for c, (lo, hi) in ((0, (0, 64)), (38, (cross - 32, cross + 32)), (38, (mr - 64, mr)), (17, (mr - 64, mr))):
                _same(rows(lo, hi)[:, c], out[c * mr + lo:c * mr + hi].cpu().numpy(), f"{case.name} column {c} t {lo}..{hi}")


def test_long_clip_splice(torch, sslib, blocks):
    import splice_model as SPM

    case = M.CASES["long_splice"]
    with _report(torch, case):
        x, ro, out = _long_block(torch, blocks, 13), _long_table(torch), _long_out(torch)
        _ok(sslib, sslib.ss_splice_packed_device(x.data_ptr(), 1, ro.data_ptr(), M.LONG_ROWS, ro.data_ptr(), M.LONG_ROWS, 13, 1, 1, 1, out.data_ptr(), None))
        torch.cuda.synchronize()
        tile = M.long_tile(13)
        _windows_same(out, M.LONG_ROWS, lambda lo, hi: _local(tile, lo, hi, 1, lambda buf: SPM.splice_ref(buf, 1, 1, 1)), case.name)


def test_long_clip_add_deltas(torch, sslib, blocks):
    from test_add_deltas import restate

    case = M.CASES["long_add_deltas"]
    with _report(torch, case):
        x, ro, out = _long_block(torch, blocks, 13), _long_table(torch), _long_out(torch)
        _ok(sslib, sslib.ss_add_deltas_packed_device(x.data_ptr(), 1, ro.data_ptr(), M.LONG_ROWS, 13, 2, 2, out.data_ptr(), None))
        torch.cuda.synchronize()
        tile = M.long_tile(13)
        _windows_same(out, M.LONG_ROWS, lambda lo, hi: _local(tile, lo, hi, 4, lambda buf: restate(buf, 2, 2)), case.name)
