"""The plumbing of the Python front that needs no device: what the five side-stage pools (CmvnStreamPool, AddDeltasStreamPool,
SpliceStreamPool, VadEnergyStreamPool, ResampleStreamPool) hand to their ``ss_*_stream_packed`` / ``ss_*_stream_flush`` entry
points on the numpy path, and when their state, place and counter move; and the release of the five handle owners.  The library
is a proxy around the real one that records the pool calls and answers them with a chosen status, so nothing reaches a device.
The expected argument lists are written out from include/speechsauce_amd.h."""
import ctypes as C
import gc

import numpy as np
import pytest

POOL, COLS = 4, 3
X, TABLE, SLOTS, STATE, OUT, HANDLE = "x", "table", "slots", "state", "out", "handle"  # the pointers of an expected argument list
SS_ERR_HIP = 4
FAKE = 0xF00D0  # the handle a faked create call hands out


class Proxy:
    """The real library, except that a pool call is recorded as (name, args) and answered with ``status``, a name in ``fail`` returns
    SS_ERR_HIP without being called, a create call in ``fake`` hands out FAKE without being called, and a ``*_destroy`` is counted
    on its way through (FAKE goes no further; with ``broken_destroy`` it raises)."""

    def __init__(self, real, status=0):
        self.real, self.status, self.fail, self.fake, self.broken_destroy = real, status, set(), set(), False
        self.calls, self.destroyed = [], []

    def __getattr__(self, name):
        fn = getattr(self.real, name)
        if "_stream_packed" in name or "_stream_flush" in name:
            def recorded(*args):
                self.calls.append((name, args))
                return self.status
            return recorded
        if name in self.fail:
            return lambda *args: SS_ERR_HIP
        if name in self.fake:
            def create(*args):
                args[-1]._obj.value = FAKE  # (the last argument of every create call: byref of the handle)
                return 0
            return create
        if name.endswith("_destroy"):
            def destroy(h):
                if self.broken_destroy:
                    raise OSError("destroy failed")
                self.destroyed.append((name, h.value))
                return None if h.value == FAKE else fn(h)
            return destroy
        return fn


@pytest.fixture
def front(sslib, monkeypatch):
    """(the front, the proxy it runs on); the memoised handles are dropped on the way in and out, as for any change of library"""
    import speechsauce_amd as ss
    from speechsauce_amd import _lib

    proxy = Proxy(sslib)
    for cb in _lib._on_switch:
        cb()
    monkeypatch.setattr(_lib, "lib", lambda: proxy)
    yield ss, proxy
    for cb in _lib._on_switch:
        cb()


# name -> (constructor arguments, the counter, rows or samples of the full entry, what it adds to the counter, the scalars between
# pool_streams and the state in the packed call, those of the flush, the output shape of the full entry, the flush shape per slot)
ROW_POOLS = {
    "CmvnStreamPool": (dict(win_size=5, variance_normalization=True), None, 4, None, (COLS, 5, 1), None, (4, COLS), None),
    "AddDeltasStreamPool": (dict(order=2, window=3), "rows_seen", 4, 4, (COLS, 2, 3), (COLS, 2, 3), (4, 3 * COLS), (6, 3 * COLS)),
    "SpliceStreamPool": (dict(left=1, right=2, stride=2), "rows_seen", 4, 4, (COLS, 1, 2, 2), (COLS, 1, 2, 2), (2, 4 * COLS), (1, 4 * COLS)),
    "VadEnergyStreamPool": (dict(energy_col=1, energy_threshold=5.5, energy_mean_scale=0.25, frames_context=2, proportion_threshold=0.5),
                            "rows_seen", 4, 4, (COLS, 1, 5.5, 0.25, 2, 0.5), (5.5, 0.25, 2, 0.5), (4,), (2,)),
}
STEMS = {"CmvnStreamPool": "cmvn", "AddDeltasStreamPool": "add_deltas", "SpliceStreamPool": "splice", "VadEnergyStreamPool": "vad_energy",
         "ResampleStreamPool": "resample"}
STATE_LENS = {"CmvnStreamPool": 4 * COLS + 1, "AddDeltasStreamPool": 2 * 6 * COLS + 1, "SpliceStreamPool": (1 * 2 + 1) * COLS + 1,
              "VadEnergyStreamPool": 2 * 2 + 4}
CASES = list(ROW_POOLS) + ["ResampleStreamPool", "ResampleStreamPool-i16"]


class Case:
    """One pool with the inputs of its case: a block of one full and one empty entry for slots [2, 0]."""

    def __init__(self, ss, case):
        self.name = case.split("-")[0]
        self.i16 = case.endswith("-i16")
        self.stem = STEMS[self.name]
        if self.name == "ResampleStreamPool":
            self.pool = ss.ResampleStreamPool(POOL, 44100, 16000)
            self.counter, self.full, self.moves = "periods_seen", 441, 1
            self.scalars, self.flush_scalars = ((2.0 ** -15,) if self.i16 else ()), ()
            assert (self.pool.period_in, self.pool.period_out) == (441, 160)
            self.out_shape, self.flush_per_slot, self.dtype = (160,), None, np.float32
            self.block = np.arange(441, dtype=np.int16) if self.i16 else np.linspace(-1, 1, 441, dtype=np.float32)
            self.kw = dict(pcm_scale=2.0 ** -15) if self.i16 else {}
            self.handle = ss._get_resampler(44100, 16000, 6, 0.99, ss._device_key(self.block)).handle.value
            self.state_len = self.pool.state_len
            self.empty_shape = (0,)
        else:
            args, self.counter, self.full, self.moves, self.scalars, self.flush_scalars, self.out_shape, self.flush_per_slot = ROW_POOLS[self.name]
            self.pool = getattr(ss, self.name)(POOL, COLS, **args)
            self.dtype = np.uint8 if self.name == "VadEnergyStreamPool" else np.float32
            self.block = np.arange(4 * COLS, dtype=np.float32).reshape(4, COLS)
            self.kw, self.handle = {}, None
            self.state_len = STATE_LENS[self.name]
            self.empty_shape = (0,) + self.out_shape[1:]
        self.table = np.array([0, self.full, self.full], np.int64)

    def call(self, block=None, table=None, slots=(2, 0)):
        return self.pool(self.block if block is None else block, self.table if table is None else table, list(slots), **self.kw)

    def flush_shape(self, n_active):
        if self.name == "ResampleStreamPool":
            return (n_active, self.pool.lag)
        return (n_active * self.flush_per_slot[0],) + self.flush_per_slot[1:]

    def seen(self):
        return getattr(self.pool, self.counter).tolist() if self.counter else None

    def expect_packed(self):
        """the host form: [rs,] vec, n_active, offsets, slots, pool_streams, scalars.., pool, out"""
        head = (HANDLE,) if self.handle is not None else ()
        return head + (X, 2, TABLE, SLOTS, POOL) + self.scalars + (STATE, OUT)

    def expect_flush(self, n_active):
        """the host form: [rs,] n_active, slots, pool_streams, scalars.., pool, out"""
        head = (HANDLE,) if self.handle is not None else ()
        return head + (n_active, SLOTS, POOL) + self.flush_scalars + (STATE, OUT)

    def check(self, args, expected, out, table=None):
        assert len(args) == len(expected), (args, expected)
        where = {X: self.block.ctypes.data, TABLE: (self.table if table is None else table).ctypes.data, STATE: self.pool.state.ctypes.data,
                 OUT: out.ctypes.data, HANDLE: self.handle}
        for i, (got, want) in enumerate(zip(args, expected)):
            if want == SLOTS:
                assert isinstance(got, int) and got not in (0, where[STATE], where[OUT]), i  # a temporary of the call: an address
            elif isinstance(want, str):
                assert (got.value if isinstance(got, C.c_void_p) else got) == where[want], (i, want)
            else:
                assert type(got) is type(want) and got == want, (i, got, want)


@pytest.mark.parametrize("case", CASES)
def test_a_call_that_went_through(front, case):
    ss, proxy = front
    c = Case(ss, case)
    assert c.pool.state is None and c.pool.state_len == c.state_len
    out = c.call()
    (name, args), = proxy.calls
    assert name == f"ss_{c.stem}_stream_packed" + ("_i16" if c.i16 else "")
    c.check(args, c.expect_packed(), out)
    assert isinstance(out, np.ndarray) and out.shape == c.out_shape and out.dtype == c.dtype
    assert isinstance(c.pool.state, np.ndarray) and c.pool.state.shape == (POOL, c.state_len) and c.pool.state.dtype == np.float32
    assert not c.pool.state.any()
    if c.counter is None:
        assert not hasattr(c.pool, "flush") and not hasattr(c.pool, "rows_seen")
        return
    assert c.seen() == [0, 0, c.moves, 0]  # slot 2 brought the full entry, slot 0 the empty one
    c.call(slots=(0, 2))
    assert c.seen() == [c.moves, 0, c.moves, 0] and len(proxy.calls) == 2
    state = c.pool.state
    flushed = c.pool.flush([2])
    (name, args) = proxy.calls[2]
    assert name == f"ss_{c.stem}_stream_flush" and len(proxy.calls) == 3
    c.check(args, c.expect_flush(1), flushed)
    assert flushed.shape == c.flush_shape(1) and flushed.dtype == c.dtype and not flushed.any()  # a host pool's flush starts from zeros
    assert c.seen() == [c.moves, 0, 0, 0] and c.pool.state is state
    c.pool.reset([0])
    assert c.seen() == [0, 0, 0, 0]


@pytest.mark.parametrize("case", CASES)
def test_a_failed_first_call_leaves_the_pool_as_it_was(front, case):
    ss, proxy = front
    c = Case(ss, case)
    proxy.status = SS_ERR_HIP
    with pytest.raises(ss.SpeechSauceError) as e:
        c.call()
    assert e.value.status == SS_ERR_HIP and len(proxy.calls) == 1
    assert c.pool.state is None and c.pool._where is None  # not allocated, not placed
    assert c.seen() in (None, [0, 0, 0, 0])
    proxy.status = 0
    out = c.call()  # ... so a later host call is taken
    assert out.shape == c.out_shape and c.pool.state.shape == (POOL, c.state_len) and c.seen() in (None, [0, 0, c.moves, 0])
    proxy.status = SS_ERR_HIP  # and a failed later call moves nothing either
    state = c.pool.state
    with pytest.raises(ss.SpeechSauceError):
        c.call(slots=(0, 2))
    assert c.pool.state is state and c.seen() in (None, [0, 0, c.moves, 0])
    if c.counter:
        with pytest.raises(ss.SpeechSauceError):
            c.pool.flush([2])
        assert c.seen() == [0, 0, c.moves, 0]


@pytest.mark.parametrize("case", CASES)
def test_nothing_to_serve_launches_nothing_and_still_places_the_pool(front, case):
    ss, proxy = front
    c = Case(ss, case)
    out = c.call(block=c.block[:0], table=np.zeros(1, np.int64), slots=())
    assert proxy.calls == []
    assert out.shape == c.empty_shape and out.dtype == c.dtype
    assert isinstance(c.pool.state, np.ndarray) and c.pool.state.shape == (POOL, c.state_len) and c.pool._where == ("host",)
    assert c.seen() in (None, [0, 0, 0, 0])
    out = c.call(block=c.block[:0], table=np.zeros(3, np.int64))  # two entries, both empty: nothing to launch either
    assert proxy.calls == [] and out.shape == c.empty_shape and c.seen() in (None, [0, 0, 0, 0])


@pytest.mark.parametrize("case", CASES)
def test_which_argument_is_decided_first(front, case):
    """a table that decreases and overruns the block, and a slot outside the pool, in one call"""
    ss, proxy = front
    c = Case(ss, case)
    bad = np.array([0, 2 * c.full, c.full], np.int64)
    with pytest.raises(ValueError) as e:
        c.call(table=bad, slots=(2, 7))
    if c.name == "CmvnStreamPool":
        assert str(e.value) == "CmvnStreamPool: row_offsets must start at 0, not decrease and end within the block's 4 rows"
    else:
        assert str(e.value) == f"{c.name}: slot 7 of entry 1 is outside the pool of 4 streams"
    with pytest.raises(ValueError) as e:  # the table alone
        c.call(table=bad)
    noun = "samples" if c.name == "ResampleStreamPool" else "rows"
    table = "sample_offsets" if c.name == "ResampleStreamPool" else "row_offsets"
    assert str(e.value) == f"{c.name}: {table} must start at 0, not decrease and end within the block's {c.full} {noun}"
    assert proxy.calls == [] and c.pool.state is None and c.pool._where is None


def test_an_entry_that_is_no_whole_period(front):
    ss, proxy = front
    pool = ss.SpliceStreamPool(POOL, COLS, 1, 2, 2)
    with pytest.raises(ValueError) as e:
        pool(np.zeros((4, COLS), np.float32), [0, 3, 4], [2, 0])
    assert str(e.value) == "SpliceStreamPool: every entry must bring whole periods of 2 rows"
    pool = ss.ResampleStreamPool(POOL, 44100, 16000)
    with pytest.raises(ValueError) as e:
        pool.push(np.zeros(441, np.float32), [0, 440, 441], [2, 0])
    assert str(e.value) == "ResampleStreamPool: every entry must bring whole periods of 441 samples"
    with pytest.raises(ValueError) as e:  # decided after the table ...
        pool.push(np.zeros(441, np.float32), [0, 440, 442], [2, 0])
    assert "sample_offsets must start at 0" in str(e.value)
    assert proxy.calls == [] and pool.state is None and pool._where is None and not pool.periods_seen.any()
    assert ss.ResampleStreamPool.__call__ is ss.ResampleStreamPool.push


@pytest.mark.parametrize("case", [c for c in CASES if c != "CmvnStreamPool"])
def test_flush_before_any_call(front, case):
    ss, proxy = front
    c = Case(ss, case)
    out = c.pool.flush([2, 0])
    assert isinstance(out, np.ndarray) and out.shape == c.flush_shape(2) and out.dtype == c.dtype and not out.any()
    assert proxy.calls == [] and c.pool.state is None and c.seen() == [0, 0, 0, 0]
    with pytest.raises(ValueError, match="slot 4 of entry 0 is outside the pool"):
        c.pool.flush([4])
    with pytest.raises(ValueError, match="slot 4 of entry 0 is outside the pool"):
        c.pool.reset([4])
    assert c.pool.flush([]).shape == c.flush_shape(0)


def test_cmvn_reset_before_the_first_call_looks_at_nothing(front):
    ss, proxy = front
    pool = ss.CmvnStreamPool(POOL, COLS, win_size=5)
    assert pool.reset([99]) is None and pool.reset() is None and pool.state is None
    pool(np.ones((4, COLS), np.float32), [0, 4, 4], [2, 0])
    pool.state[:] = 1
    pool.reset([-1])  # once there is a state the index is numpy's business, not the slot rule's
    assert pool.state[3].tolist() == [0] * pool.state_len and pool.state[:3].all()
    pool.reset()
    assert not pool.state.any()


# ---- the handle owners -----------------------------------------------------------------------------------------------------------

def _kaldi_params(ss, lib):
    p = ss.SsKaldiParams()
    assert lib.ss_kaldi_params_default(C.byref(p), 16000) == 0
    return p


def _owners(ss, lib):
    """name of the create call -> (name of the destroy call, the owner's class, its constructor arguments)"""
    return {
        "ss_config_create": ("ss_config_destroy", ss.SpeechConfig, (ss.make_params(),)),
        "ss_resampler_create": ("ss_resampler_destroy", ss.Resampler, (44100, 16000)),
        "ss_kaldi_config_create": ("ss_kaldi_config_destroy", ss.KaldiConfig, (_kaldi_params(ss, lib),)),
        "ss_whisper_config_create": ("ss_whisper_config_destroy", ss.WhisperConfig, (80,)),
        "ss_affine_create": ("ss_affine_destroy", ss.Affine, (np.arange(6, dtype=np.float32).reshape(2, 3),)),
    }


def _build(ss, proxy, create, cls, args):
    """The owner.  A handle that keeps tables in device memory cannot be created without a device: there the create call is faked,
    which leaves everything of the owner but the library's own work to run."""
    try:
        return cls(*args)
    except ss.SpeechSauceError as e:
        assert e.status == SS_ERR_HIP and cls not in (ss.Resampler, ss.Affine)  # (these two are built on the host)
    proxy.fake = {create}
    try:
        return cls(*args)
    finally:
        proxy.fake = set()


def test_every_owner_releases_its_handle_once(front):
    ss, proxy = front
    for create, (destroy, cls, args) in _owners(ss, proxy).items():
        obj = _build(ss, proxy, create, cls, args)
        h = obj.handle.value
        assert h and obj._owner is proxy and proxy.destroyed == []
        obj.__del__()  # (called by hand: an exception would surface here)
        assert proxy.destroyed == [(destroy, h)] and obj.handle is None
        del obj
        gc.collect()
        assert proxy.destroyed == [(destroy, h)], create  # the collector's call finds nothing left to release
        proxy.destroyed.clear()
    rs = ss._get_resampler(44100, 16000)  # a memoised one: released when the cache lets go of it
    h = rs.handle.value
    assert ss._get_resampler(44100, 16000) is rs
    del rs
    gc.collect()
    assert proxy.destroyed == []
    ss._get_resampler.cache_clear()
    gc.collect()
    assert proxy.destroyed == [("ss_resampler_destroy", h)]
    cfg = _build(ss, proxy, "ss_config_create", ss._get_speech_config, (16000,))
    h = cfg.handle.value
    assert ss._get_speech_config(16000) is cfg
    del cfg
    ss._get_speech_config.cache_clear()
    gc.collect()
    assert proxy.destroyed[1:] == [("ss_config_destroy", h)]


def test_a_half_built_owner_and_a_failing_destroy_do_not_raise(front):
    ss, proxy = front
    for create, (destroy, cls, args) in _owners(ss, proxy).items():
        cls.__new__(cls).__del__()  # not even __init__ has run
        proxy.fail = {create}
        obj = cls.__new__(cls)
        with pytest.raises(ss.SpeechSauceError) as e:
            obj.__init__(*args)
        assert e.value.status == SS_ERR_HIP
        obj.__del__()  # (called by hand: an exception would surface here)
        assert proxy.destroyed == [] and obj.handle is None, create  # the create call filled nothing in: nothing to release
        proxy.fail = set()
        obj = _build(ss, proxy, create, cls, args)
        assert obj.handle.value
        proxy.broken_destroy = True
        obj.__del__()
        proxy.broken_destroy = False
        assert obj.handle is None
    gc.collect()
    assert proxy.destroyed == []
