"""The NeMo / Parakeet front end over a pool of stream states on the device (ss_nstream_*; the pool and flush builds of ss_nemo_c256,
ss_nemo512_pool.hip).

Bit for bit against the dense call of the same handle: however a stream is cut into calls, its pool rows are rows 0 .. K - 1 of
ss_nemo_log_mel_device on zeros(L * 160) ++ stream, and the rows with the first L dropped, followed by the flush rows, are
ss_nemo_log_mel_device on the stream itself; the PCM calls are bit for bit the float calls on the converted samples.  Parity against
the f64 restatement (tests/nemo_model.py): the block metric and the bar of tests/test_nemo.py, 1e-4.  Every output and every pool is
filled with a sentinel first; whatever a call does not own keeps it."""
import ctypes as C
from functools import lru_cache

import numpy as np
import pytest

import nemo_model as nm
import nemo_stream_model as sm
from test_nemo_cpu import BAR, SS_ERR_ARG, SS_ERR_DEVICE, SS_ERR_UNSUPPORTED, SS_OK, make_nemo_params

pytestmark = pytest.mark.gpu
SENTINEL = -7777.0
HOPS = [0, 1, 3, 7, 18]   # the five streams
SLOTS = [5, 0, 3, 6, 1]   # scattered over a 7-row pool; rows 2 and 4 belong to nobody
POOL = 7
WINDOWS = {320: "10", 322: "13", 400: "13", 512: "16"}  # W -> NE: the three builds, L = 0 (320) and L = 1


def dev(a):
    import torch

    return torch.from_numpy(np.array(a, order="C")).cuda()  # (a copy: the shared inputs are read-only)


@lru_cache(maxsize=None)
def stream(k, pcm_scale=None):
    """stream k: seeded noise at 0.1, or (pcm_scale) the int16 samples whose converted form is the float stream"""
    n = HOPS[k] * 160
    if pcm_scale is None:
        x = nm.make_input(n, 500 + k)
    else:
        x = np.clip(np.round(nm.make_input(n, 500 + k) * 0.3 * 32768.0), -32768, 32767).astype(np.int16)
    x.setflags(write=False)
    return x


def converted(k, scale):
    return (stream(k, scale).astype(np.float32) * np.float32(scale)).astype(np.float32)


class Rig:
    """one handle (normalize none) and the raw device calls on it"""

    def __init__(self, ss, sslib, n_mels, W, **kw):
        self.ss, self.lib, self.M, self.W = ss, sslib, n_mels, W
        self.cfg = ss.NemoConfig(make_nemo_params(sslib, n_mels, win_length=W, normalize=0, **kw))
        self.S, self.L = sm.sizes(W)

    def status(self):
        return self.lib.ss_nemo_config_device_status(self.cfg.handle)

    def dense(self, x):
        """ss_nemo_log_mel_device on one clip (numpy float32) -> tensor [len / 160, M]"""
        import torch

        T = len(x) // 160
        out = torch.full((T, self.M), SENTINEL, dtype=torch.float32, device="cuda")
        if T:
            xd = dev(x)
            assert self.lib.ss_nemo_log_mel_device(self.cfg.handle, xd.data_ptr(), 1, len(x), len(x), out.data_ptr(), None) == SS_OK
        torch.cuda.synchronize()
        return out

    def fresh_pool(self, named=()):
        """a pool full of the sentinel, the named rows zero (fresh streams)"""
        import torch

        pool = torch.full((POOL, self.S), SENTINEL, dtype=torch.float32, device="cuda")
        for s in named:
            pool[s] = 0.0
        return pool

    def raw(self, x, so, ro, total_rows, slots, pool, out, scale=None, stream=None, pool_streams=None):
        """the device call as it stands: x a tensor (float32, or int16 with `scale`) or an address, the tables tensors"""
        n = slots.numel()
        ps = pool.shape[0] if pool_streams is None else pool_streams
        xp = x if isinstance(x, int) else x.data_ptr()
        if scale is None:
            return self.lib.ss_nstream_log_mel_packed_device(self.cfg.handle, xp, n, so.data_ptr(), ro.data_ptr(), total_rows, slots.data_ptr(),
                                                             ps, pool.data_ptr(), out.data_ptr(), stream)
        return self.lib.ss_nstream_log_mel_packed_i16_device(self.cfg.handle, xp, n, so.data_ptr(), ro.data_ptr(), total_rows, slots.data_ptr(), ps,
                                                             C.c_float(scale), pool.data_ptr(), out.data_ptr(), stream)

    def call(self, chunks, slots, pool, scale=None, slack=3):
        """one pool call over numpy chunks -> the rows of each entry (tensors); the output's slack rows must keep the sentinel"""
        import torch

        lens = [len(c) for c in chunks]
        so = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        ro = so // 160
        R = int(ro[-1])
        x = dev(np.concatenate(chunks) if chunks else np.zeros(0, np.float32 if scale is None else np.int16))
        if x.numel() == 0:
            x = torch.zeros(2, dtype=x.dtype, device="cuda")  # (an address to hand over: nothing of it is read)
        out = torch.full((R + slack, self.M), SENTINEL, dtype=torch.float32, device="cuda")
        assert self.raw(x, dev(so), dev(ro), R + slack, dev(np.asarray(slots, np.int32)), pool, out, scale) == SS_OK
        torch.cuda.synchronize()
        assert bool((out[R:] == SENTINEL).all()), "rows past ro[n_active] were written"
        return [out[int(ro[i]):int(ro[i + 1])] for i in range(len(chunks))]

    def flush(self, slots, pool, stream=None):
        import torch

        out = torch.full((len(slots) * self.L + 2, self.M), SENTINEL, dtype=torch.float32, device="cuda")
        sl = dev(np.asarray(slots, np.int32))
        assert self.lib.ss_nstream_flush_device(self.cfg.handle, len(slots), sl.data_ptr(), pool.shape[0], pool.data_ptr(), out.data_ptr(), stream) == SS_OK
        torch.cuda.synchronize()
        assert bool((out[len(slots) * self.L:] == SENTINEL).all())
        return out[:len(slots) * self.L]


def schedules():
    """the three cuts -> {name: [call, ...]}, a call = [(stream k, hops), ...]"""
    one = [[(k, HOPS[k]) for k in range(5)]]
    two = [[(k, HOPS[k] // 2) for k in range(5)], [(k, HOPS[k] - HOPS[k] // 2) for k in range(5)]]
    ticks = [[(k, 1 if t < HOPS[k] else 0) for k in range(5)] for t in range(max(HOPS))]  # one-hop calls with R_i = 0 entries
    return {"one_call": one, "two_calls": two, "one_hop_calls": ticks}


def serve(rig, calls, samples, pool, scale_of_call=lambda i: None):
    """runs the calls -> per stream the concatenated rows; samples(k, scale) -> stream k's samples in the call's format"""
    import torch

    at = [0] * 5
    rows = [[torch.empty((0, rig.M), device="cuda")] for _ in range(5)]
    for i, call in enumerate(calls):
        scale = scale_of_call(i)
        chunks = []
        for k, hops in call:
            chunks.append(samples(k, scale)[at[k] * 160:(at[k] + hops) * 160])
            at[k] += hops
        got = rig.call(chunks, [SLOTS[k] for k, _ in call], pool, scale)
        for (k, _), r in zip(call, got):
            rows[k].append(r)
    assert at == HOPS
    return [torch.cat(r) for r in rows]


@pytest.mark.parametrize("cut", ["one_call", "two_calls", "one_hop_calls"])
@pytest.mark.parametrize("n_mels", [80, 128])
@pytest.mark.parametrize("W", list(WINDOWS))
def test_equals_the_dense_call_however_the_stream_is_cut(ss, sslib, W, n_mels, cut):
    import torch

    rig = Rig(ss, sslib, n_mels, W)
    S, L = rig.S, rig.L
    pool = rig.fresh_pool(SLOTS)
    rows = serve(rig, schedules()[cut], lambda k, scale: stream(k), pool)
    assert sslib.ss_last_kernel_name().decode() == f"ss_nemo_c256<{WINDOWS[W]},sp>"
    for k in range(5):
        x = stream(k)
        warm = rig.dense(np.concatenate([np.zeros(L * 160, np.float32), x]))[:HOPS[k]]
        assert rows[k].shape == (HOPS[k], n_mels) and torch.equal(rows[k], warm), (k, "pool rows")
        want_state = np.concatenate([np.zeros(S, np.float32), x])[len(x):]
        np.testing.assert_array_equal(pool[SLOTS[k]].cpu().numpy(), want_state)
    assert bool((pool[[2, 4]] == SENTINEL).all())  # unnamed pool rows
    tail = rig.flush(SLOTS, pool)
    if L:
        assert sslib.ss_last_kernel_name().decode() == f"ss_nemo_c256<{WINDOWS[W]},fl>"
    for k in range(5):
        own = rig.dense(stream(k))
        both = torch.cat([rows[k][L:], tail[k * L:(k + 1) * L]])
        if HOPS[k] >= L:
            assert torch.equal(both[:HOPS[k]], own) and both.shape[0] == HOPS[k] + (L if HOPS[k] == 0 else 0), (k, "rows[L:] ++ flush")
    assert bool((pool[SLOTS] == 0.0).all()) and bool((pool[[2, 4]] == SENTINEL).all())
    assert rig.status() == SS_OK


@pytest.mark.parametrize("n_mels", [80, 128])
@pytest.mark.parametrize("W", list(WINDOWS))
def test_parity_against_the_f64_restatement(ss, sslib, W, n_mels):
    import torch

    rig = Rig(ss, sslib, n_mels, W)
    pool = rig.fresh_pool(SLOTS)
    rows = serve(rig, schedules()["two_calls"], lambda k, scale: stream(k), pool)
    tail = rig.flush(SLOTS, pool)
    worst = {}
    for k in range(1, 5):
        got = torch.cat([rows[k][rig.L:], tail[k * rig.L:(k + 1) * rig.L]]).cpu().numpy()
        worst[HOPS[k]] = nm.block_metric(got, nm.log_mel(stream(k), n_mels, W))
    print(f"nemo stream pool, win_length {W}, {n_mels} bands, rows[L:] ++ flush against f64: " + ", ".join(f"{h} hops: {m:.3g}" for h, m in worst.items()))
    assert max(worst.values()) <= BAR


@pytest.mark.parametrize("scale", [2.0 ** -15, 1.0])
@pytest.mark.parametrize("W,n_mels", [(320, 80), (322, 128), (400, 80), (512, 128)])
def test_pcm_equals_the_float_pool_on_the_converted_samples(ss, sslib, W, n_mels, scale):
    import torch

    rig = Rig(ss, sslib, n_mels, W)
    calls = schedules()["one_hop_calls"]
    samples = lambda k, s: stream(k, scale) if s is not None else converted(k, scale)  # noqa: E731
    pool_f = rig.fresh_pool(SLOTS)
    want = serve(rig, calls, samples, pool_f)
    for name, mode in (("all PCM", lambda i: scale), ("alternating", lambda i: scale if i % 2 == 0 else None)):
        pool = rig.fresh_pool(SLOTS)
        got = serve(rig, calls, samples, pool, mode)
        for k in range(5):
            assert torch.equal(got[k], want[k]), (name, k)
        assert torch.equal(pool, pool_f), name
    # one call of everything: interior quads (raw dwords across the prefetch) next to mixed ones
    pool = rig.fresh_pool(SLOTS)
    got = serve(rig, schedules()["one_call"], samples, pool, lambda i: scale)
    assert sslib.ss_last_kernel_name().decode() == f"ss_nemo_c256<{WINDOWS[W]},spi>"
    for k in range(5):
        assert torch.equal(got[k], want[k]), ("one call", k)
    assert torch.equal(pool, pool_f)
    assert torch.equal(rig.flush(SLOTS, pool), rig.flush(SLOTS, pool_f))
    assert rig.status() == SS_OK


def test_pcm_buffer_at_an_odd_element_offset(ss, sslib):
    """d_x needs 2-byte alignment only: the same chunks at an odd int16 offset of a 4-byte aligned buffer"""
    import torch

    rig = Rig(ss, sslib, 80, 400)
    scale = 2.0 ** -15
    chunks = [stream(k, scale) for k in (3, 4)]
    slots = [SLOTS[3], SLOTS[4]]
    pool_a, pool_b = rig.fresh_pool(slots), rig.fresh_pool(slots)
    want = torch.cat(rig.call(chunks, slots, pool_a, scale, slack=0))
    x = np.concatenate(chunks)
    buf = torch.zeros(x.size + 3, dtype=torch.int16, device="cuda")
    buf[1:1 + x.size] = dev(x)
    assert buf.data_ptr() % 4 == 0
    so = np.asarray([0, len(chunks[0]), x.size], np.int64)
    out = torch.full((25 + 2, 80), SENTINEL, dtype=torch.float32, device="cuda")
    assert rig.raw(buf.data_ptr() + 2, dev(so), dev(so // 160), 27, dev(np.asarray(slots, np.int32)), pool_b, out, scale) == SS_OK
    torch.cuda.synchronize()
    assert torch.equal(out[:25], want) and bool((out[25:] == SENTINEL).all()) and torch.equal(pool_a, pool_b)
    assert rig.raw(buf.data_ptr() + 1, dev(so), dev(so // 160), 27, dev(np.asarray(slots, np.int32)), pool_b, out, scale) == SS_ERR_ARG  # odd byte address


def test_persistent_loop(ss, sslib):
    """64 entries x 200 hops = 3200 quads, more than 12 waves on every CU: every wave goes round the persistent loop again (the LDS
    claim, the prefetch, the carried cursor); bit for bit one dense call per stream"""
    import torch

    cus = int(torch.cuda.get_device_properties(0).multi_processor_count)
    B, T = nm.LOOP_CLIPS, nm.LOOP_FRAMES
    assert (B, T) == (64, 200) and nm.loop_quads() == 3200 > nm.WAVES * cus, "the shape rule of the loop test does not hold on this device"
    rig = Rig(ss, sslib, 128, 400)
    L, S = rig.L, rig.S
    g = torch.Generator(device="cuda")
    g.manual_seed(5)
    x = torch.zeros((B, L * 160 + T * 160), dtype=torch.float32, device="cuda")
    x[:, L * 160:] = torch.randn((B, T * 160), generator=g, device="cuda", dtype=torch.float32).mul_(0.1)
    chunks = x[:, L * 160:].contiguous()
    so = dev(np.arange(B + 1, dtype=np.int64) * (T * 160))
    ro = dev(np.arange(B + 1, dtype=np.int64) * T)
    slots = dev(np.random.default_rng(2).permutation(B).astype(np.int32))
    pool = torch.zeros((B, S), dtype=torch.float32, device="cuda")
    out = torch.full((B * T + 1, 128), SENTINEL, dtype=torch.float32, device="cuda")
    assert rig.raw(chunks.view(-1), so, ro, B * T + 1, slots, pool, out) == SS_OK
    torch.cuda.synchronize()
    assert sslib.ss_last_kernel_name().decode() == "ss_nemo_c256<13,sp>"
    dense = torch.empty((B, T + L, 128), dtype=torch.float32, device="cuda")
    assert sslib.ss_nemo_log_mel_device(rig.cfg.handle, x.data_ptr(), B, x.shape[1], x.shape[1], dense.data_ptr(), None) == SS_OK
    torch.cuda.synchronize()
    assert torch.equal(out[:B * T].view(B, T, 128), dense[:, :T]) and bool((out[B * T:] == SENTINEL).all())
    assert torch.equal(pool[slots.long()], chunks[:, T * 160 - S:])
    own = torch.empty((B, T, 128), dtype=torch.float32, device="cuda")
    assert sslib.ss_nemo_log_mel_device(rig.cfg.handle, chunks.data_ptr(), B, T * 160, T * 160, own.data_ptr(), None) == SS_OK
    tail = rig.flush(slots.cpu().tolist(), pool)
    assert torch.equal(tail, own[:, T - L:].reshape(B * L, 128)) and torch.equal(out[:B * T].view(B, T, 128)[:, L:], own[:, :T - L])
    assert not bool(pool.any()) and rig.status() == SS_OK


@pytest.mark.parametrize("pcm", [False, True], ids=["float", "pcm"])
def test_containment(ss, sslib, pcm):
    """One call with a not-whole-hops entry, an ro mismatch, a slot outside the pool and an entry that ends past total_rows among good
    entries: the good ones are exact, the bad ones leave their rows and pool rows untouched, the handle reports once.  Nothing here
    may fault: the kernels skip, they do not chase."""
    import torch

    rig = Rig(ss, sslib, 80, 400)
    scale = 2.0 ** -15 if pcm else None
    #          good  not whole  good  ro too long  slot outside  good   past total_rows
    lens = [480, 170, 800, 320, 640, 160, 480]
    rows = [3, 1, 5, 3, 4, 1, 3]
    slots = [5, 0, 3, 6, POOL, 1, 2]
    bad = {1, 3, 4, 6}
    assert [n // 160 for n in lens] != rows and lens[1] % 160 and rows[3] != lens[3] // 160
    so = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    ro = np.concatenate([[0], np.cumsum(rows)]).astype(np.int64)
    total_rows = int(ro[-1]) - 1
    if pcm:
        sig = np.clip(np.round(nm.make_input(int(so[-1]), 77) * 9000.0), -32768, 32767).astype(np.int16)
        as_float = (sig.astype(np.float32) * np.float32(scale)).astype(np.float32)
    else:
        sig = as_float = nm.make_input(int(so[-1]), 77)
    pool = torch.full((POOL, rig.S), 0.5, dtype=torch.float32, device="cuda")  # every stream mid-way: a recognisable state
    before = pool.clone()
    out = torch.full((int(ro[-1]) + 2, 80), SENTINEL, dtype=torch.float32, device="cuda")
    assert rig.status() == SS_OK
    assert rig.raw(dev(sig), dev(so), dev(ro), total_rows, dev(np.asarray(slots, np.int32)), pool, out, scale) == SS_OK
    torch.cuda.synchronize()
    assert rig.status() == SS_ERR_DEVICE
    assert rig.status() == SS_OK
    for i in range(len(lens)):
        lo, hi = int(ro[i]), int(ro[i + 1])
        if i in bad:
            assert bool((out[lo:hi] == SENTINEL).all()), i
            if 0 <= slots[i] < POOL:
                assert torch.equal(pool[slots[i]], before[slots[i]]), i
        else:
            clean_pool = before.clone()
            chunk = as_float[int(so[i]):int(so[i + 1])]
            want = rig.call([chunk], [slots[i]], clean_pool)[0]
            assert torch.equal(out[lo:hi], want), i
            assert torch.equal(pool[slots[i]], clean_pool[slots[i]]), i
    assert bool((out[int(ro[-1]):] == SENTINEL).all()) and torch.equal(pool[4], before[4])
    # the flush: a slot outside the pool is skipped and reported; the others are served and zeroed
    fl = torch.full((3, 80), SENTINEL, dtype=torch.float32, device="cuda")
    sl = dev(np.asarray([5, POOL, 3], np.int32))
    keep = pool.clone()
    assert sslib.ss_nstream_flush_device(rig.cfg.handle, 3, sl.data_ptr(), POOL, pool.data_ptr(), fl.data_ptr(), None) == SS_OK
    torch.cuda.synchronize()
    assert rig.status() == SS_ERR_DEVICE and rig.status() == SS_OK
    assert bool((fl[1] == SENTINEL).all()) and bool((fl[[0, 2]] != SENTINEL).all())
    assert not bool(pool[[5, 3]].any()) and torch.equal(pool[[0, 1, 2, 4, 6]], keep[[0, 1, 2, 4, 6]])
    clean = keep.clone()
    assert torch.equal(rig.flush([5, 3], clean), fl[[0, 2]])


def test_argument_rules(ss, sslib):
    import torch

    rig = Rig(ss, sslib, 80, 400)
    x = torch.zeros(320, device="cuda")
    so, ro, sl = dev(np.asarray([0, 320], np.int64)), dev(np.asarray([0, 2], np.int64)), dev(np.zeros(1, np.int32))
    pool = rig.fresh_pool([0])
    before = pool.clone()
    out = torch.full((2, 80), SENTINEL, dtype=torch.float32, device="cuda")
    h, lib = rig.cfg.handle, sslib
    a = dict(x=x.data_ptr(), so=so.data_ptr(), ro=ro.data_ptr(), sl=sl.data_ptr(), pool=pool.data_ptr(), out=out.data_ptr())

    def call(n=1, rows=2, streams=POOL, **nulls):
        p = {**a, **nulls}
        return lib.ss_nstream_log_mel_packed_device(h, p["x"], n, p["so"], p["ro"], rows, p["sl"], streams, p["pool"], p["out"], None)

    assert call(n=0, x=None, so=None, ro=None, sl=None, pool=None, out=None) == SS_OK  # no entries: no launch, no buffers
    for name in a:
        assert call(**{name: None}) == SS_ERR_ARG, name
    assert call(n=2 ** 31) == SS_ERR_ARG and call(rows=2 ** 31) == SS_ERR_ARG and call(streams=2 ** 31) == SS_ERR_ARG and call(streams=0) == SS_ERR_ARG
    assert call(out=pool.data_ptr() + 4 * rig.S) == SS_ERR_ARG  # the output inside the pool
    assert lib.ss_nstream_log_mel_packed_i16_device(h, a["x"], 1, a["so"], a["ro"], 2, a["sl"], POOL, C.c_float(3.0), a["pool"], a["out"], None) == SS_ERR_ARG
    assert lib.ss_nstream_flush_device(h, 0, None, POOL, None, None, None) == SS_OK
    assert lib.ss_nstream_flush_device(h, 1, None, POOL, a["pool"], a["out"], None) == SS_ERR_ARG
    assert lib.ss_nstream_flush_device(h, 1, a["sl"], POOL, None, a["out"], None) == SS_ERR_ARG
    assert lib.ss_nstream_flush_device(h, 1, a["sl"], POOL, a["pool"], None, None) == SS_ERR_ARG
    assert lib.ss_nstream_flush_device(h, 1, a["sl"], 2 ** 31, a["pool"], a["out"], None) == SS_ERR_ARG
    assert lib.ss_nstream_flush_device(h, 1, a["sl"], POOL, a["pool"], pool.data_ptr() + 8, None) == SS_ERR_ARG
    # host forms: the tables are checked first, duplicate slots are refused, the caller's pool is written last
    hx, hso = np.zeros(480, np.float32), np.asarray([0, 160, 480], np.int64)
    hpool, hout = np.full((POOL, rig.S), 3.0, np.float32), np.full((3, 80), SENTINEL, np.float32)
    for bad_so, bad_sl in (([0, 170, 480], [1, 2]), ([0, 320, 160], [1, 2]), (hso, [1, 1]), (hso, [1, POOL])):
        bso, bsl = np.asarray(bad_so, np.int64), np.asarray(bad_sl, np.int32)
        assert lib.ss_nstream_log_mel_packed(h, hx.ctypes.data, 2, bso.ctypes.data, bsl.ctypes.data, POOL, hpool.ctypes.data, hout.ctypes.data) == SS_ERR_ARG
    dup = np.asarray([1, 1], np.int32)
    assert lib.ss_nstream_flush(h, 2, dup.ctypes.data, POOL, hpool.ctypes.data, hout.ctypes.data) == SS_ERR_ARG
    torch.cuda.synchronize()
    assert torch.equal(pool, before) and bool((out == SENTINEL).all()) and (hpool == 3.0).all() and (hout == SENTINEL).all()
    # a per-feature handle: a stream has no clip statistics
    per = ss.NemoConfig(make_nemo_params(sslib, 80))
    assert per.params.normalize == 1
    ph = per.handle
    assert lib.ss_nstream_log_mel_packed_device(ph, a["x"], 1, a["so"], a["ro"], 2, a["sl"], POOL, a["pool"], a["out"], None) == SS_ERR_UNSUPPORTED
    assert lib.ss_nstream_log_mel_packed_i16_device(ph, a["x"], 1, a["so"], a["ro"], 2, a["sl"], POOL, C.c_float(1.0), a["pool"], a["out"], None) == SS_ERR_UNSUPPORTED
    assert lib.ss_nstream_flush_device(ph, 1, a["sl"], POOL, a["pool"], a["out"], None) == SS_ERR_UNSUPPORTED
    sl1 = np.zeros(1, np.int32)
    assert lib.ss_nstream_log_mel_packed(ph, hx.ctypes.data, 1, hso[:2].ctypes.data, sl1.ctypes.data, POOL, hpool.ctypes.data, hout.ctypes.data) == SS_ERR_UNSUPPORTED
    pcm = np.zeros(160, np.int16)
    assert lib.ss_nstream_log_mel_packed_i16(ph, pcm.ctypes.data, 1, hso[:2].ctypes.data, sl1.ctypes.data, POOL, 1.0, hpool.ctypes.data, hout.ctypes.data) == SS_ERR_UNSUPPORTED
    assert lib.ss_nstream_flush(ph, 1, sl1.ctypes.data, POOL, hpool.ctypes.data, hout.ctypes.data) == SS_ERR_UNSUPPORTED
    assert lib.ss_nstream_flush(ph, 0, None, POOL, None, None) == SS_ERR_UNSUPPORTED  # on every call, an empty one included
    torch.cuda.synchronize()
    assert torch.equal(pool, before) and (hpool == 3.0).all() and (hout == SENTINEL).all()


def test_graph_replay_over_changing_tables_equals_eager_calls(ss, sslib):
    """one tick (the pool call) and one flush captured on a side stream, replayed over changed chunks, tables and slots"""
    import torch

    rig = Rig(ss, sslib, 80, 400)
    N, CAP, NF = 5, 24, 2
    x = torch.zeros(CAP * 160, device="cuda")
    d_so, d_ro = torch.zeros(N + 1, dtype=torch.int64, device="cuda"), torch.zeros(N + 1, dtype=torch.int64, device="cuda")
    d_sl = torch.arange(N, dtype=torch.int32, device="cuda")
    d_fl = torch.arange(NF, dtype=torch.int32, device="cuda")
    out = torch.full((CAP, 80), SENTINEL, device="cuda")
    tail = torch.full((NF * rig.L, 80), SENTINEL, device="cuda")
    pool_g = torch.zeros((POOL, rig.S), device="cuda")
    pool_e = pool_g.clone()
    h = rig.cfg.handle

    def tick(pool, stream):
        assert rig.raw(x, d_so, d_ro, CAP, d_sl, pool, out, stream=stream) == SS_OK
        assert sslib.ss_nstream_flush_device(h, NF, d_fl.data_ptr(), POOL, pool.data_ptr(), tail.data_ptr(), stream) == SS_OK

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up outside the capture (the zero tables are N entries without rows)
        tick(pool_g.clone(), side.cuda_stream)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        tick(pool_g, torch.cuda.current_stream().cuda_stream)
    rng = np.random.default_rng(8)
    for k, hops in enumerate(([0, 1, 3, 7, 12], [4, 0, 0, 2, 1], [5, 5, 5, 5, 4])):
        slots = rng.permutation(POOL)[:N].astype(np.int32)
        ends = rng.permutation(POOL)[:NF].astype(np.int32)
        so = np.concatenate([[0], np.cumsum(np.asarray(hops) * 160)]).astype(np.int64)
        xs = nm.make_input(int(so[-1]), 60 + k)
        want = rig.call([xs[int(so[i]):int(so[i + 1])] for i in range(N)], slots.tolist(), pool_e, slack=0)
        want_tail = rig.flush(ends.tolist(), pool_e)
        x[:xs.size] = dev(xs)
        d_so.copy_(dev(so))
        d_ro.copy_(dev(so // 160))
        d_sl.copy_(dev(slots))
        d_fl.copy_(dev(ends))
        out.fill_(SENTINEL)
        tail.fill_(SENTINEL)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        R = int(so[-1]) // 160
        assert torch.equal(out[:R], torch.cat(want)) and bool((out[R:] == SENTINEL).all()), k
        assert torch.equal(tail, want_tail) and torch.equal(pool_g, pool_e), k
    assert rig.status() == SS_OK


@pytest.mark.parametrize("on_device", [False, True], ids=["numpy", "tensors"])
def test_python_front(ss, on_device):
    import torch

    put = dev if on_device else (lambda a: a)
    host = (lambda t: t.cpu().numpy()) if on_device else (lambda a: a)
    xs = [nm.make_input(h * 160, 900 + i) for i, h in enumerate((6, 9, 4))]
    want = [host(ss.nemo_log_mel(put(x), n_mels=80, normalize="none")) for x in xs]
    pool = ss.NemoLogMelStreamPool(6)
    assert (pool.state_len, pool.delay_rows, pool.hop) == (361, 1, 160)
    slots = [4, 1, 3]
    # call 1: a packed buffer with lengths; call 2: a list of chunks; call 3: PCM on stream 0 next to an empty entry
    first = [x[:320] for x in xs]
    r1, ro1 = pool(put(np.concatenate(first)), [320, 320, 320], slots)
    assert ro1.tolist() == [0, 2, 4, 6] and pool.state.shape == (6, 361)
    r2, ro2 = pool([put(x[320:]) for x in xs[1:]], None, slots[1:])
    assert ro2.tolist() == [0, 7, 9]
    rest = xs[0][320:]
    pcm = np.round(rest * 32768.0).astype(np.int16)
    r3, ro3 = pool(put(pcm), [0, pcm.size, 0], [0, 4, 5], pcm_scale=2.0 ** -15)
    assert ro3.tolist() == [0, 0, 4, 4]
    tail = host(pool.flush(slots))
    assert tail.shape == (3, 80)
    r1, r2, r3 = host(r1), host(r2), host(r3)
    np.testing.assert_array_equal(np.concatenate([r1[2:4], r2[0:7]])[1:], want[1][:-1])
    np.testing.assert_array_equal(np.concatenate([r1[4:6], r2[7:9]])[1:], want[2][:-1])
    np.testing.assert_array_equal(tail[1], want[1][-1])
    np.testing.assert_array_equal(tail[2], want[2][-1])
    # stream 0: its float head is exact; the PCM tail is another signal (rounded samples) -- the float pool on the converted samples
    np.testing.assert_array_equal(r1[1], want[0][0])
    ref = ss.NemoLogMelStreamPool(6)
    ref(put(xs[0][:320]), [320], [4])
    r3_ref, _ = ref(put((pcm.astype(np.float32) * np.float32(2.0 ** -15)).astype(np.float32)), [pcm.size], [4])
    np.testing.assert_array_equal(r3, host(r3_ref))
    np.testing.assert_array_equal(tail[0], host(ref.flush([4]))[0])
    assert not bool(host(pool.state)[slots].any())  # flushed slots are fresh
    # reset: a slot mid-stream becomes a fresh stream
    pool(put(xs[1][:480]), [480], [2])
    pool.reset([2])
    again, _ = pool(put(xs[1]), [xs[1].size], [2])
    np.testing.assert_array_equal(host(again)[1:], want[1][:-1])
    pool.reset()
    assert not bool(host(pool.state).any())
    if on_device:
        assert isinstance(r1, np.ndarray) and isinstance(pool.state, torch.Tensor)
