"""Ragged streaming MFCC / mfe over a pool of stream states: ss_frame_stream_packed_row_offsets, ss_mfcc_stream_packed /
ss_mfe_stream_packed (host pointers), their *_device forms, and the Python front's MfccStreamPool / MfeStreamPool.

A pool is the [pool_streams x S] state block of the dense streaming calls.  One call serves n_active entries; entry i is the chunk
x[so[i] : so[i+1]] (R_i whole hops, R_i = 0 allowed) of the stream whose state is pool row slots[i], and its rows are rows
ro[i] .. ro[i+1] of the packed output.  Per entry the rows and the pool row afterwards are what the dense streaming call gives for
that stream alone.  Expected values come from the dense streaming calls (tests/test_frame_stream.py checks those against the
one-shot calls and the oracle) and from the f64 oracle, never from the ragged calls themselves.
"""
import ctypes as C

import numpy as np
import pytest

from common import RTOL, rel

POOL_KERNEL = b"ss_mfcc_c256sp<10,exact,bank421,sym>"
POOL_MFE_KERNEL = b"ss_mfcc_c256sp<10,exact,bank421,mfe>"
GENERIC_POOL_PREFIX = b"ss_front_generic_fstreamp<"

# the configurations of tests/test_frame_stream.py's SWEEP: everything but the default shape runs on the generic kernel
SWEEP = {
    "fft1024": dict(fft_points=1024, frame_length=0.025, frame_stride=0.01),
    "fft4096": dict(sample_rate=44100, fft_points=4096, frame_length=4096 / 44100, frame_stride=1024 / 44100, num_cepstral=40,
                    num_filters=256, high_frequency=22050.0),
    "chirpz": dict(fft_points=400, frame_length=0.025, frame_stride=0.01),
    "hann": dict(mfcc_window="hann"),
    "preemph1": dict(preemph_coef=0.97, preemph_shift=1),
    "preemph_step": dict(preemph_coef=0.97, preemph_shift=160),
    "ortho": dict(dct_norm="ortho"),
    "slaney": dict(fft_points=1024, mel_scale="slaney", mel_norm="slaney"),
    "padded": dict(framing="padded", fft_points=1024, frame_length=0.025),
    "flen_eq_step": dict(frame_length=0.01, frame_stride=0.01),
    "flen_lt_step": dict(frame_length=0.01, frame_stride=0.02),
}


def _sizes(sslib, p):
    fl, st, S = C.c_size_t(), C.c_size_t(), C.c_size_t()
    assert sslib.ss_frame_sizes(C.byref(p), C.byref(fl), C.byref(st)) == 0
    rc = sslib.ss_frame_stream_state_len(C.byref(p), C.byref(S))
    return rc, fl.value, st.value, S.value


def _row_offsets(sslib, p, so):
    so = np.asarray(so, dtype=np.int64)
    ro = np.full(so.size, -1, dtype=np.int64)
    rc = sslib.ss_frame_stream_packed_row_offsets(C.byref(p), so.size - 1, so.ctypes.data, ro.ctypes.data)
    return rc, ro


# ---------------------------------------------------------------- CPU ---------------------------------------------------------

def test_row_offsets_follow_the_formula(sslib):
    from speechsauce_amd import _lib

    p = _lib.make_params()  # step 160
    rc, ro = _row_offsets(sslib, p, [0, 320, 320, 480, 480, 480, 1280])
    assert rc == 0 and ro.tolist() == [0, 2, 2, 3, 3, 3, 8]
    rc, ro = _row_offsets(sslib, p, [0, 0, 0])  # nothing but entries without rows
    assert rc == 0 and ro.tolist() == [0, 0, 0]
    rc, ro = _row_offsets(sslib, p, [0])  # no entries
    assert rc == 0 and ro.tolist() == [0]
    p2 = _lib.make_params(frame_length=0.025, frame_stride=0.015)  # step 240
    rc, ro = _row_offsets(sslib, p2, [0, 240, 960, 960])
    assert rc == 0 and ro.tolist() == [0, 1, 4, 4]


def test_row_offsets_rejections(sslib):
    from speechsauce_amd import _lib

    p = _lib.make_params()
    assert _row_offsets(sslib, p, [160, 320])[0] == 3  # so[0] != 0
    assert _row_offsets(sslib, p, [0, 320, 160])[0] == 3  # a decreasing pair
    assert b"entry 1" in sslib.ss_last_error_string()
    assert _row_offsets(sslib, p, [0, 160, 330])[0] == 3  # not whole hops
    assert b"entry 1" in sslib.ss_last_error_string()
    assert _row_offsets(sslib, p, [0, 160 * (1 << 24)])[0] == 3  # longer than 2^31 - 1 samples
    so = np.zeros(2, np.int64)
    ro = np.zeros(2, np.int64)
    assert sslib.ss_frame_stream_packed_row_offsets(None, 1, so.ctypes.data, ro.ctypes.data) == 3
    assert sslib.ss_frame_stream_packed_row_offsets(C.byref(p), 1, None, ro.ctypes.data) == 3
    assert sslib.ss_frame_stream_packed_row_offsets(C.byref(p), 1, so.ctypes.data, None) == 3
    for framing in ("literal", "center"):  # a stream has no clip end
        assert _row_offsets(sslib, _lib.make_params(framing=framing), [0, 160])[0] == 2
    assert _row_offsets(sslib, _lib.make_params(framing="padded"), [0, 160, 480])[0] == 0


def test_compute_entries_reject_a_null_config(sslib):
    assert sslib.ss_mfcc_stream_packed_device(None, None, 1, None, None, 1, None, 1, 1, None, None, None) == 3
    assert sslib.ss_mfe_stream_packed_device(None, None, 1, None, None, 1, None, 1, None, None, None, None) == 3
    assert sslib.ss_mfcc_stream_packed(None, None, 1, None, None, 1, 1, None, None) == 3
    assert sslib.ss_mfe_stream_packed(None, None, 1, None, None, 1, None, None, None) == 3


def _has_gpu():
    try:
        import torch

        return torch.cuda.is_available()
    except Exception:
        return False


@pytest.mark.skipif(_has_gpu(), reason="checks the no-device failure mode")
def test_python_classes_fail_loudly_without_a_device(sslib):
    import speechsauce_amd as ss
    from speechsauce_amd import SpeechSauceError

    for obj in (ss.MfccStreamPool(4, 16000, norm_frames=100), ss.MfeStreamPool(4, 16000)):
        with pytest.raises(SpeechSauceError) as e:
            obj([np.zeros(320, np.float32), np.zeros(0, np.float32)], [2, 0])
        assert e.value.status == 4
        assert obj.state is None


def test_python_argument_rules(sslib):
    import speechsauce_amd as ss

    m = ss.MfccStreamPool(4, 16000, norm_frames=101)
    assert m.hop == 160 and m.frame_len == 320 and m.state_len == 160 and m.state is None and m.norm_frames == 101
    assert m.pool_streams == 4
    z = lambda n, dt=np.float32: np.zeros(n, dt)  # noqa: E731
    with pytest.raises(TypeError):
        m([z(320, np.float64)], [0])  # wrong dtype
    with pytest.raises(ValueError):
        m([z(330)], [0])  # a partial hop
    with pytest.raises(ValueError):
        m([z(320), z(160)], [1, 1])  # a slot named twice
    with pytest.raises(ValueError):
        m([z(320)], [4])  # a slot outside the pool
    with pytest.raises(ValueError):
        m([z(320)], [-1])
    with pytest.raises(ValueError):
        m([z(320), z(160)], [1])  # len(chunks) != len(slots)
    with pytest.raises(ValueError):
        m(z(480), [0, 1], lengths=[320, 320])  # lengths do not add up to the packed buffer
    with pytest.raises(ValueError):
        m([np.zeros((2, 160), np.float32)], [0])  # chunks are 1-D
    with pytest.raises(TypeError):
        m(z(320), [0])  # a packed buffer needs lengths
    assert m.state is None  # nothing was created by the rejected calls
    m.reset()
    m.reset(slots=[1])  # no state yet: nothing to do
    with pytest.raises(ValueError):
        ss.MfccStreamPool(4, 16000)  # the reference DCT scaling needs norm_frames
    with pytest.raises(ValueError):
        ss.MfccStreamPool(4, 16000, norm_frames=0)
    assert ss.MfccStreamPool(1, 16000, dct_norm="ortho").state_len == 160
    with pytest.raises(ValueError):
        ss.MfeStreamPool(0, 16000)
    with pytest.raises(ss.SpeechSauceError) as e:
        ss.MfccStreamPool(2, 16000, norm_frames=10, framing="center")
    assert e.value.status == 2
    assert ss.MfeStreamPool(3, 16000, preemph_coef=0.97).state_len == 161
    assert "MfccStreamPool" in ss.__all__ and "MfeStreamPool" in ss.__all__


# ---------------------------------------------------------------- GPU ---------------------------------------------------------

def _cfg(ss, **kw):
    from speechsauce_amd import _lib

    return ss.SpeechConfig(_lib.make_params(**kw))


def _gsig(torch, shape, seed):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    return torch.randn(shape, generator=g, device="cuda", dtype=torch.float32).mul_(0.1)


def _dense(torch, lib, cfg, x, state, norm_frames, fn="mfcc"):
    """One ss_mfcc_stream_device / ss_mfe_stream_device call on [B, n] x (the expected values); state is updated in place."""
    B, n = x.shape
    r = C.c_size_t()
    assert lib.ss_frame_stream_rows(C.byref(cfg.params), n, C.byref(r)) == 0
    R = r.value
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    sp = state.data_ptr() if state is not None and state.numel() else None
    ld = x.stride(0) if B > 1 else n
    if fn == "mfcc":
        out = torch.full((B, R, cfg.params.num_cepstral), float("nan"), device="cuda")
        rc = lib.ss_mfcc_stream_device(cfg.handle, x.data_ptr(), B, n, ld, norm_frames, sp, out.data_ptr(), st)
        assert rc == 0, lib.ss_last_error_string()
        return (out,)
    feat = torch.full((B, R, cfg.params.num_filters), float("nan"), device="cuda")
    en = torch.full((B, R), float("nan"), device="cuda")
    rc = lib.ss_mfe_stream_device(cfg.handle, x.data_ptr(), B, n, ld, sp, feat.data_ptr(), en.data_ptr(), st)
    assert rc == 0, lib.ss_last_error_string()
    return feat, en


def _alloc_outs(torch, cfg, rows, fn, fill=float("nan")):
    if fn == "mfcc":
        return (torch.full((rows, cfg.params.num_cepstral), fill, device="cuda"),)
    return torch.full((rows, cfg.params.num_filters), fill, device="cuda"), torch.full((rows,), fill, device="cuda")


def _raw_call(torch, lib, cfg, x, n_active, so, ro, total_rows, slots, pool_streams, pool, norm_frames, outs, fn="mfcc", stream=None):
    """The device entry on device tables as they are; returns its status."""
    st = C.c_void_p(stream if stream is not None else torch.cuda.current_stream().cuda_stream)
    pp = pool.data_ptr() if pool is not None and pool.numel() else None
    if fn == "mfcc":
        return lib.ss_mfcc_stream_packed_device(cfg.handle, x.data_ptr(), n_active, so.data_ptr(), ro.data_ptr(), total_rows, slots.data_ptr(),
                                                pool_streams, norm_frames, pp, outs[0].data_ptr(), st)
    return lib.ss_mfe_stream_packed_device(cfg.handle, x.data_ptr(), n_active, so.data_ptr(), ro.data_ptr(), total_rows, slots.data_ptr(),
                                           pool_streams, pp, outs[0].data_ptr(), outs[1].data_ptr(), st)


def _pool_call(torch, lib, cfg, chunks, slots, pool, pool_streams, norm_frames, fn="mfcc"):
    """One ragged call on a list of 1-D device chunks; returns (outs, ro) with ro the host row offsets."""
    _, _, step, _ = _sizes(lib, cfg.params)
    lens = [int(c.numel()) for c in chunks]
    so = np.zeros(len(lens) + 1, np.int64)
    np.cumsum(lens, out=so[1:])
    rc, ro = _row_offsets(lib, cfg.params, so)
    assert rc == 0, lib.ss_last_error_string()
    x = torch.cat(list(chunks)) if so[-1] else torch.zeros(1, device="cuda")
    outs = _alloc_outs(torch, cfg, int(ro[-1]), fn)
    d_so, d_ro = torch.from_numpy(so).cuda(), torch.from_numpy(ro).cuda()
    d_sl = torch.tensor(list(slots), dtype=torch.int32, device="cuda")
    rc = _raw_call(torch, lib, cfg, x, len(lens), d_so, d_ro, int(ro[-1]), d_sl, pool_streams, pool, norm_frames, outs, fn)
    assert rc == 0, lib.ss_last_error_string()
    torch.cuda.synchronize()  # the temporaries of this helper die here
    return outs, ro


def _schedule(rng, n_streams, G, K):
    """hops[k][b]: the hops stream b delivers in call k (-1: absent from the call, 0: present without audio); every stream's
    positive entries sum to G."""
    hops = rng.multinomial(G, np.ones(K) / K, size=n_streams).T.astype(np.int64)  # [K, n_streams]
    absent = (hops == 0) & (rng.random(hops.shape) < 0.5)
    hops[absent] = -1
    return hops


@pytest.mark.gpu
@pytest.mark.parametrize("fn", ["mfcc", "mfe"])
def test_headline_pool_equals_the_dense_stream_bit_for_bit(ss, sslib, fn):
    import torch

    cfg = _cfg(ss)
    POOL, B, G, K, STEP = 2048, 1024, 16, 8, 160
    rng = np.random.default_rng(31)
    hops = _schedule(rng, B, G, K)
    # the schedule itself: entries without rows, absent streams, one, two and four or more hops, every stream fed G hops
    assert (hops == 0).any() and (hops == -1).any() and (hops == 1).any() and (hops == 2).any() and (hops >= 4).any()
    assert (np.where(hops > 0, hops, 0).sum(axis=0) == G).all()
    assert len({tuple(col) for col in hops.T}) > B // 2  # the streams' splits differ
    slot_of = rng.permutation(POOL)[:B]
    s = _gsig(torch, (B, G * STEP), 32)
    pool = _gsig(torch, (POOL, STEP), 33)
    pool[torch.from_numpy(slot_of).cuda()] = 0.0  # the streams open fresh; the other rows keep their random content
    never_named = np.setdiff1d(np.arange(POOL), slot_of)
    before = pool.clone()
    cols = [13] if fn == "mfcc" else [40, 1]
    got = [torch.full((B, G, c), float("nan"), device="cuda") for c in cols]
    at = np.zeros(B, np.int64)
    names, orders = [], []
    for k in range(K):
        present = np.flatnonzero(hops[k] >= 0)
        order = rng.permutation(present)
        orders.append(tuple(order[:8]))
        chunks = [s[b, at[b] * STEP:(at[b] + hops[k, b]) * STEP] for b in order]
        outs, ro = _pool_call(torch, sslib, cfg, chunks, slot_of[order], pool, POOL, G + 1, fn)
        names.append(sslib.ss_last_kernel_name())
        for i, b in enumerate(order):
            r = hops[k, b]
            for o, g in zip(outs, got):
                if r:
                    g[b, at[b]:at[b] + r] = o[ro[i]:ro[i + 1]].reshape(r, -1)
            at[b] += r
    assert len(set(orders)) == K  # the entries stand in a different order in every call
    assert set(names) == {POOL_KERNEL if fn == "mfcc" else POOL_MFE_KERNEL}, names
    state = torch.zeros((B, STEP), device="cuda")
    want = _dense(torch, sslib, cfg, s, state, G + 1, fn)
    torch.cuda.synchronize()
    assert (at == G).all()
    for g, w in zip(got, want):
        assert torch.isfinite(g).all()
        assert torch.equal(g.reshape(w.shape), w)
    assert torch.equal(pool[torch.from_numpy(slot_of).cuda()], state)
    idx = torch.from_numpy(never_named).cuda()
    assert torch.equal(pool[idx], before[idx])


# four streams, eight hops each, four calls (-1: absent); stream 1 and 3 meet one-hop chunks, every call has its own order
GEN_HOPS = np.array([[2, 1, 0, 3], [0, 4, 3, 1], [5, -1, 1, 2], [1, 3, 4, 2]])
GEN_ORDER = [[2, 0, 3, 1], [1, 3, 0, 2], [3, 2, 0], [0, 1, 2, 3]]
GEN_SLOTS = [5, 0, 3, 6]
GEN_POOL = 7


def _ragged_feed(torch, lib, cfg, s, pool, fn="mfcc"):
    """Feed s [4, 8 * step] through GEN_HOPS / GEN_ORDER on slots GEN_SLOTS; returns the rows per stream and the kernel names."""
    _, _, step, _ = _sizes(lib, cfg.params)
    B, G = s.shape[0], s.shape[1] // step
    cols = [cfg.params.num_cepstral] if fn == "mfcc" else [cfg.params.num_filters, 1]
    got = [torch.full((B, G, c), float("nan"), device="cuda") for c in cols]
    at = [0] * B
    names = []
    for k in range(len(GEN_ORDER)):
        order = GEN_ORDER[k]
        chunks = [s[b, at[b] * step:(at[b] + GEN_HOPS[k][b]) * step] for b in order]
        outs, ro = _pool_call(torch, lib, cfg, chunks, [GEN_SLOTS[b] for b in order], pool, GEN_POOL, G + 1, fn)
        names.append(lib.ss_last_kernel_name())
        for i, b in enumerate(order):
            r = int(GEN_HOPS[k][b])
            for o, g in zip(outs, got):
                if r:
                    g[b, at[b]:at[b] + r] = o[ro[i]:ro[i + 1]].reshape(r, -1)
            at[b] += r
    assert at == [G] * B
    return got, names


def _equivalence_signal(s, flen, step):
    """zeros(flen) ++ s ++ zeros(step): its one-shot frames 1 .. G are a stream's rows 0 .. G - 1"""
    B = s.shape[0]
    return np.concatenate([np.zeros((B, flen), np.float32), s, np.zeros((B, step), np.float32)], axis=1)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SWEEP))
def test_generic_pool_matches_the_oracle_and_the_dense_stream(ss, sslib, oracle, name):
    import torch

    kw = SWEEP[name]
    cfg = _cfg(ss, **kw)
    rc, flen, step, S = _sizes(sslib, cfg.params)
    assert rc == 0
    if name == "preemph_step":
        assert S == 320 and S > step  # a one-hop chunk is shorter than the state: the advance shifts the row
    if name == "flen_lt_step":
        assert S == 0  # a null pool
    B, G = 4, 8
    s = _gsig(torch, (B, G * step), 34)
    pool = torch.zeros((GEN_POOL, S), device="cuda") if S else None
    (got,), names = _ragged_feed(torch, sslib, cfg, s, pool)
    assert all(n.startswith(GENERIC_POOL_PREFIX) for n in names), names
    state = torch.zeros((B, S), device="cuda")
    (want,) = _dense(torch, sslib, cfg, s, state if S else None, G + 1)
    assert sslib.ss_last_kernel_name().startswith(b"ss_front_generic_fstream<")
    torch.cuda.synchronize()
    p = oracle.make_params(**kw)
    x = _equivalence_signal(s.cpu().numpy(), flen, step)
    g = got.cpu().numpy()
    for b in range(B):
        ref = oracle.mfcc(p, x[b])[1:]
        print(name, b, "rel", rel(g[b], ref))
        assert rel(g[b], ref) <= RTOL, (name, b, rel(g[b], ref))
    assert torch.equal(got, want)
    if S:
        assert torch.equal(pool[torch.tensor(GEN_SLOTS, device="cuda")], state)
        others = [r for r in range(GEN_POOL) if r not in GEN_SLOTS]
        assert not pool[others].any()


@pytest.mark.gpu
@pytest.mark.parametrize("fn", ["mfcc", "mfe"])
def test_forced_generic_pool_on_the_default_shape(ss, sslab, fn):
    import torch

    from speechsauce_amd import _lib

    with _lib.use_library(sslab):
        sslab.ss_debug_force_generic(1)
        try:
            cfg = _cfg(ss)
            s = _gsig(torch, (4, 8 * 160), 35)
            pool = torch.zeros((GEN_POOL, 160), device="cuda")
            got, names = _ragged_feed(torch, sslab, cfg, s, pool, fn)
            state = torch.zeros((4, 160), device="cuda")
            want = _dense(torch, sslab, cfg, s, state, 9, fn)
            torch.cuda.synchronize()
            assert all(n.startswith(GENERIC_POOL_PREFIX) for n in names), names
            for g, w in zip(got, want):
                assert torch.equal(g.reshape(w.shape), w)
            assert torch.equal(pool[torch.tensor(GEN_SLOTS, device="cuda")], state)
        finally:
            sslab.ss_debug_force_generic(0)


@pytest.mark.gpu
@pytest.mark.parametrize("kernel,fn", [("headline", "mfcc"), ("headline", "mfe"), ("generic", "mfcc")])
def test_bad_device_tables_are_contained(ss, sslib, kernel, fn):
    """Input validation on the device: every access is bounds-checked by the entry decoder before it happens, so the bad entries
    are skipped, nothing outside the buffers is touched, and the config's error word is raised."""
    import torch

    kw = {} if kernel == "headline" else dict(preemph_coef=0.97, preemph_shift=1)
    cfg = _cfg(ss, **kw)
    _, _, step, S = _sizes(sslib, cfg.params)
    POOL, GUARD, FILL = 8, 4, -777.0
    # (hops of samples, extra samples, rows claimed in ro, slot, good)
    entries = [(2, 0, 2, 1, True),
               (1, 0, 1, POOL, False),   # slot = pool_streams
               (1, 0, 1, 3, True),
               (2, 0, 2, -1, False),     # slot = -1
               (1, 2, 1, 2, False),      # a chunk of step + 2 samples
               (3, 0, 3, 5, True),
               (1, 0, 2, 6, False),      # ro claims one row too many
               (1, 0, 1, 0, True),
               (2, 0, 2, 7, False)]      # rows end one past total_rows
    so = np.zeros(len(entries) + 1, np.int64)
    ro = np.zeros(len(entries) + 1, np.int64)
    for i, (h, extra, claimed, _, _) in enumerate(entries):
        so[i + 1] = so[i] + h * step + extra
        ro[i + 1] = ro[i] + claimed
    total_rows = int(ro[-1]) - 1
    x = _gsig(torch, (int(so[-1]),), 36)
    pool_g = torch.full((POOL + 2 * GUARD, S), FILL, device="cuda")
    pool = pool_g[GUARD:GUARD + POOL]
    pool.copy_(_gsig(torch, (POOL, S), 37))
    before = pool.clone()
    outs_g = _alloc_outs(torch, cfg, total_rows + 2 * GUARD, fn, FILL)
    outs = tuple(o[GUARD:GUARD + total_rows] for o in outs_g)
    # expected values of the good entries: the dense call on that stream alone
    want, want_state = {}, {}
    for i, (h, _, _, slot, good) in enumerate(entries):
        if good:
            st = before[slot:slot + 1].clone()
            want[i] = _dense(torch, sslib, cfg, x[so[i]:so[i + 1]][None, :].contiguous(), st, 20, fn)
            want_state[slot] = st
    d_so, d_ro = torch.from_numpy(so).cuda(), torch.from_numpy(ro).cuda()
    d_sl = torch.tensor([e[3] for e in entries], dtype=torch.int32, device="cuda")
    assert sslib.ss_config_device_status(cfg.handle) == 0
    rc = _raw_call(torch, sslib, cfg, x, len(entries), d_so, d_ro, total_rows, d_sl, POOL, pool, 20, outs, fn)
    assert rc == 0, sslib.ss_last_error_string()  # the tables are device data: the call itself cannot know
    name = sslib.ss_last_kernel_name()
    torch.cuda.synchronize()
    if kernel == "headline":
        assert name == (POOL_KERNEL if fn == "mfcc" else POOL_MFE_KERNEL)
    else:
        assert name.startswith(GENERIC_POOL_PREFIX)
    for i, (h, _, claimed, slot, good) in enumerate(entries):
        r0, r1 = int(ro[i]), min(int(ro[i + 1]), total_rows)
        for k, o in enumerate(outs):
            if good:
                assert torch.equal(o[r0:r1].reshape(want[i][k].shape[1:]), want[i][k][0]), (i, k)
            else:
                assert (o[r0:r1] == FILL).all(), (i, k)  # the pre-fill is still there
    for slot in range(POOL):
        assert torch.equal(pool[slot], want_state[slot][0] if slot in want_state else before[slot]), slot
    for o in outs_g:
        assert (o[:GUARD] == FILL).all() and (o[GUARD + total_rows:] == FILL).all()
    assert (pool_g[:GUARD] == FILL).all() and (pool_g[GUARD + POOL:] == FILL).all()
    assert sslib.ss_config_device_status(cfg.handle) == 6  # SS_ERR_DEVICE, read and cleared
    assert sslib.ss_config_device_status(cfg.handle) == 0
    good_chunks = [x[so[i]:so[i + 1]] for i, e in enumerate(entries) if e[4]]
    _pool_call(torch, sslib, cfg, good_chunks, [e[3] for e in entries if e[4]], pool, POOL, 20, fn)  # asserts rc == 0
    assert sslib.ss_config_device_status(cfg.handle) == 0


def _hip_runtime():
    """The HIP runtime this process has loaded (torch's), for the stream-capture calls the graph-shape check needs."""
    with open("/proc/self/maps") as f:
        paths = {line.split()[-1] for line in f if "libamdhip64" in line}
    assert paths, "no HIP runtime loaded"
    return C.CDLL(sorted(paths)[0])


@pytest.mark.gpu
def test_graph_replay_over_changing_tables_equals_eager_calls(ss, sslib):
    import torch

    cfg = _cfg(ss)
    N, CAP, POOL, STEP, K = 256, 1024, 512, 160, 5
    rng = np.random.default_rng(38)
    x = torch.zeros(CAP * STEP, device="cuda")
    d_so = torch.zeros(N + 1, dtype=torch.int64, device="cuda")
    d_ro = torch.zeros(N + 1, dtype=torch.int64, device="cuda")
    d_sl = torch.arange(N, dtype=torch.int32, device="cuda")
    out = torch.zeros((CAP, 13), device="cuda")
    pool_g = _gsig(torch, (POOL, STEP), 39)
    pool_e = pool_g.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up outside the capture (on a scratch pool; the zero tables are N entries without rows)
        rc = _raw_call(torch, sslib, cfg, x, N, d_so, d_ro, CAP, d_sl, POOL, pool_g.clone(), 100, (out,), stream=side.cuda_stream)
        assert rc == 0, sslib.ss_last_error_string()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    # the shape of the captured work: two kernel nodes, one edge
    hip = _hip_runtime()
    raw, graph = torch.cuda.Stream(), C.c_void_p()
    assert hip.hipStreamBeginCapture(C.c_void_p(raw.cuda_stream), 2) == 0  # hipStreamCaptureModeRelaxed
    rc = _raw_call(torch, sslib, cfg, x, N, d_so, d_ro, CAP, d_sl, POOL, pool_g, 100, (out,), stream=raw.cuda_stream)
    assert hip.hipStreamEndCapture(C.c_void_p(raw.cuda_stream), C.byref(graph)) == 0
    assert rc == 0, sslib.ss_last_error_string()
    n_nodes, n_edges = C.c_size_t(), C.c_size_t()
    assert hip.hipGraphGetNodes(graph, None, C.byref(n_nodes)) == 0
    assert hip.hipGraphGetEdges(graph, None, None, C.byref(n_edges)) == 0
    assert hip.hipGraphDestroy(graph) == 0
    assert (n_nodes.value, n_edges.value) == (2, 1)  # a linear chain: the rows, then the pool advance
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        rc = _raw_call(torch, sslib, cfg, x, N, d_so, d_ro, CAP, d_sl, POOL, pool_g, 100, (out,))
    assert rc == 0
    for k in range(K):
        n_live = int(rng.integers(100, N + 1))
        hops = np.zeros(N, np.int64)
        hops[rng.permutation(N)[:n_live]] = rng.integers(0, 5, n_live)  # unused capacity: entries without rows
        assert hops.sum() <= CAP and (hops == 0).any() and (hops >= 3).any()
        slots = rng.permutation(POOL)[:N].astype(np.int32)
        so = np.zeros(N + 1, np.int64)
        np.cumsum(hops * STEP, out=so[1:])
        ro = so // STEP
        xs = _gsig(torch, (int(so[-1]),), 40 + k)
        # eager, on the other pool
        chunks = [xs[so[i]:so[i + 1]] for i in range(N)]
        (want,), ro_e = _pool_call(torch, sslib, cfg, chunks, slots, pool_e, POOL, 100)
        assert np.array_equal(ro_e, ro)
        # replay over rewritten static buffers
        x[:xs.numel()] = xs
        d_so.copy_(torch.from_numpy(so))
        d_ro.copy_(torch.from_numpy(ro))
        d_sl.copy_(torch.from_numpy(slots))
        out.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out[:int(ro[-1])], want), k
        assert torch.isnan(out[int(ro[-1]):]).all()  # rows past the last entry are left alone
        assert torch.equal(pool_g, pool_e), k
    assert sslib.ss_config_device_status(cfg.handle) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("fn", ["mfcc", "mfe"])
def test_host_form_equals_the_device_form(ss, sslib, fn):
    import torch

    cfg = _cfg(ss)
    POOL, STEP = 16, 160
    hops = [3, 0, 1, 5, 2]
    slots = np.array([9, 2, 15, 0, 7], np.int32)
    so = np.zeros(len(hops) + 1, np.int64)
    np.cumsum(np.array(hops) * STEP, out=so[1:])
    x = _gsig(torch, (int(so[-1]),), 50)
    pool_d = _gsig(torch, (POOL, STEP), 51)
    pool_h = pool_d.cpu().numpy().copy()
    before = pool_h.copy()
    dev, ro = _pool_call(torch, sslib, cfg, [x[so[i]:so[i + 1]] for i in range(len(hops))], slots, pool_d, POOL, 30, fn)
    R = int(ro[-1])
    xh = x.cpu().numpy()
    FILL = np.float32(-3.0)
    houts = [np.full((R, 13), FILL)] if fn == "mfcc" else [np.full((R, 40), FILL), np.full((R,), FILL)]

    def host(so_, slots_, pool_streams=POOL):
        so_, slots_ = np.asarray(so_, np.int64), np.asarray(slots_, np.int32)
        if fn == "mfcc":
            return sslib.ss_mfcc_stream_packed(cfg.handle, xh.ctypes.data, len(slots_), so_.ctypes.data, slots_.ctypes.data, pool_streams,
                                               30, pool_h.ctypes.data, houts[0].ctypes.data)
        return sslib.ss_mfe_stream_packed(cfg.handle, xh.ctypes.data, len(slots_), so_.ctypes.data, slots_.ctypes.data, pool_streams,
                                          pool_h.ctypes.data, houts[0].ctypes.data, houts[1].ctypes.data)

    # host-side rejections: the pool and the outputs stay as they are, the first bad entry is named
    assert host(so, [9, 2, 15, 2, 7]) == 3 and b"entry 3" in sslib.ss_last_error_string()  # a slot named twice
    assert host(so, [9, 2, POOL, 0, 7]) == 3 and b"entry 2" in sslib.ss_last_error_string()  # a slot outside the pool
    assert host(so, [9, -1, 15, 0, 7]) == 3 and b"entry 1" in sslib.ss_last_error_string()
    bad = so.copy()
    bad[4] += 8
    assert host(bad, slots) == 3 and b"entry 3" in sslib.ss_last_error_string()  # a partial hop
    bad = so.copy()
    bad[0] = STEP
    assert host(bad, slots) == 3  # so[0] != 0
    assert host(so, slots, pool_streams=1 << 31) == 3
    assert np.array_equal(pool_h, before) and all((o == FILL).all() for o in houts)
    assert host(so[:1], slots[:0]) == 0  # no entries: nothing to do
    assert np.array_equal(pool_h, before) and all((o == FILL).all() for o in houts)
    assert host(so, slots) == 0, sslib.ss_last_error_string()
    for h, d in zip(houts, dev):
        assert np.array_equal(h, d.cpu().numpy())
    assert np.array_equal(pool_h, pool_d.cpu().numpy())
    changed = {int(r) for r in np.flatnonzero((pool_h != before).any(axis=1))}
    assert changed == {int(s) for s, h in zip(slots, hops) if h > 0}  # only named rows with audio moved


@pytest.mark.gpu
def test_python_classes_equal_the_ctypes_path(ss, sslib):
    import torch

    cfg = _cfg(ss)
    POOL, STEP = 8, 160
    a = _gsig(torch, (3, 6 * STEP), 52)
    calls = [([a[0, :2 * STEP], a[1, :0], a[2, :STEP]], [4, 1, 6]),
             ([a[2, STEP:5 * STEP], a[0, 2 * STEP:3 * STEP]], [6, 4]),
             ([a[1, :3 * STEP]], [1])]
    pool = torch.zeros((POOL, STEP), device="cuda")
    want_m, want_e = [], []
    pool_e = torch.zeros((POOL, STEP), device="cuda")
    for chunks, slots in calls:
        want_m.append(_pool_call(torch, sslib, cfg, chunks, slots, pool, POOL, 30))
        want_e.append(_pool_call(torch, sslib, cfg, chunks, slots, pool_e, POOL, 1, "mfe"))
    for to in (lambda t: t, lambda t: t.cpu().numpy()):
        np_ = lambda t: t.cpu().numpy() if torch.is_tensor(t) else t  # noqa: E731
        m = ss.MfccStreamPool(POOL, 16000, norm_frames=30)
        e = ss.MfeStreamPool(POOL, 16000)
        for k, (chunks, slots) in enumerate(calls):
            rows, ro = m([to(c) for c in chunks], slots)
            assert torch.is_tensor(rows) == torch.is_tensor(to(chunks[0]))
            assert np.array_equal(ro, want_m[k][1]) and np.array_equal(np_(rows), want_m[k][0][0].cpu().numpy())
            if k == 1:  # the packed-buffer form
                packed = to(torch.cat(chunks))
                feat, en, ro = e(packed, slots, lengths=[int(c.numel()) for c in chunks])
            else:
                feat, en, ro = e([to(c) for c in chunks], slots)
            assert np.array_equal(ro, want_e[k][1])
            assert np.array_equal(np_(feat), want_e[k][0][0].cpu().numpy()) and np.array_equal(np_(en), want_e[k][0][1].cpu().numpy())
        torch.cuda.synchronize()
        assert np.array_equal(np_(m.state), pool.cpu().numpy()) and np.array_equal(np_(e.state), pool_e.cpu().numpy())
        assert m.state.shape == (POOL, STEP)
        # reset(slots=[...]) makes exactly those streams fresh
        m.reset(slots=[4])
        st = np_(m.state)
        assert not st[4].any() and np.array_equal(st[6], pool[6].cpu().numpy()) and np.array_equal(st[1], pool[1].cpu().numpy())
        rows, _ = m([to(a[0, :2 * STEP]), to(a[2, 5 * STEP:])], [4, 6])
        fresh = _dense(torch, sslib, cfg, a[0:1, :2 * STEP].contiguous(), torch.zeros((1, STEP), device="cuda"), 30)[0][0]
        cont = _dense(torch, sslib, cfg, a[2:3, 5 * STEP:].contiguous(), pool[6:7].clone(), 30)[0][0]
        torch.cuda.synchronize()
        assert np.array_equal(np_(rows), torch.cat([fresh, cont]).cpu().numpy())
        m.reset()
        assert not np_(m.state).any()


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", ["headline", "generic"])
def test_an_entry_does_not_depend_on_its_place_in_the_call(ss, sslib, kernel):
    import torch

    kw = {} if kernel == "headline" else dict(preemph_coef=0.97, preemph_shift=1)
    cfg = _cfg(ss, **kw)
    _, _, step, S = _sizes(sslib, cfg.params)
    POOL = 12
    base = _gsig(torch, (POOL, S), 60)
    mine = _gsig(torch, (3 * step,), 61)
    other = [_gsig(torch, (h * step,), 62 + h) for h in (1, 4, 2, 5)]
    empty = mine[:0]
    layouts = {"first": ([mine] + other, [7, 0, 1, 2, 3]),
               "last": (other + [mine], [0, 1, 2, 3, 7]),
               "between_empties": (other[:2] + [empty, mine, empty] + other[2:], [0, 1, 9, 7, 10, 2, 3])}
    rows, states = {}, {}
    for key, (chunks, slots) in layouts.items():
        pool = base.clone()
        (out,), ro = _pool_call(torch, sslib, cfg, chunks, slots, pool, POOL, 25)
        i = slots.index(7)
        rows[key] = out[ro[i]:ro[i + 1]].clone()
        states[key] = pool[7].clone()
        if key == "between_empties":
            assert torch.equal(pool[9], base[9]) and torch.equal(pool[10], base[10])  # entries without rows leave their rows alone
    st = base[7:8].clone()
    (want,) = _dense(torch, sslib, cfg, mine[None, :].contiguous(), st, 25)
    torch.cuda.synchronize()
    for key in layouts:
        assert rows[key].shape == (3, 13)
        assert torch.equal(rows[key], want[0]), key
        assert torch.equal(states[key], st[0]), key
