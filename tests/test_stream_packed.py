"""Ragged streaming mel spectrogram / STFT over a pool of stream states: ss_stream_packed_row_offsets,
ss_mel_spectrogram_stream_packed / ss_stft_stream_packed (host pointers), their *_device forms, and the Python front's
MelSpectrogramStreamPool / StftStreamPool.

A pool is the [pool_streams x S] state block of the dense streaming calls (S = W - H).  One call serves n_active entries; entry i is
the chunk x[so[i] : so[i+1]] (R_i whole hops, R_i = 0 allowed) of the stream whose state is pool row slots[i]; its rows are rows
ro[i] .. ro[i+1] of the packed row space (mel: its [M x R_i] block at out + M ro[i]).  Per entry the rows and the pool row
afterwards are what the dense continuous streaming call gives for that stream alone.  Expected values come from the dense streaming
calls (tests/test_stream.py checks those against the one-shot calls and the oracle) and from the f64 oracle, never from the ragged
calls themselves.
"""
import ctypes as C

import numpy as np
import pytest

from common import CONFIGS, RTOL, rel

CONT = 1  # SS_STREAM_CONTINUOUS

POOL_KERNEL = b"ss_mel_c1024sp<w12,mel6321>"
DENSE_W12_KERNEL = b"ss_mel_c1024s<w12,mel6321>"
GENERIC_POOL_PREFIX = b"ss_front_generic_streamp<"
GENERIC_DENSE_PREFIX = b"ss_front_generic_stream<"

# the sweep of tests/test_stream.py
CFG3 = dict(CONFIGS["cfg3"])  # 2048 / 512, 128 filters: the dedicated kernel's shape
CFG3_KW = dict(frame_length=0.032, num_filters=128, fft_length=2048, high_frequency=8000.0)
ODD_HOP = dict(sample_rate=16000, fft_points=2048, frame_length=600 / 16000, num_filters=64)  # H = 600 does not divide W
CHIRPZ = dict(sample_rate=16000, fft_points=1000, frame_length=400 / 16000, num_filters=40)  # chirp-z W = 1000, H = 400
SWEEP = {"cfg3": CFG3, "odd_hop": ODD_HOP, "chirpz": CHIRPZ, "W512": dict(sample_rate=16000, fft_points=512, frame_length=0.016),
         "W1024": dict(sample_rate=16000, fft_points=1024, frame_length=333 / 16000),
         "W441": dict(sample_rate=22050, fft_points=441, frame_length=0.01)}


def _hop(p):
    return int(np.float32(p.frame_length) * np.float32(p.sample_rate))


def _row_offsets(sslib, p, so):
    so = np.asarray(so, dtype=np.int64)
    ro = np.full(so.size, -1, dtype=np.int64)
    rc = sslib.ss_stream_packed_row_offsets(C.byref(p), so.size - 1, so.ctypes.data, ro.ctypes.data)
    return rc, ro


# ---------------------------------------------------------------- CPU ---------------------------------------------------------

@pytest.mark.parametrize("name", ["cfg3", "odd_hop", "chirpz"])
def test_row_offsets_follow_the_formula(sslib, name):
    from speechsauce_amd import _lib

    p = _lib.make_params(**SWEEP[name])
    H = _hop(p)
    assert H == {"cfg3": 512, "odd_hop": 600, "chirpz": 400}[name]
    rng = np.random.default_rng(70)
    for n in (1, 7, 200):
        hops = rng.integers(0, 5, n)
        hops[rng.random(n) < 0.3] = 0
        if n > 1:
            hops[0], hops[-1] = 0, 0  # entries without rows at both ends too
        so = np.zeros(n + 1, np.int64)
        np.cumsum(hops * H, out=so[1:])
        rc, ro = _row_offsets(sslib, p, so)
        assert rc == 0, sslib.ss_last_error_string()
        assert ro[0] == 0 and np.array_equal(np.diff(ro), hops)
    rc, ro = _row_offsets(sslib, p, [0, 0, 0])  # nothing but entries without rows
    assert rc == 0 and ro.tolist() == [0, 0, 0]
    rc, ro = _row_offsets(sslib, p, [0])  # no entries
    assert rc == 0 and ro.tolist() == [0]


def test_row_offsets_rejections(sslib):
    from speechsauce_amd import _lib

    p = _lib.make_params(**CFG3)
    assert _row_offsets(sslib, p, [512, 1024])[0] == 3  # so[0] != 0
    assert _row_offsets(sslib, p, [0, 1024, 512])[0] == 3  # a decreasing pair
    assert b"entry 1" in sslib.ss_last_error_string()
    assert _row_offsets(sslib, p, [0, 512, 1030])[0] == 3  # not whole hops
    assert b"entry 1" in sslib.ss_last_error_string()
    assert _row_offsets(sslib, p, [0, 512 * (1 << 22)])[0] == 3  # longer than 2^31 - 1 samples
    so = np.zeros(2, np.int64)
    ro = np.zeros(2, np.int64)
    assert sslib.ss_stream_packed_row_offsets(None, 1, so.ctypes.data, ro.ctypes.data) == 3
    assert sslib.ss_stream_packed_row_offsets(C.byref(p), 1, None, ro.ctypes.data) == 3
    assert sslib.ss_stream_packed_row_offsets(C.byref(p), 1, so.ctypes.data, None) == 3
    no_stft = _lib.make_params(sample_rate=16000, fft_points=512, frame_length=300 / 16000)  # W < 2H
    assert _row_offsets(sslib, no_stft, [0, 300])[0] == 2


def test_compute_entries_reject_a_null_config(sslib):
    assert sslib.ss_mel_spectrogram_stream_packed_device(None, None, 1, None, None, 1, None, 1, None, None, None) == 3
    assert sslib.ss_stft_stream_packed_device(None, None, 1, None, None, 1, None, 1, None, None, None) == 3
    assert sslib.ss_mel_spectrogram_stream_packed(None, None, 1, None, None, 1, None, None) == 3
    assert sslib.ss_stft_stream_packed(None, None, 1, None, None, 1, None, None) == 3


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

    for obj in (ss.MelSpectrogramStreamPool(4, 16000, **CFG3_KW), ss.StftStreamPool(4, 16000, frame_length=0.032, fft_length=2048)):
        with pytest.raises(SpeechSauceError) as e:
            obj([np.zeros(1024, np.float32), np.zeros(0, np.float32)], [2, 0])
        assert e.value.status == 4


def test_python_argument_rules(sslib):
    import speechsauce_amd as ss

    m = ss.MelSpectrogramStreamPool(4, 16000, **CFG3_KW)
    assert m.hop == 512 and m.state_len == 1536 and m.state is None and m.pool_streams == 4 and m.mode == "continuous"
    z = lambda n, dt=np.float32: np.zeros(n, dt)  # noqa: E731
    with pytest.raises(TypeError):
        m([z(1024, np.float64)], [0])  # wrong dtype
    with pytest.raises(ValueError):
        m([z(1000)], [0])  # a partial hop
    with pytest.raises(ValueError):
        m([z(1024), z(512)], [1, 1])  # a slot named twice
    with pytest.raises(ValueError):
        m([z(1024)], [4])  # a slot outside the pool
    with pytest.raises(ValueError):
        m([z(1024)], [-1])
    with pytest.raises(ValueError):
        m([z(1024), z(512)], [1])  # len(chunks) != len(slots)
    with pytest.raises(ValueError):
        m(z(1536), [0, 1], lengths=[1024, 1024])  # lengths do not add up to the packed buffer
    with pytest.raises(ValueError):
        m([np.zeros((2, 512), np.float32)], [0])  # chunks are 1-D
    with pytest.raises(TypeError):
        m(z(1024), [0])  # a packed buffer needs lengths
    assert m.state is None  # nothing was created by the rejected calls
    m.reset()
    m.reset(slots=[1])  # no state yet: nothing to do
    with pytest.raises(TypeError):
        ss.MelSpectrogramStreamPool(4, 16000, mode="reference", **CFG3_KW)  # continuous only: there is no mode to choose
    with pytest.raises(ValueError):
        ss.StftStreamPool(0, 16000)
    with pytest.raises(ss.SpeechSauceError) as e:
        ss.StftStreamPool(2, 16000, frame_length=300 / 16000)  # fft_length 512 < 2 hops: no STFT path
    assert e.value.status == 2
    r = ss.StftStreamPool(3, 16000, fft_length=2048, frame_length=600 / 16000)
    assert r.hop == 600 and r.state_len == 1448 and r.pool_streams == 3
    assert "MelSpectrogramStreamPool" in ss.__all__ and "StftStreamPool" in ss.__all__
    # the frame-path pools share the plumbing and keep their rules
    f = ss.MfccStreamPool(4, 16000, norm_frames=10)
    assert f.pool_streams == 4 and f.hop == 160 and isinstance(f, ss._StreamPoolMixin) and isinstance(m, ss._StreamPoolMixin)


# ---------------------------------------------------------------- GPU ---------------------------------------------------------

def _cfg(ss, **kw):
    from speechsauce_amd import _lib

    return ss.SpeechConfig(_lib.make_params(**kw))


def _gsig(torch, shape, seed):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    return torch.randn(shape, generator=g, device="cuda", dtype=torch.float32).mul_(0.1)


def _dims(cfg):
    p = cfg.params
    H = _hop(p)
    return H, p.fft_points - H, p.num_filters, p.fft_points // 2 + 1


def _dense(torch, lib, cfg, x, state, fn="mel"):
    """One dense continuous call on ONE stream: x a 1-D chunk, state its [1, S] row (updated in place).  Returns mel [M, R] /
    stft [R, F, 2] -- the expected values."""
    n = int(x.numel())
    H, _, M, F = _dims(cfg)
    R = n // H
    x = x.contiguous()
    if fn == "mel":
        out = torch.full((M, R), float("nan"), device="cuda")
        f = lib.ss_mel_spectrogram_stream_device
    else:
        out = torch.full((R, F, 2), float("nan"), device="cuda")
        f = lib.ss_stft_stream_device
    rc = f(cfg.handle, CONT, x.data_ptr(), 1, n, n, state.data_ptr(), out.data_ptr(), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, lib.ss_last_error_string()
    torch.cuda.synchronize()  # x may be a temporary
    return out


def _alloc_out(torch, cfg, rows, fn, fill=float("nan")):
    _, _, M, F = _dims(cfg)
    return torch.full((M * rows,), fill, device="cuda") if fn == "mel" else torch.full((rows, F, 2), fill, device="cuda")


def _block(cfg, out, ro, i, fn, r1=None):
    """Entry i's part of a packed output: mel [M, R_i] (rows are columns), stft [R_i, F, 2]."""
    _, _, M, _ = _dims(cfg)
    r0, r1 = int(ro[i]), int(ro[i + 1]) if r1 is None else r1
    return out[M * r0:M * r1].reshape(M, r1 - r0) if fn == "mel" else out[r0:r1]


def _raw_call(torch, lib, cfg, x, n_active, so, ro, total_rows, slots, pool_streams, pool, out, fn="mel", stream=None):
    """The device entry on device tables as they are; returns its status."""
    st = C.c_void_p(stream if stream is not None else torch.cuda.current_stream().cuda_stream)
    f = lib.ss_mel_spectrogram_stream_packed_device if fn == "mel" else lib.ss_stft_stream_packed_device
    return f(cfg.handle, x.data_ptr(), n_active, so.data_ptr(), ro.data_ptr(), total_rows, slots.data_ptr(), pool_streams, pool.data_ptr(),
             out.data_ptr(), st)


def _pool_call(torch, lib, cfg, chunks, slots, pool, pool_streams, fn="mel"):
    """One ragged call on a list of 1-D device chunks; returns (out, ro) with ro the host row offsets."""
    lens = [int(c.numel()) for c in chunks]
    so = np.zeros(len(lens) + 1, np.int64)
    np.cumsum(lens, out=so[1:])
    rc, ro = _row_offsets(lib, cfg.params, so)
    assert rc == 0, lib.ss_last_error_string()
    x = torch.cat(list(chunks)) if so[-1] else torch.zeros(1, device="cuda")
    out = _alloc_out(torch, cfg, int(ro[-1]), fn)
    if out.numel() == 0:
        out = torch.full((1,), float("nan"), device="cuda")
    d_so, d_ro = torch.from_numpy(so).cuda(), torch.from_numpy(ro).cuda()
    d_sl = torch.tensor([int(v) for v in slots], dtype=torch.int32, device="cuda")
    rc = _raw_call(torch, lib, cfg, x, len(lens), d_so, d_ro, int(ro[-1]), d_sl, pool_streams, pool, out, fn)
    assert rc == 0, lib.ss_last_error_string()
    torch.cuda.synchronize()  # the temporaries of this helper die here
    return out, ro


def _schedule(rng, n_streams, K):
    """hops[k][b]: the hops stream b delivers in tick k (-1: absent from the call, 0: present without audio, else 1 .. 4)"""
    hops = rng.integers(1, 5, (K, n_streams))
    u = rng.random(hops.shape)
    hops[u < 0.2] = 0
    hops[u < 0.1] = -1
    return hops


def _ragged_ticks(torch, lib, cfg, s, hops, slot_of, pool, pool_streams, rng, fn="mel"):
    """Feed the streams s [B, *] through the schedule `hops`, every tick in a shuffled order.  Returns per stream the list of its
    blocks, the kernel names and the chunk boundaries (in hops) per stream."""
    H = _dims(cfg)[0]
    B = s.shape[0]
    at = np.zeros(B, np.int64)
    got = [[] for _ in range(B)]
    names, orders = [], []
    for k in range(hops.shape[0]):
        present = np.flatnonzero(hops[k] >= 0)
        order = rng.permutation(present)
        orders.append(tuple(order[:6]))
        chunks = [s[b, at[b] * H:(at[b] + hops[k, b]) * H] for b in order]
        out, ro = _pool_call(torch, lib, cfg, chunks, slot_of[order], pool, pool_streams, fn)
        names.append(lib.ss_last_kernel_name())
        for i, b in enumerate(order):
            if hops[k, b]:
                got[b].append(_block(cfg, out, ro, i, fn).clone())
            at[b] += hops[k, b]
    return got, names, orders


def _dense_ticks(torch, lib, cfg, s, hops, fn="mel"):
    """The expected values: every stream on its own, the same chunks through the dense continuous call (n_streams = 1)."""
    H, S, _, _ = _dims(cfg)
    B = s.shape[0]
    want, states, names = [[] for _ in range(B)], [], set()
    for b in range(B):
        state = torch.zeros((1, S), device="cuda")
        at = 0
        for k in range(hops.shape[0]):
            if hops[k, b] > 0:
                want[b].append(_dense(torch, lib, cfg, s[b, at * H:(at + hops[k, b]) * H], state, fn))
                names.add(lib.ss_last_kernel_name())
                at += hops[k, b]
        states.append(state[0])
    return want, torch.stack(states), names


@pytest.mark.gpu
def test_headline_pool_equals_the_dense_stream_bit_for_bit(ss, sslib, sslab):
    """cfg3, mel: a 64-row pool over several ticks of a random schedule against per-stream dense continuous calls -- identical to
    the twelve-wave dense build (forced through the lab library), within RTOL of the build a lone small dense call picks."""
    import torch

    from speechsauce_amd import _lib

    cfg = _cfg(ss, **CFG3)
    POOL, B, K, H = 64, 48, 6, 512
    rng = np.random.default_rng(71)
    hops = _schedule(rng, B, K)
    assert (hops == 0).any() and (hops == -1).any() and all((hops == h).any() for h in (1, 2, 3, 4))
    G = int(np.where(hops > 0, hops, 0).sum(axis=0).max())
    slot_of = rng.permutation(POOL)[:B]
    s = _gsig(torch, (B, G * H), 72)
    pool = _gsig(torch, (POOL, 1536), 73)
    pool[torch.from_numpy(slot_of).cuda()] = 0.0  # the streams open fresh; the other rows keep their random content
    never_named = torch.from_numpy(np.setdiff1d(np.arange(POOL), slot_of)).cuda()
    before = pool.clone()
    got, names, orders = _ragged_ticks(torch, sslib, cfg, s, hops, slot_of, pool, POOL, rng)
    assert set(names) == {POOL_KERNEL}, names
    assert len(set(orders)) == K  # the entries stand in a different order in every tick
    with _lib.use_library(sslab):
        try:
            sslab.ss_debug_mel_tile(3)  # twelve waves wherever that build exists
            want, state, dense_names = _dense_ticks(torch, sslab, _cfg(ss, **CFG3), s, hops)
        finally:
            sslab.ss_debug_mel_tile(1)
    assert dense_names == {DENSE_W12_KERNEL}, dense_names
    loose, _, loose_names = _dense_ticks(torch, sslib, cfg, s, hops)  # the automatic choice for one stream: eight waves
    assert all(n.startswith(b"ss_mel_c1024s") for n in loose_names), loose_names
    worst = 0.0
    for b in range(B):
        assert len(got[b]) == len(want[b]) == int((hops[:, b] > 0).sum())
        for g, w, lo in zip(got[b], want[b], loose[b]):
            assert torch.isfinite(g).all()
            assert torch.equal(g, w), b
            worst = max(worst, rel(g.cpu().numpy(), lo.cpu().numpy()))
    print("headline pool against the unforced dense call: worst rel", worst)
    assert worst <= RTOL
    assert torch.equal(pool[torch.from_numpy(slot_of).cuda()], state)
    assert torch.equal(pool[never_named], before[never_named])
    assert sslib.ss_config_device_status(cfg.handle) == 0


@pytest.mark.gpu
def test_headline_pool_at_an_odd_hop(ss, sslib, sslab):
    """H = 600 does not divide W = 2048 (S = 1448, chunks start at either parity): the dedicated kernel's ragged build with run-time
    tap counts, against the twelve-wave dense build."""
    import torch

    from speechsauce_amd import _lib

    cfg = _cfg(ss, **ODD_HOP)
    POOL, B, K, H = 9, 7, 4, 600
    rng = np.random.default_rng(74)
    hops = _schedule(rng, B, K)
    G = int(np.where(hops > 0, hops, 0).sum(axis=0).max())
    slot_of = rng.permutation(POOL)[:B]
    s = _gsig(torch, (B, G * H), 75)
    pool = torch.zeros((POOL, 2048 - H), device="cuda")
    got, names, _ = _ragged_ticks(torch, sslib, cfg, s, hops, slot_of, pool, POOL, rng)
    assert all(n.startswith(b"ss_mel_c1024sp<w12") for n in names), names
    with _lib.use_library(sslab):
        try:
            sslab.ss_debug_mel_tile(3)
            want, state, dense_names = _dense_ticks(torch, sslab, _cfg(ss, **ODD_HOP), s, hops)
        finally:
            sslab.ss_debug_mel_tile(1)
    assert all(n.startswith(b"ss_mel_c1024s<w12") for n in dense_names), dense_names
    for b in range(B):
        for g, w in zip(got[b], want[b]):
            assert torch.equal(g, w), b
    assert torch.equal(pool[torch.from_numpy(slot_of).cuda()], state)


# four streams, eight hops each, four calls (-1: absent); streams 1 and 3 meet one-hop chunks, every call has its own order
GEN_HOPS = np.array([[2, 1, 0, 3], [0, 4, 3, 1], [5, -1, 1, 2], [1, 3, 4, 2]])
GEN_ORDER = [[2, 0, 3, 1], [1, 3, 0, 2], [3, 2, 0], [0, 1, 2, 3]]
GEN_SLOTS = [5, 0, 3, 6]
GEN_POOL = 7


def _ragged_feed(torch, lib, cfg, s, pool, fn):
    """Feed s [4, 8 H] through GEN_HOPS / GEN_ORDER on slots GEN_SLOTS; returns the blocks per stream and the kernel names."""
    H = _dims(cfg)[0]
    B = s.shape[0]
    got = [[] for _ in range(B)]
    at = [0] * B
    names = []
    for k in range(len(GEN_ORDER)):
        order = GEN_ORDER[k]
        chunks = [s[b, at[b] * H:(at[b] + GEN_HOPS[k][b]) * H] for b in order]
        out, ro = _pool_call(torch, lib, cfg, chunks, [GEN_SLOTS[b] for b in order], pool, GEN_POOL, fn)
        names.append(lib.ss_last_kernel_name())
        for i, b in enumerate(order):
            if GEN_HOPS[k][b]:
                got[b].append(_block(cfg, out, ro, i, fn).clone())
            at[b] += int(GEN_HOPS[k][b])
    assert at == [8] * B
    return got, names


def expect_continuous(oracle, p, s, fn="mel"):
    """Rows of a continuous stream fed s (any cut): the real rows of the one-shot call on zeros(n_pad H) ++ s
    (tests/test_stream.py's construction)."""
    H, n_pad, _ = oracle.stft_sizes(p)
    T = s.shape[-1] // H
    x = np.concatenate([np.zeros(s.shape[:-1] + (n_pad * H,), np.float32), s], axis=-1)
    if fn == "mel":
        return oracle.mel_spectrogram(p, np.atleast_2d(x))[..., :T]
    return oracle.stft(p, np.atleast_2d(x))[:, :T]


@pytest.mark.gpu
@pytest.mark.parametrize("fn", ["mel", "stft"])
@pytest.mark.parametrize("name", list(SWEEP))
def test_generic_pool_matches_the_oracle_and_the_dense_stream(ss, sslab, oracle, name, fn):
    """Every shape of the sweep on the generic kernel (forced through the lab library: the 2048-point mel shapes would take the
    dedicated kernel), mel and stft: identical to the dense generic stream per stream, within RTOL of the f64 oracle."""
    import torch

    from speechsauce_amd import _lib

    kw = SWEEP[name]
    with _lib.use_library(sslab):
        sslab.ss_debug_force_generic(1)
        try:
            cfg = _cfg(ss, **kw)
            H, S, M, F = _dims(cfg)
            s = _gsig(torch, (4, 8 * H), 76)
            pool = torch.zeros((GEN_POOL, S), device="cuda")
            got, names = _ragged_feed(torch, sslab, cfg, s, pool, fn)
            assert all(n.startswith(GENERIC_POOL_PREFIX) for n in names), names
            assert all((b",chirpz>" in n) == (name in ("chirpz", "W441")) for n in names), names
            hops = np.array(GEN_HOPS)
            want, state, dense_names = _dense_ticks(torch, sslab, cfg, s, hops, fn)
            assert all(n.startswith(GENERIC_DENSE_PREFIX) for n in dense_names), dense_names
        finally:
            sslab.ss_debug_force_generic(0)
    for b in range(4):
        assert len(got[b]) == len(want[b])
        for g, w in zip(got[b], want[b]):
            assert torch.equal(g, w), (name, fn, b)
    assert torch.equal(pool[torch.tensor(GEN_SLOTS, device="cuda")], state)
    others = [r for r in range(GEN_POOL) if r not in GEN_SLOTS]
    assert not pool[others].any()
    p = oracle.make_params(**kw)
    ref = expect_continuous(oracle, p, s.cpu().numpy(), fn)
    for b in range(4):
        g = torch.cat(got[b], dim=1 if fn == "mel" else 0).cpu().numpy()
        if fn == "stft":
            g = g[..., 0] + 1j * g[..., 1]
        err = float(np.abs(g - ref[b]).max() / np.abs(ref[b]).max())
        print(name, fn, b, "rel", err)
        assert g.shape == ref[b].shape and err <= RTOL, (name, fn, b, err)


@pytest.mark.gpu
@pytest.mark.parametrize("kernel,fn", [("headline", "mel"), ("generic", "mel"), ("generic", "stft")])
def test_an_entry_does_not_depend_on_its_place_in_the_call(ss, sslib, kernel, fn):
    import torch

    cfg = _cfg(ss, **(CFG3 if kernel == "headline" else CHIRPZ))
    H, S, _, _ = _dims(cfg)
    POOL = 12
    base = _gsig(torch, (POOL, S), 77)
    mine = _gsig(torch, (3 * H,), 78)
    other = [_gsig(torch, (h * H,), 79 + h) for h in (1, 4, 2, 5)]
    empty = mine[:0]
    layouts = {"first": ([mine] + other, [7, 0, 1, 2, 3]),
               "last": (other + [mine], [0, 1, 2, 3, 7]),
               "alone": ([mine], [7]),
               "between_empties": (other[:2] + [empty, empty, mine, empty] + other[2:], [0, 1, 9, 11, 7, 10, 2, 3])}
    rows, states = {}, {}
    for key, (chunks, slots) in layouts.items():
        pool = base.clone()
        out, ro = _pool_call(torch, sslib, cfg, chunks, slots, pool, POOL, fn)
        name = sslib.ss_last_kernel_name()
        assert name == POOL_KERNEL if kernel == "headline" else name.startswith(GENERIC_POOL_PREFIX), name
        rows[key] = _block(cfg, out, ro, slots.index(7), fn).clone()
        states[key] = pool[7].clone()
        if key == "between_empties":  # entries without rows leave their pool rows alone
            assert all(torch.equal(pool[r], base[r]) for r in (9, 10, 11))
    for key in layouts:
        assert torch.isfinite(rows[key]).all()
        assert torch.equal(rows[key], rows["first"]), key
        assert torch.equal(states[key], states["first"]), key
    if kernel == "generic":  # (the headline build's dense twin needs the lab library: the bit-for-bit test above)
        st = base[7:8].clone()
        want = _dense(torch, sslib, cfg, mine, st, fn)
        assert torch.equal(rows["first"], want) and torch.equal(states["first"], st[0])
    assert torch.equal(states["first"], torch.cat([base[7], mine])[-S:])  # last S samples of old row ++ chunk


@pytest.mark.gpu
@pytest.mark.parametrize("kernel,fn", [("headline", "mel"), ("generic", "mel"), ("generic", "stft")])
def test_bad_device_tables_are_contained(ss, sslib, sslab, kernel, fn):
    """Input validation on the device: every access is bounds-checked by the entry decoder before it happens, so the bad entries
    are skipped, nothing outside the buffers is touched, and the config's error word is raised.  The tables are merely
    inconsistent: no access outside the buffers is attempted."""
    import torch

    from speechsauce_amd import _lib

    kw = CFG3 if kernel == "headline" else CHIRPZ
    cfg = _cfg(ss, **kw)
    H, S, M, F = _dims(cfg)
    POOL, GUARD, FILL = 8, 4, -777.0
    # (hops of samples, extra samples, rows claimed in ro, slot, good)
    entries = [(2, 0, 2, 1, True),
               (1, 0, 1, POOL, False),   # slot = pool_streams
               (1, 0, 1, 3, True),
               (2, 0, 2, -1, False),     # slot = -1
               (1, 2, 1, 2, False),      # a chunk of H + 2 samples
               (3, 0, 3, 5, True),
               (0, 0, 0, 4, True),       # an entry without rows
               (1, 0, 2, 6, False),      # ro claims one row too many
               (1, 0, 1, 0, True),
               (2, 0, 2, 7, False)]      # rows end one past total_rows
    so = np.zeros(len(entries) + 1, np.int64)
    ro = np.zeros(len(entries) + 1, np.int64)
    for i, (h, extra, claimed, _, _) in enumerate(entries):
        so[i + 1] = so[i] + h * H + extra
        ro[i + 1] = ro[i] + claimed
    total_rows = int(ro[-1]) - 1
    x = _gsig(torch, (int(so[-1]),), 80)
    pool_g = torch.full((POOL + 2 * GUARD, S), FILL, device="cuda")
    pool = pool_g[GUARD:GUARD + POOL]
    pool.copy_(_gsig(torch, (POOL, S), 81))
    before = pool.clone()
    out_g = _alloc_out(torch, cfg, total_rows + 2 * GUARD, fn, FILL)
    out = out_g[M * GUARD:M * (GUARD + total_rows)] if fn == "mel" else out_g[GUARD:GUARD + total_rows]
    # expected values of the good entries: the dense call on that stream alone (headline: the twelve-wave dense build)
    want, want_state = {}, {}

    def expected(lib, cfg_d):
        for i, (h, _, _, slot, good) in enumerate(entries):
            if good:
                st = before[slot:slot + 1].clone()
                if h:
                    want[i] = _dense(torch, lib, cfg_d, x[so[i]:so[i + 1]], st, fn)
                want_state[slot] = st

    if kernel == "headline":
        with _lib.use_library(sslab):
            try:
                sslab.ss_debug_mel_tile(3)
                expected(sslab, _cfg(ss, **kw))
                assert sslab.ss_last_kernel_name() == DENSE_W12_KERNEL
            finally:
                sslab.ss_debug_mel_tile(1)
    else:
        expected(sslib, cfg)
    d_so, d_ro = torch.from_numpy(so).cuda(), torch.from_numpy(ro).cuda()
    d_sl = torch.tensor([e[3] for e in entries], dtype=torch.int32, device="cuda")
    assert sslib.ss_config_device_status(cfg.handle) == 0
    rc = _raw_call(torch, sslib, cfg, x, len(entries), d_so, d_ro, total_rows, d_sl, POOL, pool, out, fn)
    assert rc == 0, sslib.ss_last_error_string()  # the tables are device data: the call itself cannot know
    name = sslib.ss_last_kernel_name()
    torch.cuda.synchronize()
    assert name == POOL_KERNEL if kernel == "headline" else name.startswith(GENERIC_POOL_PREFIX), name
    for i, (h, _, claimed, slot, good) in enumerate(entries):
        r1 = min(int(ro[i + 1]), total_rows)
        blk = _block(cfg, out, ro, i, fn, r1)
        if good and h:
            assert torch.equal(blk, want[i]), i
        elif not good:
            assert (blk == FILL).all(), i  # the pre-fill is still there
    for slot in range(POOL):
        assert torch.equal(pool[slot], want_state[slot][0] if slot in want_state else before[slot]), slot
    assert torch.equal(pool[4], before[4])  # the entry without rows
    lo, hi = (M * GUARD, M * (GUARD + total_rows)) if fn == "mel" else (GUARD, GUARD + total_rows)
    assert (out_g[:lo] == FILL).all() and (out_g[hi:] == FILL).all()
    assert (pool_g[:GUARD] == FILL).all() and (pool_g[GUARD + POOL:] == FILL).all()
    assert sslib.ss_config_device_status(cfg.handle) == 6  # SS_ERR_DEVICE, read and cleared
    assert sslib.ss_config_device_status(cfg.handle) == 0
    good_chunks = [x[so[i]:so[i + 1]] for i, e in enumerate(entries) if e[4]]
    _pool_call(torch, sslib, cfg, good_chunks, [e[3] for e in entries if e[4]], pool, POOL, fn)  # asserts rc == 0
    assert sslib.ss_config_device_status(cfg.handle) == 0


def _hip_runtime():
    """The HIP runtime this process has loaded (torch's), for the stream-capture calls the graph-shape check needs."""
    with open("/proc/self/maps") as f:
        paths = {line.split()[-1] for line in f if "libamdhip64" in line}
    assert paths, "no HIP runtime loaded"
    return C.CDLL(sorted(paths)[0])


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", ["headline", "generic"])
def test_graph_replay_over_changing_tables_equals_eager_calls(ss, sslib, kernel):
    import torch

    cfg = _cfg(ss, **(CFG3 if kernel == "headline" else CHIRPZ))
    H, S, M, _ = _dims(cfg)
    N, CAP, POOL, K = 96, 384, 160, 4
    rng = np.random.default_rng(82)
    x = torch.zeros(CAP * H, device="cuda")
    d_so = torch.zeros(N + 1, dtype=torch.int64, device="cuda")
    d_ro = torch.zeros(N + 1, dtype=torch.int64, device="cuda")
    d_sl = torch.arange(N, dtype=torch.int32, device="cuda")
    out = torch.zeros(M * CAP, device="cuda")
    pool_g = _gsig(torch, (POOL, S), 83)
    pool_e = pool_g.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up outside the capture (on a scratch pool; the zero tables are N entries without rows)
        rc = _raw_call(torch, sslib, cfg, x, N, d_so, d_ro, CAP, d_sl, POOL, pool_g.clone(), out, stream=side.cuda_stream)
        assert rc == 0, sslib.ss_last_error_string()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    # the shape of the captured work: two kernel nodes, one edge
    hip = _hip_runtime()
    raw, graph = torch.cuda.Stream(), C.c_void_p()
    assert hip.hipStreamBeginCapture(C.c_void_p(raw.cuda_stream), 2) == 0  # hipStreamCaptureModeRelaxed
    rc = _raw_call(torch, sslib, cfg, x, N, d_so, d_ro, CAP, d_sl, POOL, pool_g, out, stream=raw.cuda_stream)
    assert hip.hipStreamEndCapture(C.c_void_p(raw.cuda_stream), C.byref(graph)) == 0
    assert rc == 0, sslib.ss_last_error_string()
    n_nodes, n_edges = C.c_size_t(), C.c_size_t()
    assert hip.hipGraphGetNodes(graph, None, C.byref(n_nodes)) == 0
    assert hip.hipGraphGetEdges(graph, None, None, C.byref(n_edges)) == 0
    assert hip.hipGraphDestroy(graph) == 0
    assert (n_nodes.value, n_edges.value) == (2, 1)  # a linear chain: the rows, then the pool advance
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        rc = _raw_call(torch, sslib, cfg, x, N, d_so, d_ro, CAP, d_sl, POOL, pool_g, out)
    assert rc == 0
    for k in range(K):
        n_live = int(rng.integers(40, N + 1))
        hops = np.zeros(N, np.int64)
        hops[rng.permutation(N)[:n_live]] = rng.integers(0, 5, n_live)  # unused capacity: entries without rows
        assert hops.sum() <= CAP and (hops == 0).any() and (hops >= 3).any()
        slots = rng.permutation(POOL)[:N].astype(np.int32)
        so = np.zeros(N + 1, np.int64)
        np.cumsum(hops * H, out=so[1:])
        ro = so // H
        xs = _gsig(torch, (int(so[-1]),), 84 + k)
        # eager, on the other pool
        want, ro_e = _pool_call(torch, sslib, cfg, [xs[so[i]:so[i + 1]] for i in range(N)], slots, pool_e, POOL)
        assert np.array_equal(ro_e, ro)
        # replay over rewritten static buffers
        x[:xs.numel()] = xs
        d_so.copy_(torch.from_numpy(so))
        d_ro.copy_(torch.from_numpy(ro))
        d_sl.copy_(torch.from_numpy(slots))
        out.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out[:M * int(ro[-1])], want), k
        assert torch.isnan(out[M * int(ro[-1]):]).all()  # rows past the last entry are left alone
        assert torch.equal(pool_g, pool_e), k
    assert sslib.ss_config_device_status(cfg.handle) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("name,fn", [("cfg3", "mel"), ("chirpz", "stft"), ("odd_hop", "stft")])
def test_host_form_equals_the_device_form(ss, sslib, name, fn):
    import torch

    cfg = _cfg(ss, **SWEEP[name])
    H, S, M, F = _dims(cfg)
    POOL = 16
    hops = [3, 0, 1, 5, 2]
    slots = np.array([9, 2, 15, 0, 7], np.int32)
    so = np.zeros(len(hops) + 1, np.int64)
    np.cumsum(np.array(hops) * H, out=so[1:])
    x = _gsig(torch, (int(so[-1]),), 90)
    pool_d = _gsig(torch, (POOL, S), 91)
    pool_h = pool_d.cpu().numpy().copy()
    before = pool_h.copy()
    dev, ro = _pool_call(torch, sslib, cfg, [x[so[i]:so[i + 1]] for i in range(len(hops))], slots, pool_d, POOL, fn)
    R = int(ro[-1])
    xh = x.cpu().numpy()
    FILL = np.float32(-3.0)
    hout = np.full((M * R,) if fn == "mel" else (R, F, 2), FILL)
    host_fn = sslib.ss_mel_spectrogram_stream_packed if fn == "mel" else sslib.ss_stft_stream_packed

    def host(so_, slots_, pool_streams=POOL, pool_=None, x_=None):
        so_, slots_ = np.asarray(so_, np.int64), np.asarray(slots_, np.int32)
        return host_fn(cfg.handle, (xh if x_ is None else x_).ctypes.data, len(slots_), so_.ctypes.data, slots_.ctypes.data, pool_streams,
                       (pool_h if pool_ is None else pool_).ctypes.data, hout.ctypes.data)

    # host-side rejections: the pool and the output stay as they are, the first bad entry is named
    assert host(so, [9, 2, 15, 2, 7]) == 3 and b"entry 3" in sslib.ss_last_error_string()  # a slot named twice
    assert host(so, [9, 2, POOL, 0, 7]) == 3 and b"entry 2" in sslib.ss_last_error_string()  # a slot outside the pool
    assert host(so, [9, -1, 15, 0, 7]) == 3 and b"entry 1" in sslib.ss_last_error_string()
    bad = so.copy()
    bad[4] += 8
    assert host(bad, slots) == 3 and b"entry 3" in sslib.ss_last_error_string()  # a partial hop
    bad = so.copy()
    bad[0] = H
    assert host(bad, slots) == 3  # so[0] != 0
    assert host(so, slots, pool_streams=1 << 31) == 3
    assert host(so, slots, pool_streams=0) == 3
    assert host(so, slots, x_=pool_h.reshape(-1)[S // 2:]) == 3  # the pool overlaps x
    assert np.array_equal(pool_h, before) and (hout == FILL).all()
    assert host(so[:1], slots[:0]) == 0  # no entries: nothing to do
    assert np.array_equal(pool_h, before) and (hout == FILL).all()
    assert host(so, slots) == 0, sslib.ss_last_error_string()
    assert np.array_equal(hout, dev.cpu().numpy())
    assert np.array_equal(pool_h, pool_d.cpu().numpy())
    changed = {int(r) for r in np.flatnonzero((pool_h != before).any(axis=1))}
    assert changed == {int(s) for s, h in zip(slots, hops) if h > 0}  # only named rows with audio moved
    # device-form argument rules: SS_ERR_ARG with everything untouched
    d_so, d_ro, d_sl = torch.from_numpy(so).cuda(), torch.from_numpy(ro).cuda(), torch.from_numpy(slots).cuda()
    snap = pool_d.clone()
    o = _alloc_out(torch, cfg, R, fn)
    n = len(hops)
    assert _raw_call(torch, sslib, cfg, x, n, d_so, d_ro, R, d_sl, 0, pool_d, o, fn) == 3  # an empty pool
    assert _raw_call(torch, sslib, cfg, x, n, d_so, d_ro, 1 << 31, d_sl, POOL, pool_d, o, fn) == 3
    assert _raw_call(torch, sslib, cfg, x, n, d_so, d_ro, R, d_sl, 1 << 31, pool_d, o, fn) == 3
    assert _raw_call(torch, sslib, cfg, x, n, d_so, d_ro, R, d_sl, POOL, pool_d, pool_d, fn) == 3  # the pool overlaps the output
    assert _raw_call(torch, sslib, cfg, pool_d[3], n, d_so, d_ro, R, d_sl, POOL, pool_d, o, fn) == 3  # the pool overlaps x
    assert _raw_call(torch, sslib, cfg, x, 0, d_so, d_ro, R, d_sl, POOL, pool_d, o, fn) == 0  # no entries: nothing launched
    torch.cuda.synchronize()
    assert torch.equal(pool_d, snap) and torch.isnan(o).all()


@pytest.mark.gpu
def test_python_classes_equal_the_ctypes_path(ss, sslib):
    import torch

    cfg_m, cfg_s = _cfg(ss, **CFG3), _cfg(ss, **CHIRPZ)
    POOL = 8
    for cls_kw, cfg, fn in ((dict(sampling_frequency=16000, **CFG3_KW), cfg_m, "mel"),
                            (dict(sampling_frequency=16000, frame_length=400 / 16000, fft_length=1000), cfg_s, "stft")):
        H, S, M, F = _dims(cfg)
        a = _gsig(torch, (3, 6 * H), 92)
        calls = [([a[0, :2 * H], a[1, :0], a[2, :H]], [4, 1, 6]),
                 ([a[2, H:5 * H], a[0, 2 * H:3 * H]], [6, 4]),
                 ([a[1, :3 * H]], [1])]
        pool = torch.zeros((POOL, S), device="cuda")
        want = [_pool_call(torch, sslib, cfg, chunks, slots, pool, POOL, fn) for chunks, slots in calls]
        np_ = lambda t: t.cpu().numpy() if torch.is_tensor(t) else t  # noqa: E731
        flat = lambda t: np_(torch.view_as_real(t) if torch.is_tensor(t) and t.is_complex() else t)  # noqa: E731
        for to in (lambda t: t, lambda t: t.cpu().numpy()):
            m = (ss.MelSpectrogramStreamPool if fn == "mel" else ss.StftStreamPool)(POOL, **cls_kw)
            assert m.hop == H and m.state_len == S
            for k, (chunks, slots) in enumerate(calls):
                if k == 1:  # the packed-buffer form
                    rows, ro = m(to(torch.cat(chunks)), slots, lengths=[int(c.numel()) for c in chunks])
                else:
                    rows, ro = m([to(c) for c in chunks], slots)
                assert torch.is_tensor(rows) == torch.is_tensor(to(chunks[0]))
                assert np.array_equal(ro, want[k][1])
                w = want[k][0].cpu().numpy()
                if fn == "mel":
                    assert rows.shape == (M * int(ro[-1]),) and np.array_equal(np_(rows), w)
                else:
                    assert rows.shape == (int(ro[-1]), F) and str(rows.dtype).endswith("complex64")
                    got = flat(rows) if torch.is_tensor(rows) else np.stack([rows.real, rows.imag], axis=-1)
                    assert np.array_equal(got, w)
            torch.cuda.synchronize()
            assert m.state.shape == (POOL, S) and np.array_equal(np_(m.state), pool.cpu().numpy())
            # reset(slots=[...]) makes exactly those streams fresh
            m.reset(slots=[4])
            st = np_(m.state)
            assert not st[4].any() and np.array_equal(st[6], pool[6].cpu().numpy()) and np.array_equal(st[1], pool[1].cpu().numpy())
            m.reset()
            assert not np_(m.state).any()


@pytest.mark.gpu
@pytest.mark.parametrize("kernel,fn", [("headline", "mel"), ("generic", "stft")])
def test_streams_left_out_are_untouched(ss, sslib, kernel, fn):
    """Pool rows not named in `slots`, and rows named by entries without samples, are bit-identical before and after."""
    import torch

    cfg = _cfg(ss, **(CFG3 if kernel == "headline" else ODD_HOP))
    H, S, _, _ = _dims(cfg)
    POOL = 40
    rng = np.random.default_rng(93)
    pool = _gsig(torch, (POOL, S), 94)
    before = pool.clone()
    named = rng.permutation(POOL)[:17]
    hops = rng.integers(0, 4, named.size)
    hops[:3] = 0
    chunks = [_gsig(torch, (int(h) * H,), 95 + i) for i, h in enumerate(hops)]
    _pool_call(torch, sslib, cfg, chunks, named, pool, POOL, fn)
    moved = {int(s) for s, h in zip(named, hops) if h > 0}
    for r in range(POOL):
        assert torch.equal(pool[r], before[r]) == (r not in moved), r
    for s, c in zip(named, chunks):
        if c.numel():
            assert torch.equal(pool[s], torch.cat([before[s], c])[-S:])
