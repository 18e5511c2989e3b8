"""Streaming STFT / mel spectrogram with a carried state per stream: ss_stream_state_len, ss_stream_rows, ss_stft_stream /
ss_mel_spectrogram_stream (host pointers), their *_device forms, and the Python front's MelSpectrogramStream / StftStream.

Every stream carries the last S = W - H samples it was fed (the reference's analysis_mem, config.rs:162, functions.rs:137-160).
Continuous mode: chunks of whole hops, one real row per hop, the same rows however the stream is cut (= the real rows of the
one-shot call on zeros(n_pad H) ++ s).  Reference mode: what stft1 / mel_spectrogram1 return on a SpeechConfig that has seen the
earlier chunks.  Expected values come from the f64 oracle on explicit histories.
"""
import ctypes as C

import numpy as np
import pytest

from common import BENCH_KERNELS, CONFIGS, RTOL

REF, CONT = 0, 1  # SS_STREAM_REFERENCE, SS_STREAM_CONTINUOUS

CFG3 = dict(CONFIGS["cfg3"])  # 2048 / 512, 128 filters: the dedicated kernel's shape
CFG3_KW = dict(frame_length=0.032, num_filters=128, fft_length=2048, high_frequency=8000.0)
ODD_HOP = dict(sample_rate=16000, fft_points=2048, frame_length=600 / 16000, num_filters=64)  # H = 600 does not divide W
CHIRPZ = dict(sample_rate=16000, fft_points=1000, frame_length=400 / 16000, num_filters=40)  # chirp-z W = 1000, H = 400
SWEEP = [CFG3, ODD_HOP, CHIRPZ, dict(sample_rate=16000, fft_points=512, frame_length=0.016),
         dict(sample_rate=16000, fft_points=1024, frame_length=333 / 16000), dict(sample_rate=22050, fft_points=441, frame_length=0.01)]


def _hop(p):
    return int(np.float32(p.frame_length) * np.float32(p.sample_rate))


def _sizes(sslib, p):
    S = C.c_size_t()
    rc = sslib.ss_stream_state_len(C.byref(p), C.byref(S))
    return rc, S.value


def _rows(sslib, p, mode, n):
    r, rr = C.c_size_t(), C.c_size_t()
    rc = sslib.ss_stream_rows(C.byref(p), mode, n, C.byref(r), C.byref(rr))
    return rc, r.value, rr.value


# ---- the expectation builder (oracle on explicit histories) --------------------------------------------------------------------

def expect_continuous(oracle, p, s, fn="mel"):
    """Rows of a continuous stream fed s (any cut): the real rows of the one-shot call on zeros(n_pad H) ++ s."""
    H, n_pad, _ = oracle.stft_sizes(p)
    T = s.shape[-1] // H
    x = np.concatenate([np.zeros(s.shape[:-1] + (n_pad * H,), np.float32), s], axis=-1)
    if fn == "mel":
        return oracle.mel_spectrogram(p, np.atleast_2d(x))[..., :T]
    return oracle.stft(p, np.atleast_2d(x))[:, :T]


def expect_reference(oracle, p, chunks, fn="mel"):
    """Per call k: rows P/H ... of the stateless oracle on (earlier chunks, each zero-padded to whole hops) ++ chunk k."""
    H, _, _ = oracle.stft_sizes(p)
    hist = np.zeros(np.atleast_2d(chunks[0]).shape[:-1] + (0,), np.float32)
    out = []
    for c in chunks:
        c = np.atleast_2d(c)
        P = hist.shape[-1]
        x = np.concatenate([hist, c], axis=-1)
        R = -(-c.shape[-1] // H)
        if fn == "mel":
            out.append(oracle.mel_spectrogram(p, x)[..., P // H:P // H + R])
        else:
            out.append(oracle.stft(p, x)[:, P // H:P // H + R])
        pad = R * H - c.shape[-1]
        hist = np.concatenate([x, np.zeros(c.shape[:-1] + (pad,), np.float32)], axis=-1)
    return out


def rel(got, want):
    """max |got - want| over max |want| (complex rows included), as tests/common.py's rel"""
    got, want = np.asarray(got), np.asarray(want)
    return float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-30))


def _sig(rng, shape):
    return (rng.standard_normal(shape) * 0.1).astype(np.float32)


# ---------------------------------------------------------------- CPU ---------------------------------------------------------

@pytest.mark.parametrize("kw", SWEEP, ids=lambda k: f"W{k['fft_points']}")
def test_state_len_and_rows_follow_the_formulas(sslib, kw):
    from speechsauce_amd import _lib

    p = _lib.make_params(**kw)
    H = _hop(p)
    W = p.fft_points
    n_pad = W // H - 1
    rc, S = _sizes(sslib, p)
    assert rc == 0 and S == W - H and S >= H
    for n in (1, H - 1, H, H + 1, 2 * H, 5 * H - 3, 16 * H, 16000):
        rc, R, Rr = _rows(sslib, p, REF, n)
        assert rc == 0
        assert R == -(-n // H) and Rr == max(R - n_pad, 0), (n, R, Rr)
        rc, R, Rr = _rows(sslib, p, CONT, n)
        if n % H:
            assert rc == 3, n  # SS_ERR_ARG: continuous mode takes whole hops
        else:
            assert rc == 0 and R == Rr == n // H
    assert _rows(sslib, p, CONT, 0)[0] == 3 and _rows(sslib, p, REF, 0)[0] == 3
    assert _rows(sslib, p, 2, H)[0] == 3  # unknown mode


def test_configs_without_an_stft_path_are_bad_configs(sslib):
    from speechsauce_amd import _lib

    p = _lib.make_params(sample_rate=16000, fft_points=512, frame_length=300 / 16000)  # W < 2H
    assert _sizes(sslib, p)[0] == 2
    assert _rows(sslib, p, CONT, 300)[0] == 2
    assert _rows(sslib, p, REF, 300)[0] == 2


def test_reference_mode_is_stateless_exactly_when_the_hop_divides_the_window(oracle):
    """The D3 observation: with H | W the n_pad rows the reference drops are exactly those that see the carried state."""
    rng = np.random.default_rng(1)
    for kw, divides in ((CFG3, True), (ODD_HOP, False)):
        p = oracle.make_params(**kw)
        H, _, _ = oracle.stft_sizes(p)
        chunks = [_sig(rng, (2, k * H)) for k in (4, 5, 6)]
        want = expect_reference(oracle, p, chunks)
        stateless = [oracle.mel_spectrogram(p, c) for c in chunks]
        same = all(np.array_equal(w, s) for w, s in zip(want[1:], stateless[1:]))
        assert same == divides, kw
        assert np.array_equal(want[0], stateless[0])  # the first call starts from zeros either way


def test_continuous_rows_are_the_frames_of_every_hop(oracle):
    """Continuous row g ends at hop g + 1 of the stream; the stateless call's row i ends at hop i + n_pad + 1: the same frames."""
    rng = np.random.default_rng(2)
    for kw in (CFG3, ODD_HOP):
        p = oracle.make_params(**kw)
        H, n_pad, _ = oracle.stft_sizes(p)
        s = _sig(rng, (2, 12 * H))
        whole = expect_continuous(oracle, p, s)
        assert whole.shape == (2, p.num_filters, 12)
        stateless = oracle.mel_spectrogram(p, s)
        assert np.array_equal(whole[..., n_pad:], stateless[..., :12 - n_pad])
        assert np.abs(whole[..., :n_pad]).max() > 0  # the first rows see the stream's start, which the stateless call drops


def test_python_argument_rules(sslib):
    import speechsauce_amd as ss

    m = ss.MelSpectrogramStream(2, 16000, **CFG3_KW)
    assert m.hop == 512 and m.state_len == 1536 and m.state is None and m.mode == "continuous"
    with pytest.raises(TypeError):
        m(np.zeros((2, 1024), np.float64))
    with pytest.raises(ValueError):
        m(np.zeros((3, 1024), np.float32))  # wrong stream count
    with pytest.raises(ValueError):
        m(np.zeros(1024, np.float32))  # 1-D needs n_streams == 1
    with pytest.raises(ValueError):
        m(np.zeros((2, 1000), np.float32))  # not whole hops: raised before anything is launched
    with pytest.raises(ValueError):
        m(np.zeros((2, 2, 512), np.float32))
    assert m.state is None  # nothing was created by the rejected calls
    with pytest.raises(ValueError):
        ss.MelSpectrogramStream(1, 16000, mode="live")
    with pytest.raises(ValueError):
        ss.StftStream(0, 16000)
    with pytest.raises(ss.SpeechSauceError) as e:
        ss.StftStream(1, 16000, frame_length=300 / 16000)  # fft_length 512 < 2 hops: no STFT path
    assert e.value.status == 2
    r = ss.StftStream(1, 16000, mode="reference", fft_length=2048, frame_length=600 / 16000)
    assert r.hop == 600 and r.state_len == 1448
    assert "MelSpectrogramStream" in ss.__all__ and "StftStream" in ss.__all__


def test_streaming_calls_reject_bad_arguments_without_a_device(sslib):
    assert sslib.ss_mel_spectrogram_stream_device(None, CONT, None, 1, 512, 512, None, None, None) == 3  # null config
    assert sslib.ss_stft_stream(None, CONT, None, 1, 512, 512, None, None) == 3


# ---------------------------------------------------------------- GPU ---------------------------------------------------------

def _cfg(ss, **kw):
    from speechsauce_amd import _lib

    return ss.SpeechConfig(_lib.make_params(**kw))


def _dev_call(torch, sslib, cfg, mode, x, state, fn="mel", stream=None):
    """One *_stream_device call on [B, n] x; returns the output tensor (mel [B, M, R] / stft [B, R, F, 2])."""
    B, n = x.shape
    r, rr = C.c_size_t(), C.c_size_t()
    assert sslib.ss_stream_rows(C.byref(cfg.params), mode, n, C.byref(r), C.byref(rr)) == 0
    R = r.value
    if fn == "mel":
        out = torch.full((B, cfg.params.num_filters, R), float("nan"), device="cuda")
        f = sslib.ss_mel_spectrogram_stream_device
    else:
        out = torch.full((B, R, cfg.params.fft_points // 2 + 1, 2), float("nan"), device="cuda")
        f = sslib.ss_stft_stream_device
    st = C.c_void_p(stream if stream is not None else torch.cuda.current_stream().cuda_stream)
    rc = f(cfg.handle, mode, x.data_ptr(), B, n, x.stride(0) if B > 1 else n, state.data_ptr(), out.data_ptr(), st)
    assert rc == 0, sslib.ss_last_error_string()
    return out


def _oneshot_mel(torch, sslib, cfg, x):
    B, n = x.shape
    r, rr = C.c_size_t(), C.c_size_t()
    assert sslib.ss_stft_rows(C.byref(cfg.params), n, C.byref(r), C.byref(rr)) == 0
    out = torch.empty((B, cfg.params.num_filters, r.value), device="cuda")
    assert sslib.ss_mel_spectrogram_device(cfg.handle, x.data_ptr(), B, n, n, out.data_ptr(), None) == 0
    return out


def _gsig(torch, shape, seed):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    return torch.randn(shape, generator=g, device="cuda", dtype=torch.float32).mul_(0.1)


def _feed(torch, sslib, cfg, mode, s, cuts, fn="mel", state=None):
    B = s.shape[0]
    S = cfg.params.fft_points - _hop(cfg.params)
    state = torch.zeros((B, S), device="cuda") if state is None else state
    outs, names, at = [], [], 0
    for c in cuts:
        outs.append(_dev_call(torch, sslib, cfg, mode, s[:, at:at + c].contiguous(), state, fn))
        names.append(sslib.ss_last_kernel_name())
        at += c
    return outs, names, state


def _cfg3_continuous_bits(torch, ss, sslib):
    """256 streams fed 1, 3, 16, 1, 8 hops against the one-shot call on zeros(n_pad H) ++ s; returns the rows, the signal and the
    two kernel names."""
    cfg = _cfg(ss, **CFG3)
    H = 512
    cuts = [1, 3, 16, 1, 8]
    B = 256
    s = _gsig(torch, (B, sum(cuts) * H), 3)
    outs, names, state = _feed(torch, sslib, cfg, CONT, s, [c * H for c in cuts])
    assert len(set(names)) == 1, names
    got = torch.cat(outs, dim=2)
    padded = torch.cat([torch.zeros((B, 3 * H), device="cuda"), s], dim=1).contiguous()
    one = _oneshot_mel(torch, sslib, cfg, padded)
    one_name = sslib.ss_last_kernel_name()
    torch.cuda.synchronize()
    assert torch.equal(got, one[:, :, :sum(cuts)])
    # another cut of the same stream: the same bits, the same final state
    outs2, _, state2 = _feed(torch, sslib, cfg, CONT, s, [c * H for c in (2, 2, 2, 10, 13)])
    assert torch.equal(torch.cat(outs2, dim=2), got) and torch.equal(state2, state)
    assert torch.equal(state, s[:, -1536:])
    return got, s, names[0], one_name


@pytest.mark.gpu
def test_cfg3_continuous_equals_the_one_shot_call_bit_for_bit(ss, sslib, sslab, oracle):
    import torch

    # product library, automatic choice: the streaming launcher picks the build the one-shot launcher picks for the same unit
    # count (eight waves for these shapes on a 256-CU part)
    got, s, name, one_name = _cfg3_continuous_bits(torch, ss, sslib)
    assert name.startswith(b"ss_mel_c1024s") and name == one_name.replace(b"ss_mel_c1024", b"ss_mel_c1024s"), (name, one_name)
    # the twelve-wave builds, forced on both sides through the lab library's selector
    with ss._lib.use_library(sslab):
        try:
            sslab.ss_debug_mel_tile(3)
            _, _, name12, one12 = _cfg3_continuous_bits(torch, ss, sslab)
        finally:
            sslab.ss_debug_mel_tile(1)
    assert (name12, one12) == (b"ss_mel_c1024s<w12,mel6321>", BENCH_KERNELS["cfg3"])
    p = oracle.make_params(**CFG3)
    pick = [0, 77, 255]
    want = expect_continuous(oracle, p, s[pick].cpu().numpy())
    g = got[pick].cpu().numpy()
    for i in range(len(pick)):
        assert rel(g[i], want[i]) <= RTOL, pick[i]


@pytest.mark.gpu
def test_cfg3_reference_mode_equals_the_stateless_call(ss, sslib, oracle):
    import torch

    cfg = _cfg(ss, **CFG3)
    H = 512
    cuts = [16 * H, 2 * H, 5 * H, 7 * H - 100, 3 * H + 1]  # real_rows 0 in the second call, partial last chunks
    B = 64
    s = _gsig(torch, (B, sum(cuts)), 4)
    outs, names, state = _feed(torch, sslib, cfg, REF, s, cuts)
    at = 0
    for c, o, nm in zip(cuts, outs, names):
        assert nm.startswith(b"ss_mel_c1024s"), nm
        one = _oneshot_mel(torch, sslib, cfg, s[:, at:at + c].contiguous())
        assert torch.equal(o, one), c
        at += c
    assert torch.count_nonzero(outs[1]) == 0 and outs[1].shape[2] == 2
    p = oracle.make_params(**CFG3)
    want = expect_reference(oracle, p, [s[:3, a:a + c].cpu().numpy() for a, c in zip(np.cumsum([0] + cuts[:-1]), cuts)])
    for o, w in zip(outs, want):
        for b in range(3):
            assert rel(o[b].cpu().numpy(), w[b]) <= RTOL


@pytest.mark.gpu
@pytest.mark.parametrize("kw", [ODD_HOP, CHIRPZ], ids=["W2048_H600", "chirpz_W1000_H400"])
@pytest.mark.parametrize("fn", ["mel", "stft"])
def test_other_shapes_match_the_oracle_in_both_modes(ss, sslib, oracle, kw, fn):
    import torch

    cfg = _cfg(ss, **kw)
    H = _hop(cfg.params)
    p = oracle.make_params(**kw)
    B = 5
    # continuous
    cuts = [3 * H, H, 6 * H, 2 * H]
    s = _gsig(torch, (B, sum(cuts)), 5)
    outs, names, _ = _feed(torch, sslib, cfg, CONT, s, cuts, fn)
    # launch_stft's candidate order: a 2048-point mel spectrogram (any hop) on the dedicated kernel's streaming build, the rest on
    # the generic kernel's
    build = b"ss_mel_c1024s" if fn == "mel" and kw["fft_points"] == 2048 else b"ss_front_generic_stream<"
    assert all(n.startswith(build) for n in names), names
    got = torch.cat(outs, dim=2 if fn == "mel" else 1).cpu().numpy()
    if fn == "stft":
        got = got[..., 0] + 1j * got[..., 1]
    want = expect_continuous(oracle, p, s.cpu().numpy(), fn)
    for b in range(B):
        assert rel(got[b], want[b]) <= RTOL, b
    # reference: partial chunks too; after a call of whole hops the next call's first row depends on the state (after a partial
    # chunk the state ends in the chunk's zero padding, more of it than the first row reads)
    cuts = [4 * H, 3 * H + 17, 5 * H, 6 * H - 1]
    s = _gsig(torch, (B, sum(cuts)), 6)
    outs, _, _ = _feed(torch, sslib, cfg, REF, s, cuts, fn)
    starts = np.cumsum([0] + cuts[:-1])
    want = expect_reference(oracle, p, [s[:, a:a + c].cpu().numpy() for a, c in zip(starts, cuts)], fn)
    for k, (o, w) in enumerate(zip(outs, want)):
        g = o.cpu().numpy()
        if fn == "stft":
            g = g[..., 0] + 1j * g[..., 1]
        for b in range(B):
            assert rel(g[b], w[b]) <= RTOL, (k, b)
        if k in (1, 3):
            stateless = _dev_call(torch, sslib, cfg, REF, s[:, starts[k]:starts[k] + cuts[k]].contiguous(),
                                  torch.zeros((B, cfg.params.fft_points - H), device="cuda"), fn)
            first = (lambda t: t[:, :, 0]) if fn == "mel" else (lambda t: t[:, 0])
            assert not torch.equal(first(o), first(stateless)), k


@pytest.mark.gpu
def test_streams_are_independent_and_reset_by_zeroing_their_row(ss, sslib):
    import torch

    cfg = _cfg(ss, **ODD_HOP)
    H = 600
    B = 7
    s = _gsig(torch, (B, 9 * H), 7)
    perm = torch.tensor([3, 0, 6, 1, 5, 2, 4], device="cuda")
    a, _, _ = _feed(torch, sslib, cfg, REF, s, [4 * H, 5 * H])
    b, _, _ = _feed(torch, sslib, cfg, REF, s[perm].contiguous(), [4 * H, 5 * H])
    for x, y in zip(a, b):
        assert torch.equal(x[perm], y)
    # zero stream 2's state between the calls: stream 2 restarts fresh, the others go on
    state = torch.zeros((B, 2048 - H), device="cuda")
    _dev_call(torch, sslib, cfg, REF, s[:, :4 * H].contiguous(), state)
    state[2].zero_()
    second = _dev_call(torch, sslib, cfg, REF, s[:, 4 * H:].contiguous(), state)
    fresh = _dev_call(torch, sslib, cfg, REF, s[:, 4 * H:].contiguous(), torch.zeros((B, 2048 - H), device="cuda"))
    assert torch.equal(second[2], fresh[2])
    keep = [i for i in range(B) if i != 2]
    assert torch.equal(second[keep], a[1][keep])


@pytest.mark.gpu
@pytest.mark.parametrize("kw", [CFG3, ODD_HOP], ids=["cfg3", "W2048_H600"])
def test_graph_replay_gives_the_eager_bits_and_state(ss, sslib, kw):
    import torch

    cfg = _cfg(ss, **kw)
    H = _hop(cfg.params)
    B, K, hops = 32, 4, 3
    S = cfg.params.fft_points - H
    chunks = [_gsig(torch, (B, hops * H), 20 + k) for k in range(K)]
    # eager
    st_e = torch.zeros((B, S), device="cuda")
    eager = [_dev_call(torch, sslib, cfg, CONT, c, st_e).clone() for c in chunks]
    # captured: one call over a static chunk buffer
    xbuf = torch.zeros((B, hops * H), device="cuda")
    st_g = torch.zeros((B, S), device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):  # warm-up off the capture, on a scratch state
        _dev_call(torch, sslib, cfg, CONT, xbuf, torch.zeros_like(st_g), stream=s.cuda_stream)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = _dev_call(torch, sslib, cfg, CONT, xbuf, st_g, stream=torch.cuda.current_stream().cuda_stream)
    for k in range(K):
        xbuf.copy_(chunks[k])
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager[k]), k
    assert torch.equal(st_g, st_e)
    cfg.device_status()


@pytest.mark.gpu
@pytest.mark.parametrize("fn", ["mel", "stft"])
def test_host_entry_points_equal_the_device_ones(ss, sslib, fn):
    import torch

    for kw in (CFG3, CHIRPZ):
        cfg = _cfg(ss, **kw)
        H = _hop(cfg.params)
        S = cfg.params.fft_points - H
        B = 6
        cuts = [2 * H, 5 * H + 3, H - 1]
        s = _gsig(torch, (B, sum(cuts)), 30)
        outs, _, st_d = _feed(torch, sslib, cfg, REF, s, cuts, fn)
        sh = s.cpu().numpy()
        st_h = np.zeros((B, S), np.float32)
        at = 0
        host_fn = sslib.ss_mel_spectrogram_stream if fn == "mel" else sslib.ss_stft_stream
        for c, o in zip(cuts, outs):
            x = np.ascontiguousarray(sh[:, at:at + c])
            out = np.empty(tuple(o.shape), np.float32)
            assert host_fn(cfg.handle, REF, x.ctypes.data, B, c, c, st_h.ctypes.data, out.ctypes.data) == 0
            assert np.array_equal(out, o.cpu().numpy())
            at += c
        assert np.array_equal(st_h, st_d.cpu().numpy())
        # rejected calls leave the state bytes as they were
        before = st_h.copy()
        x = np.ascontiguousarray(sh[:, :H + 1])
        out = np.empty((B, 2 * (cfg.params.fft_points // 2 + 1) * 2 + cfg.params.num_filters * 2), np.float32)
        assert host_fn(cfg.handle, CONT, x.ctypes.data, B, H + 1, H + 1, st_h.ctypes.data, out.ctypes.data) == 3  # not whole hops
        assert host_fn(cfg.handle, REF, x.ctypes.data, B, H + 1, H, st_h.ctypes.data, out.ctypes.data) == 3  # ld < n
        assert host_fn(cfg.handle, REF, st_h.ctypes.data, 1, H, H, st_h.ctypes.data, out.ctypes.data) == 3  # state overlaps x
        assert np.array_equal(st_h, before)
        xd = torch.from_numpy(x).cuda()
        before_d = st_d.clone()
        dev_fn = sslib.ss_mel_spectrogram_stream_device if fn == "mel" else sslib.ss_stft_stream_device
        od = torch.empty(1 << 20, device="cuda")
        assert dev_fn(cfg.handle, CONT, xd.data_ptr(), B, H + 1, H + 1, st_d.data_ptr(), od.data_ptr(), None) == 3
        assert dev_fn(cfg.handle, REF, xd.data_ptr(), B, H + 1, H + 1, st_d.data_ptr(), st_d.data_ptr(), None) == 3  # overlaps out
        assert dev_fn(cfg.handle, REF, xd.data_ptr(), 0, H + 1, H + 1, None, None, None) == 0  # no streams: nothing launched
        torch.cuda.synchronize()
        assert torch.equal(st_d, before_d)


@pytest.mark.gpu
def test_python_front_on_rocm_tensors_and_numpy(ss, sslib, oracle):
    import torch

    B, H = 256, 512
    s = _gsig(torch, (B, 29 * H), 3)
    m = ss.MelSpectrogramStream(B, 16000, **CFG3_KW)
    got = torch.cat([m(s[:, a * H:(a + c) * H]) for a, c in ((0, 1), (1, 3), (4, 16), (20, 1), (21, 8))], dim=2)
    assert isinstance(m.state, torch.Tensor) and m.state.shape == (B, 1536)
    outs, _, state = _feed(torch, sslib, _cfg(ss, **CFG3), CONT, s, [c * H for c in (1, 3, 16, 1, 8)])
    torch.cuda.synchronize()
    assert torch.equal(got, torch.cat(outs, dim=2)) and torch.equal(m.state, state)
    p = oracle.make_params(**CFG3)
    assert rel(got[9].cpu().numpy(), expect_continuous(oracle, p, s[9:10].cpu().numpy())[0]) <= RTOL
    with pytest.raises(ValueError):
        m(s[:, :H].cpu().numpy())  # the state lives on the device
    mh = ss.MelSpectrogramStream(B, 16000, **CFG3_KW)
    host = np.concatenate([mh(s[:, a * H:(a + 4) * H].cpu().numpy()) for a in range(0, 28, 4)] + [mh(s[:, 28 * H:].cpu().numpy())], axis=2)
    assert isinstance(mh.state, np.ndarray) and np.array_equal(host, got.cpu().numpy())
    # reset: a fresh start for the chosen streams only
    m.reset([0, 5])
    again = m(s[:, :4 * H])
    fresh = ss.MelSpectrogramStream(B, 16000, **CFG3_KW)(s[:, :4 * H])
    assert torch.equal(again[[0, 5]], fresh[[0, 5]]) and not torch.equal(again[1], fresh[1])
    # StftStream, reference mode at H = 600 and the chirp-z size, against the oracle
    for kw in (ODD_HOP, CHIRPZ):
        Hs = _hop(_cfg(ss, **kw).params)
        p = oracle.make_params(**kw)
        st = ss.StftStream(3, kw["sample_rate"], frame_length=kw["frame_length"], fft_length=kw["fft_points"], mode="reference")
        x = _gsig(torch, (3, 7 * Hs + 11), 40)
        cuts = [2 * Hs, 3 * Hs + 5, 2 * Hs + 6]
        starts = np.cumsum([0] + cuts[:-1])
        want = expect_reference(oracle, p, [x[:, a:a + c].cpu().numpy() for a, c in zip(starts, cuts)], "stft")
        for a, c, w in zip(starts, cuts, want):
            z = st(x[:, a:a + c])
            assert z.dtype == torch.complex64 and z.shape == w.shape
            assert rel(z.cpu().numpy(), w) <= RTOL
        one = ss.StftStream(1, kw["sample_rate"], frame_length=kw["frame_length"], fft_length=kw["fft_points"])
        zh = one(x[0, :4 * Hs].cpu().numpy())
        assert isinstance(zh, np.ndarray) and zh.shape == (1, 4, kw["fft_points"] // 2 + 1)
        assert rel(zh[0], expect_continuous(oracle, p, x[:1, :4 * Hs].cpu().numpy(), "stft")[0]) <= RTOL
