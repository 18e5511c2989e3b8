"""Streaming MFCC / mfe with a carried frame state per stream: ss_frame_stream_state_len, ss_frame_stream_rows, ss_mfcc_stream /
ss_mfe_stream (host pointers), their *_device forms, and the Python front's MfccStream / MfeStream.

Every stream carries the last S = max(flen + sh - step, 0) samples it was fed.  A call of n = R * step samples gives R rows; row g
of a stream (hops since its reset) is the frame s[(g+1) step - flen : (g+1) step] with zeros before the stream's start.  With G rows
fed, the rows equal rows 1 .. G of the one-shot call on zeros(flen) ++ s ++ zeros(step) (G + 1 frames), whose reference DCT scaling
then uses T = G + 1 = norm_frames.  Expected values come from that one-shot call or from the f64 oracle on the same signal.
"""
import ctypes as C

import numpy as np
import pytest

from common import BENCH_KERNELS, RTOL, rel

EPS = np.float32(np.finfo(np.float32).eps)
STREAM_KERNEL = b"ss_mfcc_c256s<10,exact,bank421,sym>"
STREAM_MFE_KERNEL = b"ss_mfcc_c256s<10,exact,bank421,mfe>"

# every other configuration runs on the generic kernel's streaming build
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


def _equivalence_signal(s, flen, step):
    """zeros(flen) ++ s ++ zeros(step): its one-shot frames 1 .. G are a stream's rows 0 .. G - 1"""
    B = s.shape[0]
    if isinstance(s, np.ndarray):
        return np.concatenate([np.zeros((B, flen), np.float32), s, np.zeros((B, step), np.float32)], axis=1)
    import torch

    z = torch.zeros
    return torch.cat([z((B, flen), device=s.device), s, z((B, step), device=s.device)], dim=1).contiguous()


# ---------------------------------------------------------------- CPU ---------------------------------------------------------

def test_state_len_follows_the_formula(sslib):
    from speechsauce_amd import _lib

    for kw, want in ((dict(), 160), (dict(preemph_coef=0.97, preemph_shift=1), 161), (dict(frame_length=0.01), 0),
                     (dict(frame_length=0.01, frame_stride=0.02), 0), (dict(preemph_coef=0.97, preemph_shift=160), 320),
                     (dict(framing="padded"), 160), (dict(preemph_shift=7), 160)):
        rc, fl, st, S = _sizes(sslib, _lib.make_params(**kw))
        assert rc == 0 and S == want, (kw, S)
    for framing in ("literal", "center"):
        p = _lib.make_params(framing=framing)
        assert _sizes(sslib, p)[0] == 2  # SS_ERR_BAD_CONFIG: a stream has no clip end
        r = C.c_size_t()
        assert sslib.ss_frame_stream_rows(C.byref(p), 1600, C.byref(r)) == 2


def test_rows_are_whole_hops(sslib):
    from speechsauce_amd import _lib

    for kw in (dict(), dict(frame_length=0.025, frame_stride=0.015), dict(sample_rate=8000, frame_stride=0.0125)):
        p = _lib.make_params(**kw)
        _, _, step, _ = _sizes(sslib, p)
        r = C.c_size_t()
        for k in (1, 2, 16, 100):
            assert sslib.ss_frame_stream_rows(C.byref(p), k * step, C.byref(r)) == 0 and r.value == k
        for n in (0, 1, step - 1, step + 1, 16 * step + 3):
            assert sslib.ss_frame_stream_rows(C.byref(p), n, C.byref(r)) == 3, n  # SS_ERR_ARG


def test_compute_entries_reject_a_null_config(sslib):
    assert sslib.ss_mfcc_stream_device(None, None, 1, 160, 160, 1, None, None, None) == 3
    assert sslib.ss_mfe_stream_device(None, None, 1, 160, 160, None, None, None, None) == 3
    assert sslib.ss_mfcc_stream(None, None, 1, 160, 160, 1, None, None) == 3
    assert sslib.ss_mfe_stream(None, None, 1, 160, 160, None, None, None) == 3


def _has_gpu():
    try:
        import torch

        return torch.cuda.is_available()
    except Exception:
        return False


@pytest.mark.skipif(_has_gpu(), reason="checks the no-device failure mode")
def test_compute_entries_fail_loudly_without_a_device(sslib):
    import speechsauce_amd as ss
    from speechsauce_amd import SpeechSauceError, make_params

    cfg = C.c_void_p()
    assert sslib.ss_config_create(C.byref(make_params()), C.byref(cfg)) == 4  # SS_ERR_HIP: no config, no call
    for obj in (ss.MfccStream(2, 16000, norm_frames=100), ss.MfeStream(2, 16000)):
        with pytest.raises(SpeechSauceError) as e:
            obj(np.zeros((2, 320), np.float32))
        assert e.value.status == 4


def test_python_argument_rules(sslib):
    import speechsauce_amd as ss

    m = ss.MfccStream(2, 16000, norm_frames=101)
    assert m.hop == 160 and m.frame_len == 320 and m.state_len == 160 and m.state is None and m.norm_frames == 101
    with pytest.raises(ValueError):
        m(np.zeros(320, np.float32))  # 1-D needs n_streams == 1
    with pytest.raises(ValueError):
        m(np.zeros((3, 320), np.float32))  # wrong stream count
    with pytest.raises(ValueError):
        m(np.zeros((2, 330), np.float32))  # not whole hops
    with pytest.raises(TypeError):
        m(np.zeros((2, 320), np.float64))
    assert m.state is None  # nothing was created by the rejected calls
    with pytest.raises(ValueError):
        ss.MfccStream(2, 16000)  # the reference DCT scaling needs norm_frames
    with pytest.raises(ValueError):
        ss.MfccStream(2, 16000, norm_frames=0)
    assert ss.MfccStream(1, 16000, dct_norm="ortho").state_len == 160  # ortho: norm_frames is not needed
    with pytest.raises(ValueError):
        ss.MfeStream(0, 16000)
    with pytest.raises(ss.SpeechSauceError) as e:
        ss.MfccStream(1, 16000, norm_frames=10, framing="center")
    assert e.value.status == 2
    assert ss.MfeStream(1, 16000, preemph_coef=0.97).state_len == 161
    assert "MfccStream" in ss.__all__ and "MfeStream" in ss.__all__


def test_oracle_equivalence_signal_has_one_frame_per_hop_plus_one(sslib, oracle):
    """The equivalence signal zeros(flen) ++ s ++ zeros(step) has G + 1 frames under contract and padded framing."""
    from speechsauce_amd import _lib

    for kw in (dict(), dict(framing="padded"), SWEEP["fft1024"], SWEEP["flen_lt_step"], SWEEP["fft4096"]):
        _, flen, step, _ = _sizes(sslib, _lib.make_params(**kw))
        p = oracle.make_params(**kw)
        for G in (1, 5, 16):
            assert oracle.num_frames(p, flen + G * step + step) == G + 1, (kw, G)


# ---------------------------------------------------------------- GPU ---------------------------------------------------------

def _cfg(ss, **kw):
    from speechsauce_amd import _lib

    return ss.SpeechConfig(_lib.make_params(**kw))


def _gsig(torch, shape, seed):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    return torch.randn(shape, generator=g, device="cuda", dtype=torch.float32).mul_(0.1)


def _dev_call(torch, lib, cfg, x, state, norm_frames, fn="mfcc", stream=None):
    """One ss_mfcc_stream_device / ss_mfe_stream_device call on [B, n] x; returns out (mfcc) or (feat, energy)."""
    B, n = x.shape
    r = C.c_size_t()
    assert lib.ss_frame_stream_rows(C.byref(cfg.params), n, C.byref(r)) == 0
    R = r.value
    st = C.c_void_p(stream if stream is not None else torch.cuda.current_stream().cuda_stream)
    sp = state.data_ptr() if state is not None and state.numel() else None
    ld = x.stride(0) if B > 1 else n
    if fn == "mfcc":
        out = torch.full((B, R, cfg.params.num_cepstral), float("nan"), device="cuda")
        rc = lib.ss_mfcc_stream_device(cfg.handle, x.data_ptr(), B, n, ld, norm_frames, sp, out.data_ptr(), st)
        assert rc == 0, lib.ss_last_error_string()
        return out
    feat = torch.full((B, R, cfg.params.num_filters), float("nan"), device="cuda")
    en = torch.full((B, R), float("nan"), device="cuda")
    rc = lib.ss_mfe_stream_device(cfg.handle, x.data_ptr(), B, n, ld, sp, feat.data_ptr(), en.data_ptr(), st)
    assert rc == 0, lib.ss_last_error_string()
    return feat, en


def _feed(torch, lib, cfg, s, cuts, norm_frames, fn="mfcc", state=None):
    """Feed s [B, G * step] in chunks of `cuts` hops; returns the concatenated rows, the kernel names and the state."""
    B = s.shape[0]
    _, _, step, S = _sizes(lib, cfg.params)
    state = torch.zeros((B, S), device="cuda") if state is None else state
    outs, names, at = [], [], 0
    for c in cuts:
        outs.append(_dev_call(torch, lib, cfg, s[:, at:at + c * step].contiguous(), state, norm_frames, fn))
        names.append(lib.ss_last_kernel_name())
        at += c * step
    if fn == "mfcc":
        return torch.cat(outs, dim=1), names, state
    return (torch.cat([o[0] for o in outs], dim=1), torch.cat([o[1] for o in outs], dim=1)), names, state


def _oneshot(torch, lib, cfg, s, fn="mfcc"):
    """Rows 1 .. G of the one-shot device call on the equivalence signal (its T = G + 1 is the stream's norm_frames)."""
    _, flen, step, _ = _sizes(lib, cfg.params)
    x = _equivalence_signal(s, flen, step)
    B, n = x.shape
    T = cfg.num_frames(n)
    assert T == s.shape[1] // step + 1
    if fn == "mfcc":
        out = torch.empty((B, T, cfg.params.num_cepstral), device="cuda")
        assert lib.ss_mfcc_batch_device(cfg.handle, x.data_ptr(), B, n, n, out.data_ptr(), None) == 0, lib.ss_last_error_string()
        return out[:, 1:]
    feat = torch.empty((B, T, cfg.params.num_filters), device="cuda")
    en = torch.empty((B, T), device="cuda")
    assert lib.ss_mfe_batch_device(cfg.handle, x.data_ptr(), B, n, n, feat.data_ptr(), en.data_ptr(), None) == 0
    return feat[:, 1:], en[:, 1:]


@pytest.mark.gpu
@pytest.mark.parametrize("dc", [True, False], ids=["dc_elimination", "no_dc_elimination"])
def test_headline_stream_equals_the_one_shot_call_bit_for_bit(ss, sslib, dc):
    import torch

    cfg = _cfg(ss, dc_elimination=dc)
    B, cuts = 1024, [3, 1, 7, 5]
    G = sum(cuts)
    s = _gsig(torch, (B, G * 160), 11)
    got, names, state = _feed(torch, sslib, cfg, s, cuts, G + 1)
    assert set(names) == {STREAM_KERNEL}, names
    want = _oneshot(torch, sslib, cfg, s)
    torch.cuda.synchronize()
    assert sslib.ss_last_kernel_name() == BENCH_KERNELS["cfg2"]
    assert got.shape == (B, G, 13) and torch.isfinite(got).all()
    assert torch.equal(got, want)
    assert torch.equal(state, s[:, -160:])


@pytest.mark.gpu
def test_cut_independence_one_hop_per_call(ss, sslib):
    import torch

    cfg = _cfg(ss)
    B, G = 1024, 16
    s = _gsig(torch, (B, G * 160), 12)
    whole, _, st1 = _feed(torch, sslib, cfg, s, [G], 50)
    hops, names, st2 = _feed(torch, sslib, cfg, s, [1] * G, 50)
    torch.cuda.synchronize()
    assert set(names) == {STREAM_KERNEL}
    assert torch.equal(whole, hops) and torch.equal(st1, st2)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SWEEP))
def test_generic_stream_matches_the_oracle(ss, sslib, oracle, name):
    import torch

    kw = SWEEP[name]
    cfg = _cfg(ss, **kw)
    rc, flen, step, S = _sizes(sslib, cfg.params)
    assert rc == 0
    B, cuts = 3, [2, 1, 5]
    G = sum(cuts)
    s = _gsig(torch, (B, G * step), 13)
    state = None if S else torch.zeros((B, 0), device="cuda")  # S == 0: a null state pointer
    got, names, _ = _feed(torch, sslib, cfg, s, cuts, G + 1, state=state)
    torch.cuda.synchronize()
    assert all(n.startswith(b"ss_front_generic_fstream<") for n in names), names
    p = oracle.make_params(**kw)
    x = _equivalence_signal(s.cpu().numpy(), flen, step)
    g = got.cpu().numpy()
    for b in range(B):
        want = oracle.mfcc(p, x[b])[1:]
        assert rel(g[b], want) <= RTOL, (name, b, rel(g[b], want))
    # one call of all G hops: the same bits
    whole, _, _ = _feed(torch, sslib, cfg, s, [G], G + 1, state=None if S else torch.zeros((B, 0), device="cuda"))
    torch.cuda.synchronize()
    assert torch.equal(whole, got)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["default", "preemph1", "hann", "chirpz", "ortho", "fft4096"])
def test_forced_generic_stream_equals_the_forced_generic_one_shot_call(ss, sslab, name):
    import torch

    from speechsauce_amd import _lib

    kw = {} if name == "default" else SWEEP[name]
    with _lib.use_library(sslab):
        sslab.ss_debug_force_generic(1)
        try:
            for fn in ("mfcc", "mfe"):
                cfg = _cfg(ss, **kw)
                _, _, step, _ = _sizes(sslab, cfg.params)
                B, cuts = 5, [1, 4, 2]
                s = _gsig(torch, (B, sum(cuts) * step), 14)
                got, names, _ = _feed(torch, sslab, cfg, s, cuts, sum(cuts) + 1, fn=fn)
                want = _oneshot(torch, sslab, cfg, s, fn=fn)
                torch.cuda.synchronize()
                assert names[0].startswith(b"ss_front_generic_fstream<")
                if fn == "mfcc":
                    assert torch.equal(got, want)
                else:
                    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
        finally:
            sslab.ss_debug_force_generic(0)


@pytest.mark.gpu
def test_mfe_stream_matches_one_shot_and_oracle(ss, sslib, oracle):
    import torch

    cfg = _cfg(ss, num_cepstral=13)
    B, cuts = 64, [4, 1, 3]
    G = sum(cuts)
    s = _gsig(torch, (B, G * 160), 15)
    s[7] = 0.0  # an all-zero stream: every feature and energy is EPS exactly (feature.rs:216-230)
    (feat, en), names, _ = _feed(torch, sslib, cfg, s, cuts, 1, fn="mfe")
    wf, we = _oneshot(torch, sslib, cfg, s, fn="mfe")
    torch.cuda.synchronize()
    assert set(names) == {STREAM_MFE_KERNEL}, names
    assert torch.equal(feat, wf) and torch.equal(en, we)
    f, e = feat.cpu().numpy(), en.cpu().numpy()
    assert np.all(f[7] == EPS) and np.all(e[7] == EPS)
    p = oracle.make_params()
    x = _equivalence_signal(s.cpu().numpy(), 320, 160)
    for b in (0, 1, 33):
        of, oe = oracle.mfe(p, x[b])
        assert rel(f[b], of[1:]) <= RTOL and rel(e[b], oe[1:]) <= RTOL


@pytest.mark.gpu
@pytest.mark.parametrize("kw", [dict(), dict(preemph_coef=0.97, preemph_shift=1)], ids=["headline", "generic"])
def test_streams_are_independent_and_reset_per_row(ss, sslib, kw):
    import torch

    cfg = _cfg(ss, **kw)
    _, _, step, S = _sizes(sslib, cfg.params)
    B = 8
    a = _gsig(torch, (B, 6 * step), 16)
    b = _gsig(torch, (B, 5 * step), 17)
    # every stream fed different audio: stream k's rows are those of a one-stream feed of its own samples
    rows_a, _, state = _feed(torch, sslib, cfg, a, [6], 40)
    for k in (0, 5):
        alone, _, _ = _feed(torch, sslib, cfg, a[k:k + 1], [2, 4], 40)
        assert torch.equal(rows_a[k:k + 1], alone)
    untouched = state.clone()
    rows_cont, _, _ = _feed(torch, sslib, cfg, b, [5], 40, state=untouched)
    state[3] = 0.0  # reset stream 3
    rows_b, _, _ = _feed(torch, sslib, cfg, b, [5], 40, state=state)
    fresh, _, _ = _feed(torch, sslib, cfg, b[3:4], [5], 40)
    torch.cuda.synchronize()
    assert torch.equal(rows_b[3:4], fresh)
    others = [k for k in range(B) if k != 3]
    assert torch.equal(rows_b[others], rows_cont[others])
    assert not torch.equal(rows_b[3], rows_cont[3])


@pytest.mark.gpu
def test_rejected_device_calls_leave_the_state_untouched(ss, sslib):
    import torch

    cfg = _cfg(ss)
    B = 4
    x = _gsig(torch, (B, 8 * 160), 18)
    state = _gsig(torch, (B, 160), 19)
    before = state.clone()
    out = torch.empty((B, 8, 13), device="cuda")
    h, st = cfg.handle, C.c_void_p(torch.cuda.current_stream().cuda_stream)
    f = sslib.ss_mfcc_stream_device
    assert f(h, x.data_ptr(), B, 8 * 160 - 1, 8 * 160, 10, state.data_ptr(), out.data_ptr(), st) == 3  # partial hop
    assert f(h, x.data_ptr(), B, 8 * 160, 100, 10, state.data_ptr(), out.data_ptr(), st) == 3  # ld < n
    assert f(h, x.data_ptr(), B, 0, 8 * 160, 10, state.data_ptr(), out.data_ptr(), st) == 3  # no samples
    assert f(h, x.data_ptr(), B, 8 * 160, 8 * 160, 0, state.data_ptr(), out.data_ptr(), st) == 3  # norm_frames 0
    assert f(h, x.data_ptr(), B, 8 * 160, 8 * 160, 10, None, out.data_ptr(), st) == 3  # null state with S > 0
    assert f(h, x.data_ptr(), B, 8 * 160, 8 * 160, 10, state.data_ptr(), None, st) == 3  # null output
    assert f(h, x.data_ptr(), 1 << 31, 8 * 160, 8 * 160, 10, state.data_ptr(), out.data_ptr(), st) == 3  # too many streams
    assert f(h, x.data_ptr(), B, 8 * 160, 8 * 160, 10, x.data_ptr() + 4 * 160, out.data_ptr(), st) == 3  # state inside x
    assert f(h, x.data_ptr(), B, 8 * 160, 8 * 160, 10, out.data_ptr(), out.data_ptr(), st) == 3  # state inside out
    en = torch.empty((B, 8), device="cuda")
    fe = sslib.ss_mfe_stream_device
    assert fe(h, x.data_ptr(), B, 8 * 160, 8 * 160, state.data_ptr(), out.data_ptr(), None, st) == 3  # null energy
    assert fe(h, x.data_ptr(), B, 8 * 160, 8 * 160, en.data_ptr(), out.data_ptr(), en.data_ptr(), st) == 3  # state == energy
    assert f(h, x.data_ptr(), 0, 8 * 160, 8 * 160, 10, None, None, st) == 0  # no streams: nothing launched
    torch.cuda.synchronize()
    assert torch.equal(state, before)


@pytest.mark.gpu
def test_graph_replay_equals_eager_calls(ss, sslib):
    import torch

    cfg = _cfg(ss)
    B, K = 1024, 5
    chunks = _gsig(torch, (K, B, 160), 20)
    # eager
    st_e = torch.zeros((B, 160), device="cuda")
    eager = [_dev_call(torch, sslib, cfg, chunks[k], st_e, 100) for k in range(K)]
    # captured: one call on a static input, replayed over new chunks copied into it
    x = torch.zeros((B, 160), device="cuda")
    st_g = torch.zeros((B, 160), device="cuda")
    out = torch.empty((B, 1, 13), device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up outside the capture (on a scratch state)
        _dev_call(torch, sslib, cfg, x, torch.zeros((B, 160), device="cuda"), 100, stream=side.cuda_stream)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        s = torch.cuda.current_stream().cuda_stream
        rc = sslib.ss_mfcc_stream_device(cfg.handle, x.data_ptr(), B, 160, 160, 100, st_g.data_ptr(), out.data_ptr(), C.c_void_p(s))
    assert rc == 0
    replayed = []
    for k in range(K):
        x.copy_(chunks[k])
        g.replay()
        replayed.append(out.clone())
    torch.cuda.synchronize()
    for k in range(K):
        assert torch.equal(replayed[k], eager[k]), k
    assert torch.equal(st_g, st_e)


@pytest.mark.gpu
def test_host_entries_and_python_front_equal_the_device_entries(ss, sslib):
    import torch

    cfg = _cfg(ss)
    B, cuts = 16, [2, 3, 1]
    G = sum(cuts)
    s = _gsig(torch, (B, G * 160), 21)
    dev, _, dstate = _feed(torch, sslib, cfg, s, cuts, 30)
    (dfeat, den), _, _ = _feed(torch, sslib, cfg, s, cuts, 1, fn="mfe")
    torch.cuda.synchronize()
    sh = s.cpu().numpy()
    # host pointers
    state = np.zeros((B, 160), np.float32)
    host, hfeat, hen, at = [], [], [], 0
    mstate = np.zeros((B, 160), np.float32)
    for c in cuts:
        x = np.ascontiguousarray(sh[:, at:at + 160 * c])
        o = np.empty((B, c, 13), np.float32)
        assert sslib.ss_mfcc_stream(cfg.handle, x.ctypes.data, B, 160 * c, 160 * c, 30, state.ctypes.data, o.ctypes.data) == 0
        f = np.empty((B, c, 40), np.float32)
        e = np.empty((B, c), np.float32)
        assert sslib.ss_mfe_stream(cfg.handle, x.ctypes.data, B, 160 * c, 160 * c, mstate.ctypes.data, f.ctypes.data, e.ctypes.data) == 0
        host.append(o), hfeat.append(f), hen.append(e)
        at += 160 * c
    assert np.array_equal(np.concatenate(host, axis=1), dev.cpu().numpy())
    assert np.array_equal(state, dstate.cpu().numpy())
    assert np.array_equal(np.concatenate(hfeat, axis=1), dfeat.cpu().numpy())
    assert np.array_equal(np.concatenate(hen, axis=1), den.cpu().numpy())
    # the Python front, torch and numpy
    for chunk_of in (lambda a, b: s[:, a:b], lambda a, b: sh[:, a:b]):
        m = ss.MfccStream(B, 16000, norm_frames=30)
        e = ss.MfeStream(B, 16000)
        rows, feats, ens, at = [], [], [], 0
        for c in cuts:
            rows.append(m(chunk_of(at, at + 160 * c)))
            f, en = e(chunk_of(at, at + 160 * c))
            feats.append(f), ens.append(en)
            at += 160 * c
        np_ = (lambda t: t.cpu().numpy()) if torch.is_tensor(rows[0]) else (lambda t: t)
        assert np.array_equal(np.concatenate([np_(r) for r in rows], axis=1), dev.cpu().numpy())
        assert np.array_equal(np.concatenate([np_(f) for f in feats], axis=1), dfeat.cpu().numpy())
        assert np.array_equal(np.concatenate([np_(t) for t in ens], axis=1), den.cpu().numpy())
        assert np.array_equal(np_(m.state), sh[:, -160:])
        m.reset([1])
        assert not np_(m.state)[1].any() and np.array_equal(np_(m.state)[0], sh[0, -160:])


@pytest.mark.gpu
def test_headline_stream_ignores_poisoned_lds(ss, sslib, sslab):
    import torch

    cfg = _cfg(ss)
    B = 1024
    s = _gsig(torch, (B, 4 * 160), 22)
    st0 = _gsig(torch, (B, 160), 23)
    a = _dev_call(torch, sslib, cfg, s, st0.clone(), 40)
    assert sslib.ss_last_kernel_name() == STREAM_KERNEL
    torch.cuda.synchronize()
    assert sslab.ss_debug_poison_lds(None) == 0
    b = _dev_call(torch, sslib, cfg, s, st0.clone(), 40)
    torch.cuda.synchronize()
    assert torch.isfinite(b).all() and torch.equal(a, b)
