"""Packed variable-length clips on the STFT path: ss_packed_row_offsets, ss_mel_spectrogram_packed / ss_stft_packed (host pointers),
their *_device forms and the Python front's mel_spectrogram_packed / mel_spectrogram_list / stft_packed.

Clip b is x[so[b] : so[b+1]]; its R_b = ceil(n_b / hop) rows are rows ro[b] .. ro[b+1] of the packed row space (mel: clip b's
[M x R_b] block starts at M * ro[b]).  Per clip, every result is what the equal-length entry points return for that clip alone.
The CPU tests cover the offsets and the argument rules; the GPU tests compare with per-clip calls and the oracle.
"""
import ctypes as C

import numpy as np
import pytest

from common import CONFIGS, RTOL, rel

PACKED_MEL_KERNEL = b"ss_mel_c1024v<w12,mel6321>"  # the packed build of the twelve-wave 2048-point mel kernel
CFG3 = CONFIGS["cfg3"]

ROW_CASES = {
    "cfg3": CFG3,
    "512_hop256": dict(fft_points=512, frame_length=0.016),
    "chirpz400_hop160": dict(fft_points=400, frame_length=0.01),
    "slaney": dict(fft_points=1024, frame_length=0.032, mel_scale="slaney", mel_norm="slaney"),
}


def _params(**kw):
    from speechsauce_amd import _lib

    return _lib.make_params(**kw)


def _so(lengths):
    so = np.zeros(len(lengths) + 1, dtype=np.int64)
    np.cumsum(np.asarray(lengths, dtype=np.int64), out=so[1:])
    return so


def _row_offsets(sslib, p, so):
    ro = np.full(so.size, -7, dtype=np.int64)
    rc = sslib.ss_packed_row_offsets(C.byref(p), so.size - 1, so.ctypes.data, ro.ctypes.data)
    return rc, ro


# ---------------------------------------------------------------- CPU ---------------------------------------------------------

@pytest.mark.parametrize("case", list(ROW_CASES))
def test_row_offsets_agree_with_the_oracle_per_clip(sslib, oracle, case):
    kw = ROW_CASES[case]
    p = _params(**kw)
    po = oracle.make_params(**kw)
    hop, n_pad, _ = oracle.stft_sizes(po)
    rng = np.random.default_rng(1)
    lengths = [1, 2, 3, hop - 1, hop, hop + 1, n_pad * hop, n_pad * hop + 1, (n_pad + 1) * hop - 1, 16001, 16000 * 16 + 7]
    lengths += rng.integers(1, 16000 * 16, 300).tolist()
    rc, ro = _row_offsets(sslib, p, _so(lengths))
    assert rc == 0
    assert ro[0] == 0 and ro.dtype == np.int64
    assert np.diff(ro).tolist() == [oracle.stft_rows(po, n)[0] for n in lengths]


def test_row_offsets_argument_errors(sslib):
    p = _params(**CFG3)
    # an empty table: ro = [0]
    rc, ro = _row_offsets(sslib, p, np.zeros(1, dtype=np.int64))
    assert rc == 0 and ro.tolist() == [0]
    # decreasing offsets / so[0] != 0: SS_ERR_ARG
    assert _row_offsets(sslib, p, np.array([0, 16000, 15000, 32000], dtype=np.int64))[0] == 3
    assert _row_offsets(sslib, p, np.array([5, 16005], dtype=np.int64))[0] == 3
    # a clip of zero samples: SS_ERR_ARG, and the message names it
    assert _row_offsets(sslib, p, _so([16000, 512, 0, 9]))[0] == 3
    assert b"clip 2" in sslib.ss_last_error_string()
    # a clip longer than 2^31 - 1 samples
    assert _row_offsets(sslib, p, np.array([0, 2 ** 31], dtype=np.int64))[0] == 3
    assert _row_offsets(sslib, p, np.array([0, 2 ** 31 - 1], dtype=np.int64))[0] == 0
    # null pointers
    ro = np.empty(2, dtype=np.int64)
    so = _so([100])
    assert sslib.ss_packed_row_offsets(C.byref(p), 1, None, ro.ctypes.data) == 3
    assert sslib.ss_packed_row_offsets(C.byref(p), 1, so.ctypes.data, None) == 3
    assert sslib.ss_packed_row_offsets(None, 1, so.ctypes.data, ro.ctypes.data) == 3
    # a config without an STFT path (fft_points < 2 * hop): SS_ERR_BAD_CONFIG
    bad = _params(fft_points=512, frame_length=0.025)  # hop 400
    assert sslib.ss_packed_row_offsets(C.byref(bad), 1, so.ctypes.data, ro.ctypes.data) == 2


def test_packed_calls_with_no_clips(sslib):
    # a null config is an argument error; the Python front's offsets need no device
    assert sslib.ss_mel_spectrogram_packed_device(None, None, 0, None, None, 0, None, None) == 3
    assert sslib.ss_stft_packed_device(None, None, 0, None, None, 0, None, None) == 3
    assert sslib.ss_mel_spectrogram_packed(None, None, 0, None, None) == 3
    import speechsauce_amd as ss

    cfg = ss.SpeechConfig.__new__(ss.SpeechConfig)  # (no handle: the offsets need only the parameters)
    cfg.params = _params(**CFG3)
    so = ss._sample_offsets([], 0, "t")
    assert ss._row_offsets(cfg, so).tolist() == [0]


def test_python_argument_rules(sslib):
    import speechsauce_amd as ss

    x = np.zeros(32000, dtype=np.float32)
    with pytest.raises(ValueError):
        ss.mel_spectrogram_packed(x, [16000, 16001], 16000)  # more samples than the buffer holds
    with pytest.raises(ValueError):
        ss.stft_packed(x, [16000, 16001], 16000)
    with pytest.raises(ValueError):
        ss.mel_spectrogram_packed(x.reshape(2, 16000), [16000, 16000], 16000)  # 2-D input
    with pytest.raises(ValueError):
        ss.stft_packed(x.reshape(2, 16000), [16000, 16000], 16000)
    with pytest.raises(TypeError):
        ss.mel_spectrogram_packed(x, [16000.0, 16000.0], 16000)  # non-integer lengths
    with pytest.raises(TypeError):
        ss.stft_packed(x, np.array([1.5, 2.5]), 16000)
    with pytest.raises(TypeError):
        ss.mel_spectrogram_packed(x.astype(np.float64), [16000, 16000], 16000)
    with pytest.raises(ValueError):
        ss.mel_spectrogram_packed(x, [16000, -1], 16000)
    assert ss.mel_spectrogram_list([], 16000) == []


# ---------------------------------------------------------------- GPU ---------------------------------------------------------

def _signal(torch, total, seed):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    return torch.randn(total, generator=g, device="cuda", dtype=torch.float32).mul_(0.05)


def _cfg3_lengths(rng, n):
    """n clips of 1 - 16 s at 16 kHz, with clips shorter than n_pad * hop (every row zero), odd lengths and edge lengths."""
    lens = rng.integers(16000, 16000 * 16 + 1, n)
    lens[:12] = [1, 511, 512, 513, 1023, 1024, 1025, 1536, 1537, 2047, 16001, 16000 * 16 - 1]
    lens[12:40] |= 1  # odd lengths: the clips behind them start at odd offsets
    rng.shuffle(lens)
    return lens.astype(np.int64)


def _per_clip_mel(torch, lib, cfg, x, so, ro, M):
    """The equal-length entry point, one clip (channels = 1) per call, into one packed block."""
    out = torch.full((M * int(ro[-1]),), float("nan"), device="cuda")
    for b in range(len(so) - 1):
        n = int(so[b + 1] - so[b])
        rc = lib.ss_mel_spectrogram_device(cfg.handle, x.data_ptr() + 4 * int(so[b]), 1, n, n, out[M * int(ro[b]):].data_ptr(), None)
        assert rc == 0, b
    return out


def _per_clip_stft(torch, lib, cfg, x, so, ro, F):
    out = torch.full((int(ro[-1]), F, 2), float("nan"), device="cuda")
    for b in range(len(so) - 1):
        n = int(so[b + 1] - so[b])
        rc = lib.ss_stft_device(cfg.handle, x.data_ptr() + 4 * int(so[b]), 1, n, n, out[int(ro[b]):].data_ptr(), None)
        assert rc == 0, b
    return out


def _clip(flat, ro, b, M):
    return flat[M * int(ro[b]):M * int(ro[b + 1])].reshape(M, int(ro[b + 1] - ro[b]))


@pytest.mark.gpu
def test_cfg3_matches_per_clip_calls_and_the_oracle(ss, sslib, sslab, oracle):
    import torch

    from speechsauce_amd import _lib

    rng = np.random.default_rng(21)
    lens = _cfg3_lengths(rng, 1024)
    x = _signal(torch, int(lens.sum()), 31)
    out, ro_d = ss.mel_spectrogram_packed(x, lens, 16000, **_front_kw(CFG3))
    torch.cuda.synchronize()
    assert sslib.ss_last_kernel_name() == PACKED_MEL_KERNEL
    M = CFG3["num_filters"]
    ro = ro_d.cpu().numpy()
    so = np.concatenate([[0], np.cumsum(lens)])
    assert out.shape == (M * int(ro[-1]),) and ro_d.device == x.device
    got = out.cpu().numpy()
    assert not np.isnan(got).any()
    # bit for bit the equal-length entry point clip by clip, on its twelve-wave build (forced in the lab library)
    with _lib.use_library(sslab):
        sslab.ss_debug_mel_tile(3)
        try:
            cfg = ss.SpeechConfig(_lib.make_params(**CFG3))
            want = _per_clip_mel(torch, sslab, cfg, x, so, ro, M)
            torch.cuda.synchronize()
            assert sslab.ss_last_kernel_name() == b"ss_mel_c1024<w12,mel6321>"
        finally:
            sslab.ss_debug_mel_tile(0)
    assert np.array_equal(got, want.cpu().numpy())
    p = oracle.make_params(**CFG3)
    _, n_pad, _ = oracle.stft_sizes(p)
    xh = x.cpu().numpy()
    for b in range(len(lens)):
        g = _clip(got, ro, b, M)
        assert np.all(g[:, g.shape[1] - min(n_pad, g.shape[1]):] == 0.0), b  # the last n_pad rows: exact zeros
        if b % 32 == 0 or lens[b] < 2048:
            assert rel(g, oracle.mel_spectrogram(p, xh[so[b]:so[b + 1]])) <= RTOL, b
    # the same block from the generic kernel's packed build (lab library, generic forced): same row counts, within RTOL
    with _lib.use_library(sslab):
        sslab.ss_debug_force_generic(1)
        try:
            gen, gro = ss.mel_spectrogram_packed(x, lens, 16000, **_front_kw(CFG3))
            torch.cuda.synchronize()
            assert sslab.ss_last_kernel_name() == b"ss_front_generic_varrows<10>"
        finally:
            sslab.ss_debug_force_generic(0)
    assert np.array_equal(gro.cpu().numpy(), ro)
    gen = gen.cpu().numpy()
    for b in range(0, len(lens), 5):
        w = _clip(got, ro, b, M)
        if np.abs(w).max() > 0:
            assert rel(_clip(gen, ro, b, M), w) <= RTOL, b


def _front_kw(kw):
    """make_params keywords -> the Python front's (sampling_frequency is positional)."""
    m = dict(frame_length=kw.get("frame_length", 0.02), frame_stride=kw.get("frame_stride", 0.01),
             num_filters=kw.get("num_filters", 40), fft_length=kw.get("fft_points", 512))
    if "high_frequency" in kw:
        m["high_frequency"] = kw["high_frequency"]
    for k in ("mel_scale", "mel_norm"):
        if k in kw:
            m[k] = kw[k]
    return m


GENERIC_CASES = {
    "512_hop256": dict(fft_points=512, frame_length=0.016),
    "1024": dict(fft_points=1024, frame_length=0.032, num_filters=64),
    "4096": dict(sample_rate=44100, fft_points=4096, frame_length=0.02, num_filters=256, high_frequency=22050.0),
    "chirpz400": dict(fft_points=400, frame_length=0.01),
    "chirpz1000": dict(fft_points=1000, frame_length=0.02),
    "slaney_norm": dict(fft_points=1024, frame_length=0.032, mel_scale="slaney", mel_norm="slaney"),
    "htk": dict(fft_points=512, frame_length=0.016, mel_scale="htk"),
}


def _generic_setup(torch, ss, kw, seed):
    from speechsauce_amd import _lib

    sr = kw.get("sample_rate", 16000)
    pkw = {k: v for k, v in kw.items() if k != "sample_rate"}
    rng = np.random.default_rng(seed)
    lens = rng.integers(1, sr * 3, 40).astype(np.int64)
    lens[:6] = [1, 17, 333, 1000, 4097, 8191]
    x = _signal(torch, int(lens.sum()), seed)
    cfg = ss.SpeechConfig(_lib.make_params(sample_rate=sr, **pkw))
    so = ss._sample_offsets(lens, x.shape[0], "t")
    ro = ss._row_offsets(cfg, so)
    return sr, pkw, lens, x, cfg, so, ro


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(GENERIC_CASES))
def test_generic_mel_matches_the_equal_length_path_and_the_oracle(ss, sslib, sslab, oracle, case):
    import torch

    from speechsauce_amd import _lib

    sr, pkw, lens, x, cfg, so, ro = _generic_setup(torch, ss, GENERIC_CASES[case], 41)
    M = cfg.params.num_filters
    dso, dro = torch.from_numpy(so).cuda(), torch.from_numpy(ro).cuda()
    out = torch.full((M * int(ro[-1]),), float("nan"), device="cuda")
    assert sslib.ss_mel_spectrogram_packed_device(cfg.handle, x.data_ptr(), len(lens), dso.data_ptr(), dro.data_ptr(), int(ro[-1]),
                                                  out.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert sslib.ss_last_kernel_name().startswith(b"ss_front_generic_varrows<")
    cfg.device_status()
    got = out.cpu().numpy()
    with _lib.use_library(sslab):
        sslab.ss_debug_force_generic(1)
        try:
            lcfg = ss.SpeechConfig(_lib.make_params(sample_rate=sr, **pkw))
            want = _per_clip_mel(torch, sslab, lcfg, x, so, ro, M)
            torch.cuda.synchronize()
        finally:
            sslab.ss_debug_force_generic(0)
    assert np.array_equal(got, want.cpu().numpy())
    p = oracle.make_params(sample_rate=sr, **pkw)
    xh = x.cpu().numpy()
    for b in range(len(lens)):
        assert rel(_clip(got, ro, b, M), oracle.mel_spectrogram(p, xh[so[b]:so[b + 1]])) <= RTOL, b


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["cfg3", "512_hop256", "chirpz400"])
def test_stft_packed_matches_the_equal_length_path_and_the_oracle(ss, sslib, sslab, oracle, case):
    import torch

    from speechsauce_amd import _lib

    kw = CFG3 if case == "cfg3" else GENERIC_CASES[case]
    sr, pkw, lens, x, cfg, so, ro = _generic_setup(torch, ss, kw, 42)
    F = cfg.params.fft_points // 2 + 1
    z, ro_d = ss.stft_packed(x, lens, sr, frame_length=pkw["frame_length"], fft_length=pkw["fft_points"])
    torch.cuda.synchronize()
    assert sslib.ss_last_kernel_name().startswith(b"ss_front_generic_varrows<")
    assert z.dtype == torch.complex64 and z.shape == (int(ro[-1]), F)
    assert np.array_equal(ro_d.cpu().numpy(), ro)
    got = torch.view_as_real(z).cpu().numpy()
    with _lib.use_library(sslab):
        sslab.ss_debug_force_generic(1)
        try:
            lcfg = ss.SpeechConfig(_lib.make_params(sample_rate=sr, **pkw))
            want = _per_clip_stft(torch, sslab, lcfg, x, so, ro, F)
            torch.cuda.synchronize()
        finally:
            sslab.ss_debug_force_generic(0)
    assert np.array_equal(got, want.cpu().numpy())
    p = oracle.make_params(sample_rate=sr, **pkw)
    _, n_pad, _ = oracle.stft_sizes(p)
    xh = x.cpu().numpy()
    zc = got[..., 0] + 1j * got[..., 1]
    for b in range(len(lens)):
        g = zc[ro[b]:ro[b + 1]]
        assert np.all(g[len(g) - min(n_pad, len(g)):] == 0), b
        w = oracle.stft(p, xh[so[b]:so[b + 1]])[0]
        assert np.abs(g - w).max() <= RTOL * max(np.abs(w).max(), 1e-30), b


@pytest.mark.gpu
@pytest.mark.parametrize("kw", [CFG3, dict(fft_points=400, frame_length=0.01)], ids=["headline", "generic"])
def test_sample_offsets_past_two_to_the_31(ss, sslib, kw):
    import torch

    from speechsauce_amd import _lib

    lens = np.array([16000, 12345, 1, 48000, 801], dtype=np.int64)
    n = int(lens.sum())
    big = 2 ** 31 + 2 ** 22  # floats (8.6e9 bytes): the clips at the end start past sample 2^31, byte 2^33
    x = torch.zeros(big, dtype=torch.float32, device="cuda")
    src = _signal(torch, n, 7)
    x[big - n:] = src
    cfg = ss.SpeechConfig(_lib.make_params(**kw))
    so = ss._sample_offsets(lens, n, "t")
    ro = ss._row_offsets(cfg, so)
    M = cfg.params.num_filters
    outs = []
    for base in (0, big - n):
        if base == 0:
            x[:n] = src
        dso = torch.from_numpy(so + base).cuda()  # (device offsets are absolute: the clips sit at the buffer's end)
        dro = torch.from_numpy(ro).cuda()
        out = torch.full((M * int(ro[-1]),), float("nan"), device="cuda")
        assert sslib.ss_mel_spectrogram_packed_device(cfg.handle, x.data_ptr(), len(lens), dso.data_ptr(), dro.data_ptr(),
                                                      int(ro[-1]), out.data_ptr(), None) == 0
        torch.cuda.synchronize()
        assert (sslib.ss_last_kernel_name() == PACKED_MEL_KERNEL) == (kw is CFG3)
        cfg.device_status()
        outs.append(out.cpu().numpy())
    assert big - n > 2 ** 31
    assert np.array_equal(outs[0], outs[1]) and not np.isnan(outs[0]).any()
    del x


@pytest.mark.gpu
@pytest.mark.parametrize("kw", [CFG3, dict(fft_points=512, frame_length=0.016)], ids=["headline", "generic"])
def test_bad_device_offsets_raise_the_error_word_and_write_nothing_outside(ss, sslib, kw):
    import torch

    from speechsauce_amd import _lib

    lens = np.array([16000, 8000, 4000, 12000], dtype=np.int64)
    x = _signal(torch, int(lens.sum()), 8)
    cfg = ss.SpeechConfig(_lib.make_params(**kw))  # a fresh config: its error word is its own
    M = cfg.params.num_filters
    so = ss._sample_offsets(lens, x.shape[0], "t")
    ro = ss._row_offsets(cfg, so)
    rows = int(ro[-1])
    dso, dro = torch.from_numpy(so).cuda(), torch.from_numpy(ro).cuda()
    good = torch.full((M * rows,), float("nan"), device="cuda")
    assert sslib.ss_mel_spectrogram_packed_device(cfg.handle, x.data_ptr(), 4, dso.data_ptr(), dro.data_ptr(), rows,
                                                  good.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert sslib.ss_config_device_status(cfg.handle) == 0
    good = good.cpu().numpy()
    SENT = 12345.0
    pad = 4096

    def run(ro_bad, total):
        block = torch.full((M * total + 2 * pad,), SENT, device="cuda")
        d = torch.from_numpy(np.asarray(ro_bad, dtype=np.int64)).cuda()
        rc = sslib.ss_mel_spectrogram_packed_device(cfg.handle, x.data_ptr(), 4, dso.data_ptr(), d.data_ptr(), total,
                                                    block[pad:].data_ptr(), None)
        assert rc == 0  # the check is the kernel's: asynchronous
        torch.cuda.synchronize()
        return block.cpu().numpy()

    # clip 1 claims one row too many; the clips behind it start one row late but are consistent in themselves
    bad = ro.copy()
    bad[2:] += 1
    blk = run(bad, int(bad[-1]))
    assert sslib.ss_config_device_status(cfg.handle) == 6  # SS_ERR_DEVICE, read and cleared
    assert sslib.ss_config_device_status(cfg.handle) == 0
    assert np.all(blk[:pad] == SENT) and np.all(blk[-pad:] == SENT)
    body = blk[pad:-pad]
    assert np.array_equal(body[:M * ro[1]], good[:M * ro[1]])               # clip 0
    assert np.all(body[M * bad[1]:M * bad[2]] == SENT)                     # clip 1 skipped
    for b in (2, 3):                                                       # clips 2, 3: one row later
        assert np.array_equal(body[M * bad[b]:M * bad[b + 1]], good[M * ro[b]:M * ro[b + 1]]), b
    # total_rows smaller than the clips' rows: the last clip is skipped; the next call on the config reports the error
    nxt = torch.empty((M * rows,), device="cuda")
    blk = run(ro, rows - 10)
    rc = sslib.ss_mel_spectrogram_packed_device(cfg.handle, x.data_ptr(), 4, dso.data_ptr(), dro.data_ptr(), rows, nxt.data_ptr(), None)
    assert rc == 6  # SS_ERR_DEVICE from the next call, which launches nothing
    assert sslib.ss_config_device_status(cfg.handle) == 0
    assert np.all(blk[:pad] == SENT) and np.all(blk[-pad:] == SENT)
    body = blk[pad:-pad]
    assert np.array_equal(body[:M * ro[3]], good[:M * ro[3]])
    assert np.all(body[M * ro[3]:] == SENT)
    # the stft form: a bad table raises the word too, nothing outside the block
    F2 = 2 * (cfg.params.fft_points // 2 + 1)
    sblk = torch.full((F2 * int(bad[-1]) + 2 * pad,), SENT, device="cuda")
    d = torch.from_numpy(bad).cuda()
    assert sslib.ss_stft_packed_device(cfg.handle, x.data_ptr(), 4, dso.data_ptr(), d.data_ptr(), int(bad[-1]),
                                       sblk[pad:].data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert sslib.ss_config_device_status(cfg.handle) == 6
    sb = sblk.cpu().numpy()
    assert np.all(sb[:pad] == SENT) and np.all(sb[-pad:] == SENT)
    assert np.all(sb[pad:-pad][F2 * bad[1]:F2 * bad[2]] == SENT)


@pytest.mark.gpu
@pytest.mark.parametrize("stft", [False, True], ids=["mel", "stft"])
def test_graph_capture_replays_on_new_input(ss, sslib, stft):
    import torch

    from speechsauce_amd import _lib

    lens = np.array([16000, 7777, 640, 32001, 20000, 1], dtype=np.int64)
    n = int(lens.sum())
    cfg = ss.SpeechConfig(_lib.make_params(**CFG3))
    so = ss._sample_offsets(lens, n, "t")
    ro = ss._row_offsets(cfg, so)
    dso, dro = torch.from_numpy(so).cuda(), torch.from_numpy(ro).cuda()
    rows = int(ro[-1])
    cols = 2 * (cfg.params.fft_points // 2 + 1) if stft else cfg.params.num_filters
    fn = sslib.ss_stft_packed_device if stft else sslib.ss_mel_spectrogram_packed_device
    x = _signal(torch, n, 9)
    out = torch.empty((rows * cols,), device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):  # warm-up off the capture
        assert fn(cfg.handle, x.data_ptr(), len(lens), dso.data_ptr(), dro.data_ptr(), rows, out.data_ptr(), C.c_void_p(s.cuda_stream)) == 0
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        rc = fn(cfg.handle, x.data_ptr(), len(lens), dso.data_ptr(), dro.data_ptr(), rows, out.data_ptr(),
                C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    for seed in (21, 22):
        x.copy_(_signal(torch, n, seed))
        g.replay()
        torch.cuda.synchronize()
        eager = torch.empty_like(out)
        assert fn(cfg.handle, x.data_ptr(), len(lens), dso.data_ptr(), dro.data_ptr(), rows, eager.data_ptr(), None) == 0
        torch.cuda.synchronize()
        assert torch.equal(out, eager)
    cfg.device_status()


@pytest.mark.gpu
def test_host_path_and_list_form_match_the_device_path(ss, sslib):
    import torch

    rng = np.random.default_rng(15)
    lens = _cfg3_lengths(rng, 64)
    x = _signal(torch, int(lens.sum()), 10)
    kw = _front_kw(CFG3)
    dev, ro_d = ss.mel_spectrogram_packed(x, lens.tolist(), 16000, **kw)
    host, ro_h = ss.mel_spectrogram_packed(x.cpu().numpy(), lens, 16000, **kw)
    torch.cuda.synchronize()
    assert isinstance(host, np.ndarray) and np.array_equal(ro_h, ro_d.cpu().numpy())
    assert np.array_equal(host, dev.cpu().numpy())
    zd, _ = ss.stft_packed(x, lens, 16000, frame_length=0.032, fft_length=2048)
    zh, _ = ss.stft_packed(x.cpu().numpy(), lens, 16000, frame_length=0.032, fft_length=2048)
    assert zh.dtype == np.complex64 and np.array_equal(zh, zd.cpu().numpy())
    so = np.concatenate([[0], np.cumsum(lens)])
    clips = [x[int(so[b]):int(so[b + 1])] for b in range(len(lens))]
    lst = ss.mel_spectrogram_list(clips, 16000, **kw)
    M = CFG3["num_filters"]
    assert len(lst) == len(lens)
    for b, f in enumerate(lst):
        assert f.shape == (M, int(ro_h[b + 1] - ro_h[b]))
        assert torch.equal(f, _clip(dev, ro_h, b, M)), b
    lst_h = ss.mel_spectrogram_list([c.cpu().numpy() for c in clips], 16000, **kw)
    assert all(np.array_equal(a, b.cpu().numpy()) for a, b in zip(lst_h, lst))
    with pytest.raises(ValueError):
        ss.mel_spectrogram_list([clips[0], clips[1].cpu().numpy()], 16000, **kw)  # device and host clips in one call
    with pytest.raises(ss.SpeechSauceError) as e:
        ss.mel_spectrogram_packed(x[:16000], [16000, 0], 16000, **kw)  # the second clip is empty
    assert e.value.status == 3 and "clip 1" in e.value.detail


@pytest.mark.gpu
def test_headline_packed_ignores_poisoned_lds(ss, sslib, sslab):
    import torch

    rng = np.random.default_rng(16)
    lens = _cfg3_lengths(rng, 256)
    x = _signal(torch, int(lens.sum()), 11)
    kw = _front_kw(CFG3)
    a, _ = ss.mel_spectrogram_packed(x, lens, 16000, **kw)
    assert sslib.ss_last_kernel_name() == PACKED_MEL_KERNEL
    torch.cuda.synchronize()
    assert sslab.ss_debug_poison_lds(None) == 0
    b, _ = ss.mel_spectrogram_packed(x, lens, 16000, **kw)
    torch.cuda.synchronize()
    assert torch.isfinite(b).all() and torch.equal(a, b)
