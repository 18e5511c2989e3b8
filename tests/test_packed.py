"""Packed variable-length clips: ss_packed_frame_offsets, ss_mfcc_packed / ss_mfe_packed (host pointers), their *_device forms
and the Python front's mfcc_packed / mfe_packed / mfcc_list.

Clip b is x[so[b] : so[b+1]]; its features are rows fo[b] .. fo[b+1] of one block.  Per clip, every result is what the
equal-length entry points return for that clip alone (own frame count, own DCT scaling, own pre-emphasis wrap, own literal-framing
rule).  The CPU tests cover the offsets and the argument rules; the GPU tests compare with per-clip calls and the oracle.
"""
import ctypes as C

import numpy as np
import pytest

from common import BENCH_KERNELS, RTOL, rel

PACKED_KERNEL = b"ss_mfcc_c256v<10,exact,bank421,sym>"  # the varlen build of the headline kernel

EPS = np.float32(1.1920929e-7)


def _params(sslib, **kw):
    from speechsauce_amd import _lib

    return _lib.make_params(**kw)


def _offsets(sslib, p, lengths):
    so = np.zeros(len(lengths) + 1, dtype=np.int64)
    np.cumsum(np.asarray(lengths, dtype=np.int64), out=so[1:])
    fo = np.full(len(lengths) + 1, -7, dtype=np.int64)
    rc = sslib.ss_packed_frame_offsets(C.byref(p), len(lengths), so.ctypes.data, fo.ctypes.data)
    return rc, so, fo


# ---------------------------------------------------------------- CPU ---------------------------------------------------------

@pytest.mark.parametrize("framing", ["contract", "padded", "center", "literal"])
def test_frame_offsets_agree_with_the_oracle_per_clip(sslib, oracle, framing):
    rng = np.random.default_rng(5)
    lengths = [480, 481, 639, 640, 799, 800, 16000, 16001] + rng.integers(480, 48000, 200).tolist()
    p = _params(sslib, framing=framing)
    rc, so, fo = _offsets(sslib, p, lengths)
    assert rc == 0
    po = oracle.make_params(framing=framing)
    want = [oracle.num_frames(po, n) for n in lengths]
    assert fo[0] == 0
    assert np.diff(fo).tolist() == want
    assert fo.dtype == np.int64


def test_frame_offsets_argument_errors(sslib):
    p = _params(sslib)
    # a clip too short for one frame: status 1, and the error names its index
    rc, _, _ = _offsets(sslib, p, [16000, 16000, 100, 16000])
    assert rc == 1
    assert b"clip 2" in sslib.ss_last_error_string()
    # decreasing offsets / so[0] != 0: status 3
    so = np.array([0, 16000, 15000, 32000], dtype=np.int64)
    fo = np.empty(4, dtype=np.int64)
    assert sslib.ss_packed_frame_offsets(C.byref(p), 3, so.ctypes.data, fo.ctypes.data) == 3
    so = np.array([5, 16005], dtype=np.int64)
    assert sslib.ss_packed_frame_offsets(C.byref(p), 1, so.ctypes.data, fo.ctypes.data) == 3
    # no clips: OK, fo = [0]
    so = np.zeros(1, dtype=np.int64)
    fo = np.full(1, -1, dtype=np.int64)
    assert sslib.ss_packed_frame_offsets(C.byref(p), 0, so.ctypes.data, fo.ctypes.data) == 0
    assert fo[0] == 0
    # null arguments
    assert sslib.ss_packed_frame_offsets(C.byref(p), 0, None, fo.ctypes.data) == 3


def test_packed_calls_with_no_clips(sslib):
    assert sslib.ss_mfcc_packed_device(None, None, 0, None, None, 0, None, None) == 3  # a null config is an argument error
    # the Python front's offsets: empty lengths give fo = [0] without touching a device
    import speechsauce_amd as ss

    cfg = ss.SpeechConfig.__new__(ss.SpeechConfig)  # (no handle: the offsets need only the parameters)
    cfg.params = _params(sslib)
    so, fo = ss._packed_offsets(cfg, [], 0, "t")
    assert so.tolist() == [0] and fo.tolist() == [0]


def test_python_argument_rules(sslib):
    import speechsauce_amd as ss

    x = np.zeros(32000, dtype=np.float32)
    with pytest.raises(TypeError):
        ss.mfcc_packed(x.astype(np.float64), [16000, 16000], 16000)
    with pytest.raises(ValueError):
        ss.mfcc_packed(x.reshape(2, 16000), [16000, 16000], 16000)
    with pytest.raises(ValueError):
        ss.mfcc_packed(x, [16000, 16001], 16000)  # more samples than the buffer holds
    with pytest.raises(ValueError):
        ss.mfcc_packed(x, [[16000, 16000]], 16000)
    with pytest.raises(TypeError):
        ss.mfcc_packed(x, [16000.0, 16000.0], 16000)
    with pytest.raises(ValueError):
        ss.mfe_packed(x, np.array([16000, -1]), 16000)


# ---------------------------------------------------------------- GPU ---------------------------------------------------------

def _lengths(rng, n):
    lens = rng.integers(480, 48001, n)
    lens[:12] = [480, 481, 639, 640, 641, 799, 800, 801, 959, 960, 963, 48000]  # 1-3-frame clips, odd and even
    rng.shuffle(lens)
    return lens.astype(np.int64)


def _signal(torch, total, seed):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    return torch.randn(total, generator=g, device="cuda", dtype=torch.float32).mul_(0.05)


def _per_clip(torch, sslib, cfg, x, so, fo, cols, mfe=False):
    """The equal-length entry point, one clip (batch = 1) per call, into one packed block"""
    out = torch.full((int(fo[-1]), cols), float("nan"), device="cuda")
    en = torch.full((int(fo[-1]),), float("nan"), device="cuda") if mfe else None
    for b in range(len(so) - 1):
        n = int(so[b + 1] - so[b])
        xp = x.data_ptr() + 4 * int(so[b])
        if mfe:
            rc = sslib.ss_mfe_batch_device(cfg.handle, xp, 1, n, n, out[int(fo[b]):].data_ptr(), en[int(fo[b]):].data_ptr(), None)
        else:
            rc = sslib.ss_mfcc_batch_device(cfg.handle, xp, 1, n, n, out[int(fo[b]):].data_ptr(), None)
        assert rc == 0, b
    return out, en


@pytest.mark.gpu
def test_headline_shape_matches_per_clip_calls_and_the_oracle(ss, sslib, sslab, oracle):
    import torch

    from speechsauce_amd import _lib

    rng = np.random.default_rng(11)
    lens = _lengths(rng, 1024)
    x = _signal(torch, int(lens.sum()), 3)
    feat, fo_d = ss.mfcc_packed(x, lens, 16000)
    torch.cuda.synchronize()
    assert sslib.ss_last_kernel_name() == PACKED_KERNEL
    fo = fo_d.cpu().numpy()
    so = np.concatenate([[0], np.cumsum(lens)])
    assert feat.shape == (int(fo[-1]), 13) and fo_d.device == x.device
    got = feat.cpu().numpy()
    xh = x.cpu().numpy()
    # bit for bit what the equal-length entry point (the dedicated kernel) computes clip by clip
    cfg = ss.SpeechConfig(_lib.make_params())
    want, _ = _per_clip(torch, sslib, cfg, x, so, fo, 13)
    torch.cuda.synchronize()
    assert sslib.ss_last_kernel_name() == BENCH_KERNELS["cfg2"]
    assert np.array_equal(got, want.cpu().numpy())
    p = oracle.make_params()
    for b in range(len(lens)):
        if b % 16 == 0 or lens[b] < 1000:
            assert rel(got[fo[b]:fo[b + 1]], oracle.mfcc(p, xh[so[b]:so[b + 1]])) <= RTOL, b
    # the same block from the generic kernel's varlen build (lab library, generic forced): within RTOL, the same frame count
    with _lib.use_library(sslab):
        sslab.ss_debug_force_generic(1)
        try:
            gen, _ = ss.mfcc_packed(x, lens, 16000)
            torch.cuda.synchronize()
            assert sslab.ss_last_kernel_name() == b"ss_front_generic_varlen<8>"
        finally:
            sslab.ss_debug_force_generic(0)
    gen = gen.cpu().numpy()
    for b in range(0, len(lens), 7):
        assert rel(gen[fo[b]:fo[b + 1]], got[fo[b]:fo[b + 1]]) <= RTOL, b


@pytest.mark.gpu
def test_mfe_packed_matches_per_clip_calls_and_the_oracle(ss, sslib, sslab, oracle):
    import torch

    from speechsauce_amd import _lib

    rng = np.random.default_rng(12)
    lens = _lengths(rng, 256)
    x = _signal(torch, int(lens.sum()), 4)
    so = np.concatenate([[0], np.cumsum(lens)])
    z = 5  # an all-zero clip: every feature and energy is EPS exactly (feature.rs:216-230)
    x[int(so[z]):int(so[z + 1])] = 0.0
    feat, en, fo_d = ss.mfe_packed(x, torch.from_numpy(lens).cuda(), 16000)
    torch.cuda.synchronize()
    fo = fo_d.cpu().numpy()
    f, e = feat.cpu().numpy(), en.cpu().numpy()
    assert np.all(f[fo[z]:fo[z + 1]] == EPS) and np.all(e[fo[z]:fo[z + 1]] == EPS)
    with _lib.use_library(sslab):
        sslab.ss_debug_force_generic(1)
        try:
            cfg = ss.SpeechConfig(_lib.make_params(num_cepstral=13))
            wf, we = _per_clip(torch, sslab, cfg, x, so, fo, 40, mfe=True)
            torch.cuda.synchronize()
        finally:
            sslab.ss_debug_force_generic(0)
    assert np.array_equal(f, wf.cpu().numpy()) and np.array_equal(e, we.cpu().numpy())
    xh = x.cpu().numpy()
    p = oracle.make_params()
    for b in range(0, len(lens), 8):
        rows = slice(int(fo[b]), int(fo[b + 1]))
        of, oe = oracle.mfe(p, xh[so[b]:so[b + 1]])
        assert rel(f[rows], of) <= RTOL and rel(e[rows], oe) <= RTOL, b


GENERIC_CASES = {
    "cfg5": dict(sample_rate=44100, fft_points=4096, frame_length=4096 / 44100, frame_stride=1024 / 44100, num_cepstral=40,
                 num_filters=256, high_frequency=22050.0),
    "fft400": dict(fft_points=400),
    "hann_preemph": dict(mfcc_window="hann", preemph_coef=0.97),
    "center": dict(framing="center"),
    "padded": dict(framing="padded"),
    "ortho_exp2": dict(dct_norm="ortho", spectrum_exponent=2),
}
# The one named exception to RTOL: the generic kernel itself (its equal-length path, whose bits the packed block reproduces -- asserted
# above) comes to 1.85e-4 of the oracle on one clip of this signal with a Hann window and pre-emphasis 0.97 (white noise, emphasised:
# the high cepstra are small beside the column maximum).  The dedicated kernels do not serve packed clips of this configuration.
GENERIC_TOL = {"hann_preemph": 3e-4}


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(GENERIC_CASES))
def test_generic_configurations_match_the_oracle_per_clip(ss, sslib, sslab, oracle, case):
    import torch

    kw = GENERIC_CASES[case]
    from speechsauce_amd import _lib

    sr = kw.get("sample_rate", 16000)
    rng = np.random.default_rng(13)
    lens = rng.integers(sr // 8, sr * 2, 24).astype(np.int64)
    lens[0] += 1 - lens[0] % 2  # odd
    x = _signal(torch, int(lens.sum()), 5)
    pkw = {k: v for k, v in kw.items() if k != "sample_rate"}
    cfg = ss.SpeechConfig(_lib.make_params(sample_rate=sr, **pkw))
    so, fo = ss._packed_offsets(cfg, lens, x.shape[0], "t")
    dso, dfo = torch.from_numpy(so).cuda(), torch.from_numpy(fo).cuda()
    Cc = cfg.params.num_cepstral
    out = torch.full((int(fo[-1]), Cc), float("nan"), device="cuda")
    assert sslib.ss_mfcc_packed_device(cfg.handle, x.data_ptr(), len(lens), dso.data_ptr(), dfo.data_ptr(), int(fo[-1]),
                                       out.data_ptr(), None) == 0
    torch.cuda.synchronize()
    cfg.device_status()
    got, xh = out.cpu().numpy(), x.cpu().numpy()
    # bit for bit the equal-length entry point clip by clip on the same (generic) kernel
    with _lib.use_library(sslab):
        sslab.ss_debug_force_generic(1)
        try:
            lcfg = ss.SpeechConfig(_lib.make_params(sample_rate=sr, **pkw))
            want, _ = _per_clip(torch, sslab, lcfg, x, so, fo, Cc)
            torch.cuda.synchronize()
        finally:
            sslab.ss_debug_force_generic(0)
    want = want.cpu().numpy()
    assert np.array_equal(got, want)
    p = oracle.make_params(sample_rate=sr, **pkw)
    tol = GENERIC_TOL.get(case, RTOL)
    for b in range(len(lens)):
        assert rel(got[fo[b]:fo[b + 1]], oracle.mfcc(p, xh[so[b]:so[b + 1]])) <= tol, b


@pytest.mark.gpu
def test_literal_framing_known_answer(ss, sslib, oracle):
    """processing.rs:110-120 as written, per clip: > 2 frames copy nothing (every row the same constant), <= 2 frames copy
    x[0..flen] into every row."""
    import torch

    lens = np.array([16000, 640, 800, 480, 9001], dtype=np.int64)  # T = 98, 2, 3, 1, 54
    x = _signal(torch, int(lens.sum()), 6)
    feat, fo_d = ss.mfcc_packed(x, lens, 16000, framing="literal")
    torch.cuda.synchronize()
    fo, got, xh = fo_d.cpu().numpy(), feat.cpu().numpy(), x.cpu().numpy()
    so = np.concatenate([[0], np.cumsum(lens)])
    p = oracle.make_params(framing="literal")
    for b in range(len(lens)):
        rows = got[fo[b]:fo[b + 1]]
        assert rel(rows, oracle.mfcc(p, xh[so[b]:so[b + 1]])) <= RTOL, b
        if fo[b + 1] - fo[b] > 2:
            assert np.all(rows[1:] == rows[1]), b  # zero frames: identical rows after the first ([0,0] has its own scale)


@pytest.mark.gpu
@pytest.mark.parametrize("kw", [{}, dict(fft_points=400)], ids=["headline", "generic"])
def test_sample_offsets_past_two_to_the_31(ss, sslib, kw):
    import torch

    from speechsauce_amd import _lib

    lens = np.array([16000, 12345, 640, 48000, 801], dtype=np.int64)
    n = int(lens.sum())
    big = 2 ** 31 + 2 ** 22  # floats (8.6e9 bytes): the clips at the end start past sample 2^31, byte 2^33
    x = torch.zeros(big, dtype=torch.float32, device="cuda")
    src = _signal(torch, n, 7)
    x[big - n:] = src
    cfg = ss.SpeechConfig(_lib.make_params(**kw))
    so, fo = ss._packed_offsets(cfg, lens, n, "t")
    outs = []
    for base in (0, big - n):
        if base == 0:
            x[:n] = src
        dso = torch.from_numpy(so + base).cuda()  # (device offsets are absolute: the clips sit at the buffer's end)
        dfo = torch.from_numpy(fo).cuda()
        out = torch.full((int(fo[-1]), 13), float("nan"), device="cuda")
        assert sslib.ss_mfcc_packed_device(cfg.handle, x.data_ptr(), len(lens), dso.data_ptr(), dfo.data_ptr(), int(fo[-1]),
                                           out.data_ptr(), None) == 0
        torch.cuda.synchronize()
        assert (sslib.ss_last_kernel_name() == PACKED_KERNEL) == (not kw)
        cfg.device_status()
        outs.append(out.cpu().numpy())
    assert big - n > 2 ** 31
    assert np.array_equal(outs[0], outs[1]) and not np.isnan(outs[0]).any()
    del x


@pytest.mark.gpu
def test_bad_device_offsets_raise_the_error_word_and_write_nothing_outside(ss, sslib):
    import torch

    from speechsauce_amd import _lib

    lens = np.array([16000, 8000, 4000, 12000], dtype=np.int64)
    x = _signal(torch, int(lens.sum()), 8)
    cfg = ss.SpeechConfig(_lib.make_params())  # a fresh config: its error word is its own
    so, fo = ss._packed_offsets(cfg, lens, x.shape[0], "t")
    rows = int(fo[-1])
    good = torch.full((rows, 13), float("nan"), device="cuda")
    dso, dfo = torch.from_numpy(so).cuda(), torch.from_numpy(fo).cuda()
    assert sslib.ss_mfcc_packed_device(cfg.handle, x.data_ptr(), 4, dso.data_ptr(), dfo.data_ptr(), rows, good.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert sslib.ss_config_device_status(cfg.handle) == 0
    good = good.cpu().numpy()
    SENT = 12345.0
    pad = 64

    def run(fo_bad, total):
        block = torch.full(((total + 2 * pad) * 13,), SENT, device="cuda")
        d = torch.from_numpy(np.asarray(fo_bad, dtype=np.int64)).cuda()
        rc = sslib.ss_mfcc_packed_device(cfg.handle, x.data_ptr(), 4, dso.data_ptr(), d.data_ptr(), total,
                                         block[pad * 13:].data_ptr(), None)
        assert rc == 0  # the check is the kernel's: asynchronous
        torch.cuda.synchronize()
        return block.cpu().numpy()

    # clip 1 claims one row too many; the clips behind it start one row late but are consistent in themselves
    bad = fo.copy()
    bad[2:] += 1
    blk = run(bad, int(bad[-1]))
    assert sslib.ss_config_device_status(cfg.handle) == 6  # SS_ERR_DEVICE, read and cleared
    assert sslib.ss_config_device_status(cfg.handle) == 0
    assert np.all(blk[:pad * 13] == SENT) and np.all(blk[-pad * 13:] == SENT)
    body = blk[pad * 13:-pad * 13].reshape(-1, 13)
    assert np.array_equal(body[:fo[1]], good[:fo[1]])                       # clip 0
    assert np.all(body[bad[1]:bad[2]] == SENT)                              # clip 1 skipped
    for b in (2, 3):                                                        # clips 2, 3: one row later
        assert np.array_equal(body[bad[b]:bad[b + 1]], good[fo[b]:fo[b + 1]]), b
    # total_frames smaller than the clips' rows: the last clip is skipped; the next call on the config reports the error
    nxt = torch.empty((rows, 13), device="cuda")
    blk = run(fo, rows - 10)
    rc = sslib.ss_mfcc_packed_device(cfg.handle, x.data_ptr(), 4, dso.data_ptr(), dfo.data_ptr(), rows, nxt.data_ptr(), None)
    assert rc == 6  # SS_ERR_DEVICE from the next call, which launches nothing
    assert sslib.ss_config_device_status(cfg.handle) == 0  # (cleared by the call that reported it)
    assert np.all(blk[:pad * 13] == SENT) and np.all(blk[-pad * 13:] == SENT)
    body = blk[pad * 13:-pad * 13].reshape(-1, 13)
    assert np.array_equal(body[:fo[3]], good[:fo[3]])
    assert np.all(body[fo[3]:] == SENT)


@pytest.mark.gpu
def test_graph_capture_replays_on_new_input(ss, sslib):
    import torch

    from speechsauce_amd import _lib

    lens = np.array([16000, 7777, 640, 32001, 20000], dtype=np.int64)
    n = int(lens.sum())
    cfg = ss.SpeechConfig(_lib.make_params())
    so, fo = ss._packed_offsets(cfg, lens, n, "t")
    dso, dfo = torch.from_numpy(so).cuda(), torch.from_numpy(fo).cuda()
    rows = int(fo[-1])
    x = _signal(torch, n, 9)
    out = torch.empty((rows, 13), device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):  # warm-up off the capture
        assert sslib.ss_mfcc_packed_device(cfg.handle, x.data_ptr(), 5, dso.data_ptr(), dfo.data_ptr(), rows, out.data_ptr(),
                                           C.c_void_p(s.cuda_stream)) == 0
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        rc = sslib.ss_mfcc_packed_device(cfg.handle, x.data_ptr(), 5, dso.data_ptr(), dfo.data_ptr(), rows, out.data_ptr(),
                                         C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    for seed in (21, 22):
        x.copy_(_signal(torch, n, seed))
        g.replay()
        torch.cuda.synchronize()
        eager = torch.empty_like(out)
        assert sslib.ss_mfcc_packed_device(cfg.handle, x.data_ptr(), 5, dso.data_ptr(), dfo.data_ptr(), rows, eager.data_ptr(),
                                           None) == 0
        torch.cuda.synchronize()
        assert torch.equal(out, eager)
    cfg.device_status()


@pytest.mark.gpu
def test_host_path_and_list_form_match_the_device_path(ss, sslib):
    import torch

    rng = np.random.default_rng(15)
    lens = _lengths(rng, 64)
    x = _signal(torch, int(lens.sum()), 10)
    dev, fo_d = ss.mfcc_packed(x, lens.tolist(), 16000)
    host, fo_h = ss.mfcc_packed(x.cpu().numpy(), lens, 16000)
    torch.cuda.synchronize()
    assert isinstance(host, np.ndarray) and np.array_equal(fo_h, fo_d.cpu().numpy())
    assert np.array_equal(host, dev.cpu().numpy())
    fh, eh, _ = ss.mfe_packed(x.cpu().numpy(), lens, 16000)
    fd, ed, _ = ss.mfe_packed(x, lens, 16000)
    assert np.array_equal(fh, fd.cpu().numpy()) and np.array_equal(eh, ed.cpu().numpy())
    so = np.concatenate([[0], np.cumsum(lens)])
    clips = [x[int(so[b]):int(so[b + 1])] for b in range(len(lens))]
    lst = ss.mfcc_list(clips, 16000)
    assert len(lst) == len(lens)
    for b, f in enumerate(lst):
        assert torch.equal(f, dev[int(fo_h[b]):int(fo_h[b + 1])]), b
    lst_h = ss.mfcc_list([c.cpu().numpy() for c in clips], 16000)
    assert all(np.array_equal(a, b.cpu().numpy()) for a, b in zip(lst_h, lst))
    with pytest.raises(ValueError):
        ss.mfcc_list([clips[0], clips[1].cpu().numpy()], 16000)  # device and host clips in one call
    with pytest.raises(ss.SpeechSauceError) as e:
        ss.mfe_packed(x[:16100], [16000, 100], 16000)  # the second clip has no frame
    assert e.value.status == 1 and "clip 1" in e.value.detail
