"""The Whisper log-mel calls fed signed 16-bit PCM: ss_whisper_log_mel[_packed]_i16[_device] and ``pcm_scale=`` of whisper_log_mel,
whisper_log_mel_packed and whisper_log_mel_list -- the PCM build of the middle launch, ss_whisper_c200i.

Contract: sample = (float)pcm * scale, scale a power of two, so ``out`` in all three dtypes, ``lengths`` and the handle's error status
are bit for bit what the float entry point gives on ``pcm.astype(float32) * scale``.  Every comparison below is on raw bits against
that float call; no tolerance appears.  Parity with f64 is the float call's (tests/test_whisper.py) and is not measured again.

The inputs are the three kinds of tests/test_whisper.py rounded to int16 (the normalised kinds times 32768 first), with -32768 and
32767 placed in every clip of two samples or more; scales are 2^-15 and 1.0."""
import ctypes as C

import numpy as np
import pytest

import whisper_model as wm
from test_whisper import BF16, F16, F32, KINDS, LENS, _bits

pytestmark = pytest.mark.gpu
SCALES = [2.0 ** -15, 1.0]
DTYPES = ("float32", "float16", "bfloat16")


@pytest.fixture(scope="module")
def torch():
    import torch

    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def ss(sslib):
    import speechsauce_amd

    return speechsauce_amd


def pcm_input(kind, n, seed):
    """wm.make_input as int16: 'pcm' is in sample units already, the others are normalised; the extremes at the clip's ends"""
    x = wm.make_input(kind, n, seed).astype(np.float64)
    p = np.clip(np.rint(x if kind == "pcm" else x * 32768.0), -32768, 32767).astype(np.int16)
    if n >= 2:
        p[0], p[-1] = -32768, 32767
    return p


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda() if a.size else torch.zeros(0, dtype=torch.int16, device="cuda")


def converted(torch, pcm, scale):
    return pcm.to(torch.float32) * scale


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("n_mels", (80, 128))
def test_dense_equals_the_float_call_bit_for_bit(ss, sslib, torch, n_mels, scale):
    """A batch row of each kind; the default frame count and 50 frames of 16000-sample rows (the trim); the rows at an even and at an
    odd sample of their allocation (a strided batch: 2-byte alignment only); every dtype."""
    x = np.stack([pcm_input(kind, 16000, 10 + i) for i, kind in enumerate(KINDS)])
    for base in (0, 1):
        buf = torch.zeros(base + 3 * 16001 + 8, dtype=torch.int16, device="cuda")
        rows = buf[base:base + 3 * 16001].view(3, 16001)[:, :16000]
        rows.copy_(torch.from_numpy(x))
        assert rows.data_ptr() % 4 == 2 * base and rows.stride(0) == 16001
        fbuf = converted(torch, buf, scale)
        frows = fbuf[base:base + 3 * 16001].view(3, 16001)[:, :16000]
        for nf in (None, 50):
            for dtype in DTYPES:
                want = ss.whisper_log_mel(frows, n_mels=n_mels, n_frames=nf, dtype=dtype)
                assert sslib.ss_last_kernel_name() == b"ss_whisper_c200"
                got = ss.whisper_log_mel(rows, n_mels=n_mels, n_frames=nf, dtype=dtype, pcm_scale=scale)
                assert sslib.ss_last_kernel_name() == b"ss_whisper_c200i"
                assert got.shape == want.shape == (3, n_mels, nf or 100) and got.dtype == want.dtype
                assert np.array_equal(_bits(got), _bits(want)), (base, nf, dtype)
    # one clip, short ones included (every frame an edge frame; an empty clip)
    for n in (0, 1, 7, 160, 333, 4801):
        p = pcm_input("normal", n, 20 + n)
        want = ss.whisper_log_mel(converted(torch, dev(torch, p), scale), n_mels=n_mels, n_frames=9)
        got = ss.whisper_log_mel(dev(torch, p), n_mels=n_mels, n_frames=9, pcm_scale=scale)
        assert np.array_equal(_bits(got), _bits(want)), n


def packed_inputs(seed=40):
    clips = [pcm_input(KINDS[i % 3], n, seed + i) for i, n in enumerate(LENS)]
    return clips, np.concatenate(clips)


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_packed_equals_the_float_call_and_every_clip_the_dense_call(ss, torch, dtype, scale):
    """LENS of tests/test_whisper.py: odd and even offsets, an empty clip, clips shorter than the reflect margin; n_frames = 100"""
    clips, packed = packed_inputs()
    pcm = dev(torch, packed)
    want, want_len = ss.whisper_log_mel_packed(converted(torch, pcm, scale), LENS, n_frames=100, dtype=dtype)
    got, got_len = ss.whisper_log_mel_packed(pcm, LENS, n_frames=100, dtype=dtype, pcm_scale=scale)
    assert got.shape == (len(LENS), 80, 100) and got_len.cpu().tolist() == [min(n // 160, 100) for n in LENS]
    assert np.array_equal(_bits(got), _bits(want)) and torch.equal(got_len, want_len)
    for b, c in enumerate(clips):
        one = ss.whisper_log_mel(dev(torch, c), n_frames=100, dtype=dtype, pcm_scale=scale)
        assert np.array_equal(_bits(got[b]), _bits(one)), b


def raw_packed(sslib, torch, cfg, x, scale, so, n_frames, code, work, out, lens):
    """the device entry as it stands (scale None: the float entry) -> its return code"""
    sc = [] if scale is None else [scale]
    fn = sslib.ss_whisper_log_mel_packed_device if scale is None else sslib.ss_whisper_log_mel_packed_i16_device
    return fn(cfg.handle, x.data_ptr(), so.numel() - 1, so.data_ptr(), *sc, n_frames, code, work.data_ptr() if work is not None else None,
              out.data_ptr(), lens.data_ptr(), C.c_void_p(torch.cuda.current_stream().cuda_stream))


@pytest.mark.parametrize("code", (F32, BF16))
def test_a_bad_table_entry_is_contained_as_in_the_float_call(ss, sslib, torch, code):
    """tests/test_whisper.py::test_a_bad_table_entry_is_contained beside the float call on the converted samples: guards untouched, the
    same blocks of -1.5, the same lengths, the same status -- whole buffers compared on bits."""
    scale = 2.0 ** -15
    cfgs = {True: ss.WhisperConfig(80), False: ss.WhisperConfig(80)}  # (each call family its own error word)
    nf, n, M = 20, 4, 80
    clips = [pcm_input("normal", k, 300 + i) for i, k in enumerate((3000, 1700, 900, 2500))]
    pcm = dev(torch, np.concatenate(clips))
    xf = converted(torch, pcm, scale)
    good = np.concatenate([[0], np.cumsum([c.size for c in clips])]).astype(np.int64)
    tdt = torch.float32 if code == F32 else torch.bfloat16
    guard = 64  # elements: a multiple of 16 bytes for both types

    def run(table, as_pcm):
        so = torch.from_numpy(table).cuda()
        blk = torch.full((n * M * nf + 2 * guard,), 7.0, dtype=tdt, device="cuda")
        wblk = torch.full((n * M * nf + 2 * guard,), 9.0, dtype=torch.float32, device="cuda")
        lblk = torch.full((n + 2,), -77, dtype=torch.int32, device="cuda")
        out, work, lens = blk[guard:guard + n * M * nf], wblk[guard:guard + n * M * nf], lblk[1:1 + n]
        rc = raw_packed(sslib, torch, cfgs[as_pcm], pcm if as_pcm else xf, scale if as_pcm else None, so, nf, code,
                        work if code != F32 else None, out, lens)
        torch.cuda.synchronize()
        status = sslib.ss_whisper_config_device_status(cfgs[as_pcm].handle)
        again = sslib.ss_whisper_config_device_status(cfgs[as_pcm].handle)
        assert bool((blk[:guard] == 7.0).all()) and bool((blk[-guard:] == 7.0).all())
        assert bool((wblk[:guard] == 9.0).all()) and bool((wblk[-guard:] == 9.0).all())
        return (rc, status, again), _bits(blk), lblk.cpu().numpy()

    codes, blk, lens = run(good, True)
    codes_f, blk_f, lens_f = run(good, False)
    assert codes == codes_f == (0, 0, 0) and np.array_equal(blk, blk_f) and np.array_equal(lens, lens_f)
    minus = _bits(torch.full((1,), -1.5, dtype=tdt))[0]
    for bad_clip in (1, 2):
        table = good.copy()
        if bad_clip == 1:
            table[2] = table[1] - 5      # a decreasing pair
        else:
            table[2], table[3] = -4, -2  # negative offsets
        codes, blk, lens = run(table, True)
        codes_f, blk_f, lens_f = run(table, False)
        assert codes == codes_f == (0, 6, 0)  # SS_ERR_DEVICE, once
        assert np.array_equal(blk, blk_f) and np.array_equal(lens, lens_f)
        body = blk[guard:-guard].reshape(n, M, nf)
        bad = [b for b in range(n) if table[b] < 0 or table[b + 1] < table[b]]
        assert bad_clip in bad and lens[0] == lens[-1] == -77
        for b in bad:
            assert (body[b] == minus).all() and lens[1 + b] == -1


@pytest.mark.parametrize("scale", SCALES)
def test_host_forms_and_python_front(ss, sslib, torch, scale):
    x = np.stack([pcm_input(KINDS[s % 3], 5000, 70 + s) for s in range(3)])
    for dtype in DTYPES:
        d = ss.whisper_log_mel(dev(torch, x), n_mels=128, n_frames=33, dtype=dtype, pcm_scale=scale)
        h = ss.whisper_log_mel(x, n_mels=128, n_frames=33, dtype=dtype, pcm_scale=scale)  # numpy in: the host form, int16 over the link
        assert isinstance(h, np.ndarray) and np.array_equal(h.view(np.uint32 if dtype == "float32" else np.uint16), _bits(d)), dtype
        assert np.array_equal(_bits(d), _bits(ss.whisper_log_mel(converted(torch, dev(torch, x), scale), n_mels=128, n_frames=33, dtype=dtype)))
    # the C entries directly: a strided host batch (ld > n_samples), the packed host form with its lengths
    cfg = ss.WhisperConfig(80)
    wide = np.concatenate([x, np.full((3, 3), 1234, np.int16)], axis=1)
    out = np.full((3, 80, 33), 7.0, np.float32)
    assert sslib.ss_whisper_log_mel_i16(cfg.handle, wide.ctypes.data, 3, 5000, 5003, scale, 33, F32, out.ctypes.data) == 0, sslib.ss_last_error_string()
    assert np.array_equal(out.view(np.uint32), _bits(ss.whisper_log_mel(dev(torch, x), n_frames=33, pcm_scale=scale)))
    clips, packed = packed_inputs()
    h_out, h_len = ss.whisper_log_mel_packed(packed, LENS, n_frames=20, pcm_scale=scale)
    d_out, d_len = ss.whisper_log_mel_packed(dev(torch, packed), LENS, n_frames=20, pcm_scale=scale)
    f_out, f_len = ss.whisper_log_mel_packed(converted(torch, dev(torch, packed), scale), LENS, n_frames=20)
    assert isinstance(h_out, np.ndarray) and np.array_equal(h_out.view(np.uint32), _bits(d_out)) and np.array_equal(h_len, d_len.cpu().numpy())
    assert np.array_equal(_bits(d_out), _bits(f_out)) and torch.equal(d_len, f_len)
    for lst in (clips, [dev(torch, c) for c in clips]):
        l_out, l_len = ss.whisper_log_mel_list(lst, n_frames=20, pcm_scale=scale)
        l_out, l_len = (l_out.cpu().numpy(), l_len.cpu().numpy()) if hasattr(l_out, "cpu") else (l_out, l_len)
        assert np.array_equal(l_out.view(np.uint32), h_out.view(np.uint32)) and np.array_equal(l_len, h_len)
    cfg.device_status()


def test_argument_errors(ss, sslib, torch):
    cfg = ss.WhisperConfig(80)
    x = torch.zeros(4000, dtype=torch.int16, device="cuda")
    out = torch.full((2 * 80 * 8 + 8,), 7.0, dtype=torch.float32, device="cuda")
    so = torch.tensor([0, 1280, 2560], dtype=torch.int64, device="cuda")
    lens = torch.full((2,), -77, dtype=torch.int32, device="cuda")
    hso = so.cpu().numpy()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    call = lambda xp, ld, sc, nf, dt, work, op: sslib.ss_whisper_log_mel_i16_device(cfg.handle, xp, 2, 1280, ld, sc, nf, dt, work, op, st)
    for bad in (3.0, 0.0, float("nan"), 2.0 ** 70):
        assert call(x.data_ptr(), 1280, bad, 8, F32, None, out.data_ptr()) == 3
        assert b"scale must be a power of two" in sslib.ss_last_error_string()
        assert sslib.ss_whisper_log_mel_packed_i16_device(cfg.handle, x.data_ptr(), 2, so.data_ptr(), bad, 8, F32, None, out.data_ptr(), lens.data_ptr(), st) == 3
        hx, ho = np.zeros(2560, np.int16), np.full((2, 80, 8), 7.0, np.float32)
        assert sslib.ss_whisper_log_mel_i16(cfg.handle, hx.ctypes.data, 2, 1280, 1280, bad, 8, F32, ho.ctypes.data) == 3
        assert sslib.ss_whisper_log_mel_packed_i16(cfg.handle, hx.ctypes.data, 2, hso.ctypes.data, bad, 8, F32, ho.ctypes.data, None) == 3
        assert (ho == 7.0).all()
    # the float call's rules, in its order
    assert call(x.data_ptr(), 1279, 1.0, 8, F32, None, out.data_ptr()) == 3   # ld < n_samples
    assert call(x.data_ptr(), 1280, 1.0, 1, F32, None, out.data_ptr()) == 3   # n_frames < 2
    assert call(None, 1280, 1.0, 8, F32, None, out.data_ptr()) == 3           # null buffers
    assert call(x.data_ptr(), 1280, 1.0, 8, BF16, None, out.data_ptr()) == 3  # the 16-bit types need the scratch
    assert call(x.data_ptr() + 1, 1280, 1.0, 8, F32, None, out.data_ptr()) == 3   # an odd address
    assert call(x.data_ptr(), 1280, 1.0, 8, F32, None, out.data_ptr() + 4) == 3
    assert sslib.ss_whisper_log_mel_packed_i16_device(cfg.handle, x.data_ptr(), 2, None, 1.0, 8, F32, None, out.data_ptr(), None, st) == 3
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((lens == -77).all())
    assert call(x.data_ptr() + 2, 1280, 1.0, 8, F32, None, out.data_ptr()) == 0   # 2-byte alignment is enough
    assert sslib.ss_whisper_log_mel_i16_device(cfg.handle, None, 0, 1280, 1280, 1.0, 8, F32, None, None, st) == 0  # an empty batch
    torch.cuda.synchronize()
    cfg.device_status()


def test_replayed_graph_over_changed_tables_equals_eager(ss, sslib, torch):
    """One packed PCM call (bfloat16: all three launches and the scratch), captured and replayed after the table and the samples were
    overwritten in place: the replay equals the eager PCM call and the float call on the new table."""
    scale = 2.0 ** -15
    cfg = ss.WhisperConfig(80)
    nf, n = 20, 6
    rng = np.random.default_rng(5)
    x = dev(torch, pcm_input("normal", 40000, 1))
    so = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    out = torch.empty((n, 80, nf), dtype=torch.bfloat16, device="cuda")
    work = torch.empty((n * 80 * nf,), dtype=torch.float32, device="cuda")
    lens = torch.empty((n,), dtype=torch.int32, device="cuda")
    tables = [np.concatenate([[0], np.cumsum(rng.integers(0, 6000, n))]).astype(np.int64) for _ in range(3)]
    so.copy_(torch.from_numpy(tables[0]).cuda())
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        assert raw_packed(sslib, torch, cfg, x, scale, so, nf, BF16, work, out, lens) == 0  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        assert raw_packed(sslib, torch, cfg, x, scale, so, nf, BF16, work, out, lens) == 0
    assert sslib.ss_last_kernel_name() == b"ss_whisper_c200i"
    for k, tab in enumerate(tables[1:] + tables[:1]):
        so.copy_(torch.from_numpy(tab).cuda())
        x.copy_(dev(torch, pcm_input("tone" if k == 1 else "normal", 40000, 2 + k)))
        out.zero_()
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        got, got_len = _bits(out).copy(), lens.cpu().numpy().copy()
        eager, eager_len = ss.whisper_log_mel_packed(x, np.diff(tab).tolist(), n_frames=nf, dtype="bfloat16", pcm_scale=scale)
        want, want_len = ss.whisper_log_mel_packed(converted(torch, x, scale), np.diff(tab).tolist(), n_frames=nf, dtype="bfloat16")
        assert np.array_equal(got, _bits(eager)) and np.array_equal(got_len, eager_len.cpu().numpy())
        assert np.array_equal(got, _bits(want)) and np.array_equal(got_len, want_len.cpu().numpy())
    cfg.device_status()
