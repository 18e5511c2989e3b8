"""The mel spectrogram / STFT calls fed signed 16-bit PCM: ss_mel_spectrogram_i16 / ss_stft_i16, their packed and ragged streaming
pool forms, the *_device forms of all six, and ``pcm_scale=`` of mel_spectrogram, stft, mel_spectrogram_packed, mel_spectrogram_list,
stft_packed, MelSpectrogramStreamPool and StftStreamPool.

Contract: sample = (float)pcm * scale, scale a power of two, so every output -- and every pool row afterwards -- is bit for bit what
the float entry point leaves on ``pcm.float() * scale`` with the same arguments.  Every comparison below is ``torch.equal`` on the raw
bits against that float call, made in the same test; outputs are pre-filled with NaN, a few rows larger than needed, and the spare
rows are compared too.  No tolerance appears.

Which kernel runs is the rule of speechsauce_amd.h: the PCM build of the kernel the float call picks, where it has one.  The dense
twelve-wave build is asked for with the lab library's ss_debug_mel_tile(3) (as tests/test_stream_packed.py does); the generic
kernel's dense runs at 2048 points use ss_debug_force_generic, because the float call runs a dedicated build there.
"""
import ctypes as C
import os

import numpy as np
import pytest

from common import CONFIGS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = [f"ss_{fn}{layout}_i16{dev}" for fn in ("mel_spectrogram", "stft") for layout in ("", "_packed", "_stream_packed")
         for dev in ("", "_device")]
SS_ERR_ARG, SS_ERR_DEVICE = 3, 6
SCALES = [2.0 ** -15, 1.0]
SPARE = 3  # rows behind every output that no call may write

CFG3 = dict(CONFIGS["cfg3"])  # 2048 / 512, 128 filters: the twelve-wave kernel's shape
CFG3_KW = dict(frame_length=0.032, num_filters=128, fft_length=2048, high_frequency=8000.0)
ODD_HOP = dict(sample_rate=16000, fft_points=2048, frame_length=600 / 16000, num_filters=64)  # H = 600 does not divide W
W512 = dict(sample_rate=16000, fft_points=512, frame_length=0.016)  # a dedicated mel kernel without a PCM build
GENERIC = {
    "W256": dict(sample_rate=16000, fft_points=256, frame_length=0.008),  # a power of two with no dedicated mel kernel
    "chirpz400": dict(sample_rate=16000, fft_points=400, frame_length=0.01),  # hop 160: the chirp-z path
    "bank_past_512": dict(CFG3, mel_scale="slaney", mel_norm="slaney"),  # a 2048-point bank over the whole spectrum
}
PACKED_LENS = [1, 511, 512, 513, 2048, 2049, 5000]  # a clip shorter than a hop, odd row counts, offsets of both parities
POOL_ROWS, POOL_SLOTS, POOL = [0, 1, 2, 3, 1], [5, 2, 7, 0, 3], 8


def _cfg(ss, **kw):
    from speechsauce_amd import _lib

    return ss.SpeechConfig(_lib.make_params(**kw))


# ---------------------------------------------------------------- CPU ---------------------------------------------------------

def test_the_twelve_entries_are_exported_and_declared(sslib):
    header = open(os.path.join(ROOT, "include", "speechsauce_amd.h")).read()
    from speechsauce_amd import _lib

    assert len(NAMES) == 12
    for n in NAMES:
        assert hasattr(sslib, n), n
        assert n in _lib.PROTOTYPES, n
        assert f"int {n}(const ss_config *cfg, const int16_t *" in header, n
    # a null config: what the float entries answer
    for fn in ("mel_spectrogram", "stft"):
        f = lambda name: getattr(sslib, f"ss_{fn}{name}")
        assert f("_i16_device")(None, None, 1, 512, 512, 1.0, None, None) == f("_device")(None, None, 1, 512, 512, None, None) == SS_ERR_ARG
        assert f("_i16")(None, None, 1, 512, 1.0, None) == f("")(None, None, 1, 512, None) == SS_ERR_ARG
        assert f("_packed_i16_device")(None, None, 1, None, 1.0, None, 1, None, None) == \
            f("_packed_device")(None, None, 1, None, None, 1, None, None) == SS_ERR_ARG
        assert f("_packed_i16")(None, None, 1, None, 1.0, None) == f("_packed")(None, None, 1, None, None) == SS_ERR_ARG
        assert f("_stream_packed_i16_device")(None, None, 1, None, None, 1, None, 1, 1.0, None, None, None) == \
            f("_stream_packed_device")(None, None, 1, None, None, 1, None, 1, None, None, None) == SS_ERR_ARG
        assert f("_stream_packed_i16")(None, None, 1, None, None, 1, 1.0, None, None) == \
            f("_stream_packed")(None, None, 1, None, None, 1, None, None) == SS_ERR_ARG
    assert sslib.ss_abi_version() == 7  # only entry points were added


def test_python_pcm_argument_rules(sslib):
    """int16 needs pcm_scale, float32 takes none, and a scale must be a power of two in [2**-64, 2**64]: all raised before the
    library is called (this test runs without a device)."""
    import speechsauce_amd as ss

    p1, f1 = np.zeros(2048, np.int16), np.zeros(2048, np.float32)
    calls = [(ss.mel_spectrogram, (), CFG3_KW), (ss.stft, (), dict(frame_length=0.032, fft_length=2048)),
             (ss.mel_spectrogram_packed, ([1024, 1024],), CFG3_KW), (ss.stft_packed, ([1024, 1024],), dict(frame_length=0.032, fft_length=2048)),
             (lambda x, *a, **k: ss.mel_spectrogram_list([x, x], *a, **k), (), CFG3_KW)]
    for fn, extra, kw in calls:
        with pytest.raises(TypeError):
            fn(p1, *extra, 16000, **kw)  # int16 without pcm_scale
        with pytest.raises(TypeError):
            fn(f1, *extra, 16000, pcm_scale=2.0 ** -15, **kw)  # floats are not PCM
        for bad in (1 / 32767, 3.0, 0, -0.5, 2.0 ** 70, 2.0 ** -65, float("nan"), float("inf")):
            with pytest.raises(ValueError):
                fn(p1, *extra, 16000, pcm_scale=bad, **kw)
    with pytest.raises(ValueError):
        ss.mel_spectrogram([np.zeros((2, 2048), np.int16)], 16000, pcm_scale=1.0, **CFG3_KW)  # a list of blocks has no PCM form
    pools = [ss.MelSpectrogramStreamPool(4, 16000, frame_length=0.032, num_filters=128, fft_length=2048, high_frequency=8000.0),
             ss.StftStreamPool(4, 16000, frame_length=0.032, fft_length=2048)]
    for pool in pools:
        with pytest.raises(TypeError):
            pool([p1[:512]], [0])
        with pytest.raises(TypeError):
            pool([f1[:512]], [0], pcm_scale=1.0)
        for bad in (3.0, 2.0 ** 70, float("nan")):
            with pytest.raises(ValueError):
                pool([p1[:512]], [0], pcm_scale=bad)
        assert pool.state is None  # nothing ran


# ---------------------------------------------------------------- GPU ---------------------------------------------------------

def _st(torch, stream=None):
    return C.c_void_p(stream if stream is not None else torch.cuda.current_stream().cuda_stream)


def _same_bits(a, b):
    import torch

    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _random_pcm(torch, n, seed):
    """n random samples, the first two the extremes -32768 and 32767"""
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    x = torch.randint(-32768, 32768, (n,), generator=g, device="cuda", dtype=torch.int32).to(torch.int16)
    if n >= 2:
        x[0], x[1] = -32768, 32767
    return x


def _row_floats(cfg, fn):
    return cfg.params.num_filters if fn == "mel" else 2 * (cfg.params.fft_points // 2 + 1)


def _hop(cfg):
    return int(np.float32(cfg.params.frame_length) * np.float32(cfg.params.sample_rate))


def _entry(lib, fn, layout, scale, dev=True):
    name = {"mel": "mel_spectrogram", "stft": "stft"}[fn]
    return getattr(lib, f"ss_{name}{layout}{'' if scale is None else '_i16'}{'_device' if dev else ''}")


def _dense(torch, lib, cfg, fn, ptr, ch, n, ld, scale, out):
    """ss_{mel_spectrogram,stft}[_i16]_device on the buffer at `ptr` (scale None: the float form); returns (status, kernel name)."""
    sc = [] if scale is None else [scale]
    rc = _entry(lib, fn, "", scale)(cfg.handle, ptr, ch, n, ld, *sc, out.data_ptr(), _st(torch))
    return rc, lib.ss_last_kernel_name()


def _check_dense(torch, lib, cfg, fn, clips, scale):
    """ld = n, ld = n + 1 and base + 1 sample through the PCM call and the float call on the converted buffer; returns the
    (float name, PCM name) pairs."""
    ch, n = clips.shape
    floats = ch * cfg.stft_rows(n)[0] * _row_floats(cfg, fn)
    names = []
    for label, base, ld in (("ld=n", 0, n), ("ld=n+1", 0, n + 1), ("base+1", 1, n)):
        buf = _random_pcm(torch, base + ch * ld + 8, 7)  # (the gaps and the tail hold samples that no window may read)
        for b in range(ch):
            buf[base + b * ld: base + b * ld + n] = clips[b]
        xf = buf.to(torch.float32) * scale
        want = torch.full((floats + SPARE * _row_floats(cfg, fn),), float("nan"), device="cuda")
        got = want.clone()
        rc, fname = _dense(torch, lib, cfg, fn, xf.data_ptr() + 4 * base, ch, n, ld, None, want)
        assert rc == 0, lib.ss_last_error_string()
        rc, iname = _dense(torch, lib, cfg, fn, buf.data_ptr() + 2 * base, ch, n, ld, scale, got)
        assert rc == 0, lib.ss_last_error_string()
        torch.cuda.synchronize()
        assert not torch.isnan(want[:floats]).any() and torch.isnan(want[floats:]).all(), label
        assert _same_bits(got, want), (label, (got != want).sum().item())
        names.append((fname, iname))
    assert lib.ss_config_device_status(cfg.handle) == 0
    return names


def _clips(torch, ch, n, seed):
    return _random_pcm(torch, ch * n, seed).reshape(ch, n)


@pytest.mark.gpu
@pytest.mark.parametrize("scale", SCALES)
def test_twelve_wave_dense_build_and_its_eight_wave_fallback(ss, sslib, sslab, scale):
    import torch

    from speechsauce_amd import _lib

    clips = _clips(torch, 3, 5000, 1)
    with _lib.use_library(sslab):
        try:
            sslab.ss_debug_mel_tile(3)  # twelve waves wherever that build exists
            names = _check_dense(torch, sslab, _cfg(ss, **CFG3), "mel", clips, scale)
        finally:
            sslab.ss_debug_mel_tile(1)
    for fname, iname in names:
        assert fname == b"ss_mel_c1024<w12,mel6321>" and iname == b"ss_mel_c1024i<w12,mel6321>", (fname, iname)
    # the same call as the product library serves it: 30 units select eight waves, so the float kernel runs behind the conversion
    for fname, iname in _check_dense(torch, sslib, _cfg(ss, **CFG3), "mel", clips, scale):
        assert fname == iname == b"ss_mel_c1024", (fname, iname)


@pytest.mark.gpu
@pytest.mark.parametrize("fn", ["mel", "stft"])
def test_dense_fallback_reports_the_float_kernel(ss, sslib, fn):
    """A dense 512-point call (a dedicated kernel without a PCM build), and stft output at 2048 points (the eight-wave family)."""
    import torch

    for kw, n in ((W512, 3000), (CFG3, 5000)):
        for fname, iname in _check_dense(torch, sslib, _cfg(ss, **kw), fn, _clips(torch, 2, n, 2), 2.0 ** -15):
            assert fname == iname and b"i16" not in iname and not iname.startswith(b"ss_mel_c1024i"), (fname, iname)


def _offsets(ss, cfg, lens):
    so = np.zeros(len(lens) + 1, np.int64)
    np.cumsum(lens, out=so[1:])
    return so, ss._row_offsets(cfg, so)


def _packed(torch, lib, cfg, fn, x, n_clips, dso, dro, total, scale, out, stream=None):
    sc = [] if scale is None else [scale]
    rc = _entry(lib, fn, "_packed", scale)(cfg.handle, x.data_ptr(), n_clips, dso.data_ptr(), *sc, dro.data_ptr(), total, out.data_ptr(),
                                           _st(torch, stream))
    return rc, lib.ss_last_kernel_name()


def _check_packed(torch, ss, lib, cfg, fn, lens, scale, seed=3):
    """The packed device forms on one buffer; returns (PCM buffer, so, ro, PCM result, kernel name)."""
    so, ro = _offsets(ss, cfg, lens)
    rows, rf = int(ro[-1]), _row_floats(cfg, fn)
    pcm = _random_pcm(torch, int(so[-1]), seed)
    xf = pcm.to(torch.float32) * scale
    dso, dro = torch.from_numpy(so).cuda(), torch.from_numpy(ro).cuda()
    want = torch.full((rf * (rows + SPARE),), float("nan"), device="cuda")
    got = want.clone()
    rc, _ = _packed(torch, lib, cfg, fn, xf, len(lens), dso, dro, rows, None, want)
    assert rc == 0, lib.ss_last_error_string()
    rc, iname = _packed(torch, lib, cfg, fn, pcm, len(lens), dso, dro, rows, scale, got)
    assert rc == 0, lib.ss_last_error_string()
    torch.cuda.synchronize()
    assert not torch.isnan(want[:rf * rows]).any() and torch.isnan(want[rf * rows:]).all()
    assert _same_bits(got, want), (got != want).sum().item()
    assert lib.ss_config_device_status(cfg.handle) == 0
    return pcm, so, ro, got[:rf * rows], iname


@pytest.mark.gpu
@pytest.mark.parametrize("scale", SCALES)
def test_packed_forms_equal_the_float_calls_bit_for_bit(ss, sslib, scale):
    import torch

    cfg = _cfg(ss, **CFG3)
    pcm, so, ro, got, iname = _check_packed(torch, ss, sslib, cfg, "mel", PACKED_LENS, scale)
    assert iname == b"ss_mel_c1024vi<w12,mel6321>", iname
    assert (so[1:-1] % 2 == 1).any() and (so[1:-1] % 2 == 0).any() and (np.diff(ro) % 2 == 1).any()
    # the host form
    host = np.full(got.numel(), np.nan, np.float32)
    x = pcm.cpu().numpy()
    rc = sslib.ss_mel_spectrogram_packed_i16(cfg.handle, x.ctypes.data, len(PACKED_LENS), so.ctypes.data, scale, host.ctypes.data)
    assert rc == 0, sslib.ss_last_error_string()
    assert _same_bits(torch.from_numpy(host).cuda(), got)
    # mel_spectrogram_list, on the device and from host arrays
    clips = [pcm[so[i]:so[i + 1]] for i in range(len(PACKED_LENS))]
    want_list = ss.mel_spectrogram_list([c.to(torch.float32) * scale for c in clips], 16000, **CFG3_KW)
    for form in (clips, [c.cpu().numpy() for c in clips]):
        got_list = ss.mel_spectrogram_list(form, 16000, pcm_scale=scale, **CFG3_KW)
        for i, (g, w) in enumerate(zip(got_list, want_list)):
            g = g if torch.is_tensor(g) else torch.from_numpy(np.ascontiguousarray(g)).cuda()
            assert _same_bits(g, w), i
            assert _same_bits(g, got[128 * int(ro[i]):128 * int(ro[i + 1])].reshape(128, -1)), i
    # stft_packed on a generic configuration, through the front
    kw = dict(frame_length=0.01, fft_length=400)
    z, zro = ss.stft_packed(pcm, PACKED_LENS, 16000, pcm_scale=scale, **kw)
    assert sslib.ss_last_kernel_name().startswith(b"ss_front_generic_varrowsi<"), sslib.ss_last_kernel_name()
    zw, _ = ss.stft_packed(pcm.to(torch.float32) * scale, PACKED_LENS, 16000, **kw)
    zh, _ = ss.stft_packed(pcm.cpu().numpy(), PACKED_LENS, 16000, pcm_scale=scale, **kw)
    assert _same_bits(torch.view_as_real(z), torch.view_as_real(zw))
    assert _same_bits(torch.view_as_real(torch.from_numpy(zh).cuda()), torch.view_as_real(zw))


def _pool_raw(torch, lib, cfg, fn, x, n_active, dso, dro, total_rows, dsl, pool_streams, scale, pool, out, stream=None, x_ptr=None):
    sc = [] if scale is None else [scale]
    rc = _entry(lib, fn, "_stream_packed", scale)(cfg.handle, x.data_ptr() if x_ptr is None else x_ptr, n_active, dso.data_ptr(), dro.data_ptr(),
                                                  total_rows, dsl.data_ptr(), pool_streams, *sc, pool.data_ptr(), out.data_ptr(),
                                                  _st(torch, stream))
    return rc, lib.ss_last_kernel_name()


def _check_pool(torch, lib, cfg, fn, scale, seed=4):
    """Two consecutive ticks on two copies of one pool: (PCM, float) on one, (float, float) on the other.  Rows and the WHOLE pool
    are compared after each tick.  Returns the PCM tick's (samples, so, ro, slots, pool before, rows, pool after, kernel name)."""
    H, S, rf = _hop(cfg), cfg.params.fft_points - _hop(cfg), _row_floats(cfg, fn)
    so = np.zeros(len(POOL_ROWS) + 1, np.int64)
    np.cumsum(np.array(POOL_ROWS) * H, out=so[1:])
    ro = so // H
    rows = int(ro[-1])
    dso, dro = torch.from_numpy(so).cuda(), torch.from_numpy(ro).cuda()
    dsl = torch.tensor(POOL_SLOTS, dtype=torch.int32, device="cuda")
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    before = torch.randn((POOL, S), generator=g, device="cuda") * 0.1
    pool_i, pool_f = before.clone(), before.clone()
    first = None
    for tick in range(2):
        pcm = _random_pcm(torch, int(so[-1]), seed + 1 + tick)
        xf = pcm.to(torch.float32) * scale
        want = torch.full((rf * (rows + SPARE),), float("nan"), device="cuda")
        got = want.clone()
        rc, _ = _pool_raw(torch, lib, cfg, fn, xf, len(POOL_ROWS), dso, dro, rows, dsl, POOL, None, pool_f, want)
        assert rc == 0, lib.ss_last_error_string()
        # the first tick is PCM, the second float on the same streams: the pool stays float
        rc, name = _pool_raw(torch, lib, cfg, fn, pcm if tick == 0 else xf, len(POOL_ROWS), dso, dro, rows, dsl, POOL,
                             scale if tick == 0 else None, pool_i, got)
        assert rc == 0, lib.ss_last_error_string()
        torch.cuda.synchronize()
        assert not torch.isnan(want[:rf * rows]).any() and torch.isnan(want[rf * rows:]).all()
        assert _same_bits(got, want), (tick, (got != want).sum().item())
        assert _same_bits(pool_i, pool_f), tick
        for slot in set(range(POOL)) - set(POOL_SLOTS) | {POOL_SLOTS[0]}:  # untouched rows, the entry without rows among them
            assert _same_bits(pool_i[slot], before[slot]), slot
        if tick == 0:
            first = (pcm, so, ro, dsl, before, got[:rf * rows].clone(), pool_i.clone(), name)
    assert lib.ss_config_device_status(cfg.handle) == 0
    return first


@pytest.mark.gpu
@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("name", ["cfg3", "odd_hop"])
def test_pool_forms_equal_the_float_calls_bit_for_bit(ss, sslib, name, scale):
    import torch

    cfg = _cfg(ss, **(CFG3 if name == "cfg3" else ODD_HOP))
    pcm, so, ro, dsl, before, rows, after, kname = _check_pool(torch, sslib, cfg, "mel", scale)
    assert kname == b"ss_mel_c1024spi<w12,mel6321>" if name == "cfg3" else kname.startswith(b"ss_mel_c1024spi<w12"), kname
    # the host form on the same tick
    S = before.shape[1]
    pool_h = before.cpu().numpy().copy()
    out_h = np.full(rows.numel(), np.nan, np.float32)
    x, sl = pcm.cpu().numpy(), np.array(POOL_SLOTS, np.int32)
    rc = sslib.ss_mel_spectrogram_stream_packed_i16(cfg.handle, x.ctypes.data, len(POOL_ROWS), so.ctypes.data, sl.ctypes.data, POOL, scale,
                                                    pool_h.ctypes.data, out_h.ctypes.data)
    assert rc == 0, sslib.ss_last_error_string()
    assert _same_bits(torch.from_numpy(out_h).cuda(), rows)
    assert _same_bits(torch.from_numpy(pool_h).cuda(), after) and pool_h.shape == (POOL, S)
    # the Python class: PCM on one call
    kw = CFG3_KW if name == "cfg3" else dict(frame_length=600 / 16000, num_filters=64, fft_length=2048)
    pool = ss.MelSpectrogramStreamPool(POOL, 16000, **kw)
    chunks = [pcm[so[i]:so[i + 1]] for i in range(len(POOL_ROWS))]
    pool([c.to(torch.float32) * 0 for c in chunks], POOL_SLOTS)  # places the pool on the device
    pool.state.copy_(before)
    out_p, ro_p = pool(chunks, POOL_SLOTS, pcm_scale=scale)
    torch.cuda.synchronize()
    assert np.array_equal(ro_p, ro) and _same_bits(out_p, rows) and _same_bits(pool.state, after)


@pytest.mark.gpu
@pytest.mark.parametrize("fn", ["mel", "stft"])
@pytest.mark.parametrize("name", list(GENERIC))
def test_generic_kernel_layouts_equal_the_float_calls_bit_for_bit(ss, sslab, name, fn):
    """Dense, packed and pool on the generic kernel's PCM builds (the lab library's ss_debug_force_generic keeps the 2048-point
    dense call off its dedicated build)."""
    import torch

    from speechsauce_amd import _lib

    kw = GENERIC[name]
    with _lib.use_library(sslab):
        try:
            sslab.ss_debug_force_generic(1)
            cfg = _cfg(ss, **kw)
            H = _hop(cfg)
            for scale in SCALES:
                for fname, iname in _check_dense(torch, sslab, cfg, fn, _clips(torch, 3, 5 * H + 77, 5), scale):
                    assert fname.startswith(b"ss_front_generic<") and iname.startswith(b"ss_front_generic_i16<"), (fname, iname)
                lens = [1, H - 1, H, H + 1, 4 * H, 4 * H + 1, 5000]
                pcm, so, ro, got, iname = _check_packed(torch, ss, sslab, cfg, fn, lens, scale)
                assert iname.startswith(b"ss_front_generic_varrowsi<"), iname
                host = np.full(got.numel(), np.nan, np.float32)
                x = pcm.cpu().numpy()
                rc = _entry(sslab, fn, "_packed", scale, dev=False)(cfg.handle, x.ctypes.data, len(lens), so.ctypes.data, scale, host.ctypes.data)
                assert rc == 0, sslab.ss_last_error_string()
                assert _same_bits(torch.from_numpy(host).cuda(), got)
                pcm, so, ro, dsl, before, rows, after, kname = _check_pool(torch, sslab, cfg, fn, scale)
                assert kname.startswith(b"ss_front_generic_streampi<"), kname
                pool_h, out_h = before.cpu().numpy().copy(), np.full(rows.numel(), np.nan, np.float32)
                x, sl = pcm.cpu().numpy(), np.array(POOL_SLOTS, np.int32)
                rc = _entry(sslab, fn, "_stream_packed", scale, dev=False)(cfg.handle, x.ctypes.data, len(POOL_ROWS), so.ctypes.data,
                                                                            sl.ctypes.data, POOL, scale, pool_h.ctypes.data, out_h.ctypes.data)
                assert rc == 0, sslab.ss_last_error_string()
                assert _same_bits(torch.from_numpy(out_h).cuda(), rows) and _same_bits(torch.from_numpy(pool_h).cuda(), after)
        finally:
            sslab.ss_debug_force_generic(0)


@pytest.mark.gpu
@pytest.mark.parametrize("fn", ["mel", "stft"])
def test_dense_host_forms_equal_the_device_forms(ss, sslib, fn):
    import torch

    for kw in (CFG3, GENERIC["chirpz400"]):
        cfg = _cfg(ss, **kw)
        ch, n, scale = 3, 5001, 2.0 ** -15
        clips = _clips(torch, ch, n, 6)
        floats = ch * cfg.stft_rows(n)[0] * _row_floats(cfg, fn)
        dev = torch.full((floats,), float("nan"), device="cuda")
        rc, _ = _dense(torch, sslib, cfg, fn, clips.data_ptr(), ch, n, n, scale, dev)
        assert rc == 0, sslib.ss_last_error_string()
        host = np.full(floats, np.nan, np.float32)
        x = clips.cpu().numpy()
        assert _entry(sslib, fn, "", scale, dev=False)(cfg.handle, x.ctypes.data, ch, n, scale, host.ctypes.data) == 0
        torch.cuda.synchronize()
        assert _same_bits(torch.from_numpy(host).cuda(), dev)
        # the front, device and host
        front = ss.mel_spectrogram if fn == "mel" else ss.stft
        fkw = dict(frame_length=float(cfg.params.frame_length), fft_length=int(cfg.params.fft_points))
        if fn == "mel":
            fkw.update(num_filters=int(cfg.params.num_filters), high_frequency=float(cfg.params.high_frequency))
        for form in (clips, x):
            got = front(form, 16000, pcm_scale=scale, **fkw)
            got = got if torch.is_tensor(got) else torch.from_numpy(np.ascontiguousarray(got)).cuda()
            got = torch.view_as_real(got) if fn == "stft" else got
            assert _same_bits(got.reshape(-1), dev), type(form)


@pytest.mark.gpu
def test_argument_rejections_leave_everything_untouched(ss, sslib):
    import torch

    cfg = _cfg(ss, **CFG3)
    H, S, FILL = 512, 2048 - 512, -777.0
    pcm = _random_pcm(torch, 4 * H + 2, 8)
    so = np.array([0, H, 3 * H], np.int64)
    ro = so // H
    dso, dro = torch.from_numpy(so).cuda(), torch.from_numpy(ro).cuda()
    dsl = torch.tensor([1, 0], dtype=torch.int32, device="cuda")
    null = torch.empty(0, device="cuda")
    assert null.data_ptr() == 0
    for fn in ("mel", "stft"):
        out = torch.full((_row_floats(cfg, fn) * 8,), FILL, device="cuda")
        pool = torch.full((2, S), FILL, device="cuda")
        bad_scales = (3.0, 0.0, -1.0, 2.0 ** 70, 2.0 ** -65, float("nan"), float("inf"), 1 / 32767)
        for bad in bad_scales:
            assert _dense(torch, sslib, cfg, fn, pcm.data_ptr(), 1, 2 * H, 2 * H, bad, out)[0] == SS_ERR_ARG, bad
            assert _packed(torch, sslib, cfg, fn, pcm, 2, dso, dro, 3, bad, out)[0] == SS_ERR_ARG, bad
            assert _pool_raw(torch, sslib, cfg, fn, pcm, 2, dso, dro, 3, dsl, 2, bad, pool, out)[0] == SS_ERR_ARG, bad
            x = pcm.cpu().numpy()
            ho, hp = np.full(8, FILL, np.float32), np.full((2, S), FILL, np.float32)
            assert _entry(sslib, fn, "", bad, dev=False)(cfg.handle, x.ctypes.data, 1, 2 * H, bad, ho.ctypes.data) == SS_ERR_ARG
            assert _entry(sslib, fn, "_packed", bad, dev=False)(cfg.handle, x.ctypes.data, 2, so.ctypes.data, bad, ho.ctypes.data) == SS_ERR_ARG
            sl = np.array([1, 0], np.int32)
            assert _entry(sslib, fn, "_stream_packed", bad, dev=False)(cfg.handle, x.ctypes.data, 2, so.ctypes.data, sl.ctypes.data, 2, bad,
                                                                       hp.ctypes.data, ho.ctypes.data) == SS_ERR_ARG
            assert (ho == FILL).all() and (hp == FILL).all()
        # a misaligned d_x in the pool device form (2-byte aligned only)
        assert _pool_raw(torch, sslib, cfg, fn, pcm, 2, dso, dro, 3, dsl, 2, 1.0, pool, out, x_ptr=pcm.data_ptr() + 2)[0] == SS_ERR_ARG
        # null buffers
        assert _dense(torch, sslib, cfg, fn, 0, 1, 2 * H, 2 * H, 1.0, out)[0] == SS_ERR_ARG
        assert _dense(torch, sslib, cfg, fn, pcm.data_ptr(), 1, 2 * H, 2 * H, 1.0, null)[0] == SS_ERR_ARG
        assert _packed(torch, sslib, cfg, fn, null, 2, dso, dro, 3, 1.0, out)[0] == SS_ERR_ARG
        assert _packed(torch, sslib, cfg, fn, pcm, 2, null, dro, 3, 1.0, out)[0] == SS_ERR_ARG
        assert _packed(torch, sslib, cfg, fn, pcm, 2, dso, dro, 3, 1.0, null)[0] == SS_ERR_ARG
        assert _pool_raw(torch, sslib, cfg, fn, null, 2, dso, dro, 3, dsl, 2, 1.0, pool, out)[0] == SS_ERR_ARG
        assert _pool_raw(torch, sslib, cfg, fn, pcm, 2, dso, dro, 3, dsl, 2, 1.0, null, out)[0] == SS_ERR_ARG
        assert _pool_raw(torch, sslib, cfg, fn, pcm, 2, dso, dro, 3, null, 2, 1.0, pool, out)[0] == SS_ERR_ARG
        # ld < n_samples
        assert _dense(torch, sslib, cfg, fn, pcm.data_ptr(), 2, 2 * H, 2 * H - 1, 1.0, out)[0] == SS_ERR_ARG
        # the pool overlapping the int16 buffer (in bytes of that buffer)
        both = torch.zeros(2 * S, device="cuda")
        as_pcm = both.view(torch.int16)
        assert _pool_raw(torch, sslib, cfg, fn, as_pcm, 2, dso, dro, 3, dsl, 2, 1.0, both.view(2, S), out)[0] == SS_ERR_ARG
        torch.cuda.synchronize()
        assert (out == FILL).all() and (pool == FILL).all(), fn
    assert sslib.ss_config_device_status(cfg.handle) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("kernel,fn", [("headline", "mel"), ("generic", "mel"), ("generic", "stft")])
def test_bad_device_tables_are_contained(ss, sslib, kernel, fn):
    """The tables of tests/test_stream_packed.py::test_bad_device_tables_are_contained (pool) and of
    tests/test_packed_mel.py::test_bad_device_offsets_raise_the_error_word_and_write_nothing_outside (packed) fed to the PCM forms:
    merely inconsistent tables, no access outside the buffers is attempted.  The PCM call must leave exactly what the float call
    leaves -- valid rows written, skipped entries' output and pool rows alone, guards intact -- and raise SS_ERR_DEVICE once."""
    import torch

    kw = CFG3 if kernel == "headline" else dict(sample_rate=16000, fft_points=1000, frame_length=400 / 16000, num_filters=40)
    scale, GUARD, FILL = 2.0 ** -15, 4, -777.0
    cfg_i, cfg_f = _cfg(ss, **kw), _cfg(ss, **kw)  # a config each: the error word is per config
    H, S, rf = _hop(cfg_i), cfg_i.params.fft_points - _hop(cfg_i), _row_floats(cfg_i, fn)
    # ---- the pool: (hops of samples, extra samples, rows claimed in ro, slot, good)
    entries = [(2, 0, 2, 1, True), (1, 0, 1, POOL, False), (1, 0, 1, 3, True), (2, 0, 2, -1, False), (1, 2, 1, 2, False),
               (3, 0, 3, 5, True), (0, 0, 0, 4, True), (1, 0, 2, 6, False), (1, 0, 1, 0, True), (2, 0, 2, 7, False)]
    so = np.zeros(len(entries) + 1, np.int64)
    ro = np.zeros(len(entries) + 1, np.int64)
    for i, (h, extra, claimed, _, _) in enumerate(entries):
        so[i + 1] = so[i] + h * H + extra
        ro[i + 1] = ro[i] + claimed
    total_rows = int(ro[-1]) - 1
    pcm = _random_pcm(torch, int(so[-1]), 9)
    xf = pcm.to(torch.float32) * scale
    dso, dro = torch.from_numpy(so).cuda(), torch.from_numpy(ro).cuda()
    dsl = torch.tensor([e[3] for e in entries], dtype=torch.int32, device="cuda")
    g = torch.Generator(device="cuda")
    g.manual_seed(10)
    res = []
    for cfg, x, sc in ((cfg_f, xf, None), (cfg_i, pcm, scale)):
        pool_g = torch.full((POOL + 2 * GUARD, S), FILL, device="cuda")
        g.manual_seed(10)
        pool_g[GUARD:GUARD + POOL] = torch.randn((POOL, S), generator=g, device="cuda") * 0.1
        out_g = torch.full((rf * (total_rows + 2 * GUARD),), FILL, device="cuda")
        assert sslib.ss_config_device_status(cfg.handle) == 0
        rc, _ = _pool_raw(torch, sslib, cfg, fn, x, len(entries), dso, dro, total_rows, dsl, POOL, sc, pool_g[GUARD:GUARD + POOL],
                          out_g[rf * GUARD:])
        assert rc == 0, sslib.ss_last_error_string()  # the tables are device data: the call itself cannot know
        torch.cuda.synchronize()
        assert sslib.ss_config_device_status(cfg.handle) == SS_ERR_DEVICE  # read and cleared
        assert sslib.ss_config_device_status(cfg.handle) == 0
        res.append((pool_g, out_g))
    (pool_f, out_f), (pool_i, out_i) = res
    assert _same_bits(out_i, out_f) and _same_bits(pool_i, pool_f)
    assert (out_i[:rf * GUARD] == FILL).all() and (out_i[rf * (GUARD + total_rows):] == FILL).all()
    assert (pool_i[:GUARD] == FILL).all() and (pool_i[GUARD + POOL:] == FILL).all()
    body = out_i[rf * GUARD:]
    for i, (h, _, _, slot, good) in enumerate(entries):
        blk = body[rf * int(ro[i]):rf * min(int(ro[i + 1]), total_rows)]
        if not good:
            assert (blk == FILL).all(), i  # the pre-fill is still there
        elif h:
            assert not (blk == FILL).any(), i
    # ---- the packed form: clip 1 claims one row too many; the clips behind it start one row late but are consistent in themselves
    lens = [16000, 8000, 4000, 12000]
    so, ro = _offsets(ss, cfg_i, lens)
    bad = ro.copy()
    bad[2:] += 1
    total = int(bad[-1])
    pcm = _random_pcm(torch, int(so[-1]), 11)
    xf = pcm.to(torch.float32) * scale
    dso, dbad = torch.from_numpy(so).cuda(), torch.from_numpy(bad).cuda()
    res = []
    for cfg, x, sc in ((cfg_f, xf, None), (cfg_i, pcm, scale)):
        blk = torch.full((rf * (total + 2 * GUARD),), FILL, device="cuda")
        rc, _ = _packed(torch, sslib, cfg, fn, x, 4, dso, dbad, total, sc, blk[rf * GUARD:])
        assert rc == 0
        torch.cuda.synchronize()
        assert sslib.ss_config_device_status(cfg.handle) == SS_ERR_DEVICE
        assert sslib.ss_config_device_status(cfg.handle) == 0
        res.append(blk)
    assert _same_bits(res[1], res[0])
    assert (res[1][:rf * GUARD] == FILL).all() and (res[1][rf * (GUARD + total):] == FILL).all()
    assert (res[1][rf * GUARD:][rf * int(bad[1]):rf * int(bad[2])] == FILL).all()  # clip 1 skipped


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", ["headline", "generic"])
def test_graph_replay_over_new_samples_and_tables_equals_eager_calls(ss, sslib, kernel):
    """The packed and the pool PCM device forms, captured once and replayed over rewritten samples and table contents."""
    import torch

    cfg = _cfg(ss, **(CFG3 if kernel == "headline" else GENERIC["chirpz400"]))
    H, S, M, scale = _hop(cfg), cfg.params.fft_points - _hop(cfg), cfg.params.num_filters, 2.0 ** -15
    N, CAP, K = 6, 24, 3
    rng = np.random.default_rng(12)
    # static buffers of the two graphs
    x = torch.zeros(CAP * H, dtype=torch.int16, device="cuda")
    p_so, p_ro = (torch.zeros(N + 1, dtype=torch.int64, device="cuda") for _ in range(2))
    s_so, s_ro = (torch.zeros(N + 1, dtype=torch.int64, device="cuda") for _ in range(2))
    s_sl = torch.arange(N, dtype=torch.int32, device="cuda")
    p_out, s_out = torch.zeros(M * CAP, device="cuda"), torch.zeros(M * CAP, device="cuda")
    g0 = torch.Generator(device="cuda")
    g0.manual_seed(13)
    pool_g = torch.randn((POOL, S), generator=g0, device="cuda") * 0.1
    pool_e = pool_g.clone()
    # warm-up outside the capture: valid one-hop clips for the packed form, entries without rows for the pool (on a scratch pool)
    lens0 = np.full(N, H, np.int64)
    so0, ro0 = _offsets(ss, cfg, lens0)
    p_so.copy_(torch.from_numpy(so0))
    p_ro.copy_(torch.from_numpy(ro0))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        assert _packed(torch, sslib, cfg, "mel", x, N, p_so, p_ro, CAP, scale, p_out, stream=side.cuda_stream)[0] == 0
        assert _pool_raw(torch, sslib, cfg, "mel", x, N, s_so, s_ro, CAP, s_sl, POOL, scale, pool_g.clone(), s_out, stream=side.cuda_stream)[0] == 0
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    gp, gs = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
    with torch.cuda.graph(gp):
        rc, _ = _packed(torch, sslib, cfg, "mel", x, N, p_so, p_ro, CAP, scale, p_out)
    assert rc == 0, sslib.ss_last_error_string()
    with torch.cuda.graph(gs):
        rc, _ = _pool_raw(torch, sslib, cfg, "mel", x, N, s_so, s_ro, CAP, s_sl, POOL, scale, pool_g, s_out)
    assert rc == 0, sslib.ss_last_error_string()
    for k in range(K):
        # packed: N clips of new lengths (odd ones among them) that fill at most CAP rows
        lens = rng.integers(1, 3 * H, N)
        lens[0] |= 1
        so, ro = _offsets(ss, cfg, lens)
        assert int(ro[-1]) <= CAP
        pcm = _random_pcm(torch, int(so[-1]), 14 + k)
        want = torch.full((M * int(ro[-1]),), float("nan"), device="cuda")
        dso, dro = torch.from_numpy(so).cuda(), torch.from_numpy(ro).cuda()
        assert _packed(torch, sslib, cfg, "mel", pcm, N, dso, dro, int(ro[-1]), scale, want)[0] == 0
        x.zero_()
        x[:pcm.numel()] = pcm
        p_so.copy_(dso)
        p_ro.copy_(dro)
        p_out.fill_(float("nan"))
        gp.replay()
        torch.cuda.synchronize()
        assert _same_bits(p_out[:want.numel()], want), k
        assert torch.isnan(p_out[want.numel():]).all()  # rows past the last clip are left alone
        # pool: new hop counts (entries without rows among them) and new slots
        hops = rng.integers(0, 5, N)
        hops[k % N] = 0
        slots = rng.permutation(POOL)[:N].astype(np.int32)
        so = np.zeros(N + 1, np.int64)
        np.cumsum(hops * H, out=so[1:])
        ro = so // H
        pcm = _random_pcm(torch, max(int(so[-1]), 2), 20 + k)
        want = torch.full((M * max(int(ro[-1]), 1),), float("nan"), device="cuda")
        dso, dro, dsl = torch.from_numpy(so).cuda(), torch.from_numpy(ro).cuda(), torch.from_numpy(slots).cuda()
        assert _pool_raw(torch, sslib, cfg, "mel", pcm, N, dso, dro, int(ro[-1]), dsl, POOL, scale, pool_e, want)[0] == 0
        x.zero_()
        x[:pcm.numel()] = pcm
        s_so.copy_(dso)
        s_ro.copy_(dro)
        s_sl.copy_(dsl)
        s_out.fill_(float("nan"))
        gs.replay()
        torch.cuda.synchronize()
        n = M * int(ro[-1])
        assert _same_bits(s_out[:n], want[:n]), k
        assert torch.isnan(s_out[n:]).all()
        assert _same_bits(pool_g, pool_e), k
    assert sslib.ss_config_device_status(cfg.handle) == 0
