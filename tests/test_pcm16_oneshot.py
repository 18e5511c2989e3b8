"""The one-shot MFCC / mfe calls fed signed 16-bit PCM: ss_mfcc_batch_i16 / ss_mfe_batch_i16 / ss_mfcc_packed_i16 / ss_mfe_packed_i16,
their *_device forms, and ``pcm_scale=`` of mfcc, mfcc_batch, mfe, mfe_batch, mfcc_packed, mfe_packed and mfcc_list.

Contract: sample = (float)pcm * scale, scale a power of two, so every output is bit for bit what the float entry point returns on
``pcm.astype(float32) * scale``.  Every comparison below is on the raw bits against that float call; no tolerance appears.

Two notes on the cases:
* The float packed calls reject a clip without a frame (ss_packed_frame_offsets: SS_ERR_SHORT_SIGNAL; on the device such a clip is
  an inconsistent entry), and in contract framing a clip's frame count is floor((n - flen) / step) (processing.rs:101): 480 samples
  are the shortest clip with a frame at the default shape.  The clip list ``[320, 321, 479, 480, 1601, 319, 0, 2000]`` therefore has
  to fail in both forms alike -- that is asserted -- and the bit comparison runs on ``[480, 481, 639, 640, 1601, 2000]``: the same
  pattern moved up to the shortest lengths the float form accepts.  The offsets still take both parities and three clips have
  exactly one frame.
* Which kernel runs is the rule of speechsauce_amd.h: the PCM build of the kernel the float call picks, where it has one.  The float
  packed calls run one of two kernels (the headline varlen build, the generic varlen build) and both have a PCM build, so the packed
  form of the ``fft_length=1024`` case reports the generic kernel's PCM build; the conversion fallback and the float kernel's own
  name are what the equal-length form of that case shows.  At 512 points the GENERIC configurations' equal-length float calls run
  dedicated builds; their generic-kernel runs use the lab library's ss_debug_force_generic, as tests/test_packed.py does.
"""
import ctypes as C
import os

import numpy as np
import pytest

from test_frame_stream_packed_pcm16 import GENERIC as POOL_GENERIC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["ss_mfcc_batch_i16", "ss_mfcc_batch_i16_device", "ss_mfe_batch_i16", "ss_mfe_batch_i16_device",
         "ss_mfcc_packed_i16", "ss_mfcc_packed_i16_device", "ss_mfe_packed_i16", "ss_mfe_packed_i16_device"]
SS_ERR_SHORT_SIGNAL, SS_ERR_ARG, SS_ERR_DEVICE = 1, 3, 6
SCALES = [2.0 ** -15, 1.0]
ISSUE_LENS = [320, 321, 479, 480, 1601, 319, 0, 2000]
LENS = [480, 481, 639, 640, 1601, 2000]  # offsets 0, 480, 961, 1600, 2240, 3841: both parities; 480, 481 and 639 give one frame


def _lens_for(flen, step):
    """LENS for another frame shape: flen + step is the shortest clip with a frame in contract framing (LENS at 320 / 160)"""
    return [flen + step, flen + step + 1, flen + 2 * step - 1, flen + 2 * step, flen + 8 * step + 1, flen + 10 * step + 80]

# the pool test's table (a Hann window with pre-emphasis whose circular wrap reads the clip's last sample, a non-power-of-two
# fft_length, a frame shorter than the hop, a pre-emphasis shift of a whole hop) plus centred frames with reflect padding
GENERIC = {k: v[0] for k, v in POOL_GENERIC.items()}
GENERIC["center_reflect"] = dict(framing="center", pad_mode="reflect", dct_norm="ortho")
GENERIC["center_zeros_hann"] = dict(framing="center", pad_mode="constant", mfcc_window="hann", dct_norm="ortho")
GENERIC["padded"] = dict(framing="padded")
GENERIC["literal"] = dict(framing="literal")


def _cfg(ss, lib=None, **kw):
    from speechsauce_amd import _lib

    return ss.SpeechConfig(_lib.make_params(**kw))


# ---------------------------------------------------------------- CPU ---------------------------------------------------------

def test_the_eight_entries_are_exported_and_declared(sslib):
    header = open(os.path.join(ROOT, "include", "speechsauce_amd.h")).read()
    from speechsauce_amd import _lib

    for n in NAMES:
        assert hasattr(sslib, n), n
        assert n in _lib.PROTOTYPES, n
        assert f"int {n}(const ss_config *cfg, const int16_t *" in header, n
    # a null config: what the float entries answer
    assert sslib.ss_mfcc_batch_i16_device(None, None, 1, 320, 320, 1.0, None, None) == \
        sslib.ss_mfcc_batch_device(None, None, 1, 320, 320, None, None) == SS_ERR_ARG
    assert sslib.ss_mfe_batch_i16_device(None, None, 1, 320, 320, 1.0, None, None, None) == \
        sslib.ss_mfe_batch_device(None, None, 1, 320, 320, None, None, None) == SS_ERR_ARG
    assert sslib.ss_mfcc_packed_i16_device(None, None, 1, None, 1.0, None, 1, None, None) == \
        sslib.ss_mfcc_packed_device(None, None, 1, None, None, 1, None, None) == SS_ERR_ARG
    assert sslib.ss_mfe_packed_i16_device(None, None, 1, None, 1.0, None, 1, None, None, None) == \
        sslib.ss_mfe_packed_device(None, None, 1, None, None, 1, None, None, None) == SS_ERR_ARG
    assert sslib.ss_mfcc_batch_i16(None, None, 1, 320, 320, 1.0, None) == sslib.ss_mfcc_batch(None, None, 1, 320, 320, None) == SS_ERR_ARG
    assert sslib.ss_mfe_batch_i16(None, None, 1, 320, 320, 1.0, None, None) == \
        sslib.ss_mfe_batch(None, None, 1, 320, 320, None, None) == SS_ERR_ARG
    assert sslib.ss_mfcc_packed_i16(None, None, 1, None, 1.0, None) == sslib.ss_mfcc_packed(None, None, 1, None, None) == SS_ERR_ARG
    assert sslib.ss_mfe_packed_i16(None, None, 1, None, 1.0, None, None) == sslib.ss_mfe_packed(None, None, 1, None, None, None) == SS_ERR_ARG


def test_python_pcm_argument_rules(sslib):
    import speechsauce_amd as ss

    p1, p2 = np.zeros(640, np.int16), np.zeros((2, 640), np.int16)
    f1, f2 = np.zeros(640, np.float32), np.zeros((2, 640), np.float32)
    one_d = [(ss.mfcc, ()), (ss.mfe, ()), (ss.mfcc_packed, ([320, 320],)), (ss.mfe_packed, ([320, 320],))]
    two_d = [(ss.mfcc_batch, ()), (ss.mfe_batch, ())]
    for fn, extra in one_d + two_d:
        pcm, flt, wrong = (p1, f1, p2) if (fn, extra) in one_d else (p2, f2, p1)
        with pytest.raises(TypeError):
            fn(flt, *extra, 16000, pcm_scale=2.0 ** -15)  # floats are not PCM
        with pytest.raises(TypeError):
            fn(pcm.astype(np.int32), *extra, 16000, pcm_scale=2.0 ** -15)
        with pytest.raises(TypeError):
            fn(pcm, *extra, 16000)  # int16 without pcm_scale: the dtype rule of the float form
        with pytest.raises(ValueError):
            fn(wrong, *extra, 16000, pcm_scale=2.0 ** -15)  # the number of dimensions
        for bad in (1 / 32767, 3.0, 0, -0.5, 2.0 ** 70, 2.0 ** -65, float("nan"), float("inf")):
            with pytest.raises(ValueError):
                fn(pcm, *extra, 16000, pcm_scale=bad)
    with pytest.raises(TypeError):
        ss.mfcc_list([f1, f1], 16000, pcm_scale=1.0)
    with pytest.raises(TypeError):
        ss.mfcc_list([p1, p1], 16000)
    with pytest.raises(ValueError):
        ss.mfcc_list([p1, p2], 16000, pcm_scale=1.0)
    with pytest.raises(ValueError):
        ss.mfcc_list([p1], 16000, pcm_scale=3.0)
    with pytest.raises(ValueError):
        ss.mfcc_batch([p2, p2], 16000, pcm_scale=2.0 ** -15)  # a list of batches has no PCM form
    with pytest.raises(ValueError):
        ss.mfcc_batch([], 16000, pcm_scale=2.0 ** -15)


# ---------------------------------------------------------------- GPU ---------------------------------------------------------

def _st(torch, stream=None):
    return C.c_void_p(stream if stream is not None else torch.cuda.current_stream().cuda_stream)


def _outs(torch, cfg, rows, fn, fill=float("nan")):
    if fn == "mfcc":
        return (torch.full((rows, cfg.params.num_cepstral), fill, device="cuda"),)
    return torch.full((rows, cfg.params.num_filters), fill, device="cuda"), torch.full((rows,), fill, device="cuda")


def _same_bits(a, b):
    import torch

    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _batch(torch, lib, cfg, fn, ptr, B, n, ld, scale, outs, stream=None):
    """ss_{mfcc,mfe}_batch[_i16]_device on the buffer at `ptr` (scale None: the float form); returns (status, kernel name)."""
    op = [o.data_ptr() for o in outs]
    sc = [] if scale is None else [scale]
    f = getattr(lib, f"ss_{fn}_batch{'' if scale is None else '_i16'}_device")
    rc = f(cfg.handle, ptr, B, n, ld, *sc, *op, _st(torch, stream))
    return rc, lib.ss_last_kernel_name()


def _packed(torch, lib, cfg, fn, ptr, n_clips, dso, dfo, total, scale, outs, stream=None):
    op = [o.data_ptr() for o in outs]
    sc = [] if scale is None else [scale]
    f = getattr(lib, f"ss_{fn}_packed{'' if scale is None else '_i16'}_device")
    rc = f(cfg.handle, ptr, n_clips, dso.data_ptr(), *sc, dfo.data_ptr(), total, *op, _st(torch, stream))
    return rc, lib.ss_last_kernel_name()


def _random_pcm(torch, n, seed):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    return torch.randint(-32768, 32768, (n,), generator=g, device="cuda", dtype=torch.int32).to(torch.int16)


def _three_clips(torch, n, seed):
    """[3, n]: random, all zeros (the zero-handling branch), -32768 / 32767 alternating with zeros between (sign extension, extremes)"""
    x = torch.zeros((3, n), dtype=torch.int16, device="cuda")
    x[0] = _random_pcm(torch, n, seed)
    x[2, 0::4] = -32768
    x[2, 2::4] = 32767
    return x


def _layouts(torch, clips):
    """The three layouts of a [B, n] block inside one flat int16 buffer: yields (label, buffer, first sample, ld)."""
    B, n = clips.shape
    for label, base, ld in (("ld=n", 0, n), ("ld=n+1", 0, n + 1), ("base+1", 1, n)):
        buf = _random_pcm(torch, base + B * ld + 8, 7)  # (the gaps and the tail hold samples that no frame may read)
        for b in range(B):
            buf[base + b * ld: base + b * ld + n] = clips[b]
        yield label, buf, base, ld


def _check_batch(torch, lib, cfg, fn, clips, scale, rows_per_clip):
    """Every layout through the PCM call and the float call on the converted buffer; returns the (float name, PCM name) pairs."""
    B, n = clips.shape
    names = []
    for label, buf, base, ld in _layouts(torch, clips):
        xf = buf.to(torch.float32) * scale
        want, got = _outs(torch, cfg, B * rows_per_clip, fn), _outs(torch, cfg, B * rows_per_clip, fn)
        rc, fname = _batch(torch, lib, cfg, fn, xf.data_ptr() + 4 * base, B, n, ld, None, want)
        assert rc == 0, lib.ss_last_error_string()
        rc, iname = _batch(torch, lib, cfg, fn, buf.data_ptr() + 2 * base, B, n, ld, scale, got)
        assert rc == 0, lib.ss_last_error_string()
        torch.cuda.synchronize()
        for g, w in zip(got, want):
            assert not torch.isnan(w).any(), label
            assert _same_bits(g, w), (label, (g != w).sum().item())
        names.append((fname, iname))
    assert lib.ss_config_device_status(cfg.handle) == 0
    return names


@pytest.mark.gpu
@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("fn", ["mfcc", "mfe"])
def test_headline_batch_form_equals_the_float_call_bit_for_bit(ss, sslib, fn, scale):
    import torch

    cfg = _cfg(ss)
    names = _check_batch(torch, sslib, cfg, fn, _three_clips(torch, 1120, 11), scale, cfg.num_frames(1120))
    for fname, iname in names:
        assert b"c256" in fname and b"c256" in iname and iname != fname, names
        assert iname == fname.replace(b"ss_mfcc_c256<", b"ss_mfcc_c256i<"), names


@pytest.mark.gpu
def test_headline_kernel_with_a_frame_window_and_with_other_banks(ss, sslib):
    """The other PCM builds of the 512-point kernel: the windowed default-bank builds and a bank with run-time tap counts."""
    import torch

    for kw, fns in ((dict(mfcc_window="hann"), ("mfcc", "mfe")), (dict(num_filters=26), ("mfcc",)), (dict(spectrum_exponent=2), ("mfcc",))):
        cfg = _cfg(ss, **kw)
        for fn in fns:
            for fname, iname in _check_batch(torch, sslib, cfg, fn, _three_clips(torch, 1120, 12), 2.0 ** -15, cfg.num_frames(1120)):
                assert fname.startswith(b"ss_mfcc_c256<"), (kw, fname)  # (the float call's own choice: a build of the 512-point kernel)
                assert iname == fname.replace(b"ss_mfcc_c256<", b"ss_mfcc_c256i<"), (kw, fname, iname)


@pytest.mark.gpu
def test_odd_frame_lengths_on_the_headline_kernel(ss, sslib):
    """An odd frame length ends in a half pair (one 16-bit load in the PCM builds).  Shapes whose float call runs the 512-point kernel."""
    import torch

    from test_frame_stream_packed import _sizes

    ran = 0
    for kw in (dict(sample_rate=22050), dict(frame_length=319.5 / 16000), dict(frame_length=320.5 / 16000), dict(frame_length=0.0251)):
        cfg = _cfg(ss, **kw)
        _, flen, step, _ = _sizes(sslib, cfg.params)
        n = flen + 6 * step + 3
        probe = torch.zeros((1, n), device="cuda")
        rc, fname = _batch(torch, sslib, cfg, "mfcc", probe.data_ptr(), 1, n, n, None, _outs(torch, cfg, cfg.num_frames(n), "mfcc"))
        assert rc == 0
        if flen % 2 == 0 or b"ss_mfcc_c256<" not in fname:
            continue
        ran += 1
        for fname, iname in _check_batch(torch, sslib, cfg, "mfcc", _three_clips(torch, n, 13), 2.0 ** -15, cfg.num_frames(n)):
            assert iname == fname.replace(b"ss_mfcc_c256<", b"ss_mfcc_c256i<"), (kw, flen, fname, iname)
    if not ran:
        pytest.skip("no candidate shape with an odd frame length runs the 512-point kernel in the float call")
    assert ran >= 1


def _packed_tables(torch, ss, cfg, lens):
    so, fo = ss._packed_offsets(cfg, np.asarray(lens, np.int64), int(np.sum(lens)), "t")
    return so, fo, torch.from_numpy(so).cuda(), torch.from_numpy(fo).cuda()


def _packed_pcm(torch, so, seed):
    """Packed clips: random, with one clip of silence and the extremes at a clip's ends."""
    pcm = _random_pcm(torch, int(so[-1]) + 2, seed)[: int(so[-1])]
    pcm[so[1]:so[2]] = 0
    pcm[so[2]], pcm[so[3] - 1] = -32768, 32767
    return pcm


def _check_packed(torch, ss, lib, cfg, fn, lens, scale, seed=21):
    so, fo, dso, dfo = _packed_tables(torch, ss, cfg, lens)
    rows = int(fo[-1])
    pcm = _packed_pcm(torch, so, seed)
    xf = pcm.to(torch.float32) * scale
    want, got = _outs(torch, cfg, rows + 2, fn), _outs(torch, cfg, rows + 2, fn)  # two spare rows: left alone
    rc, fname = _packed(torch, lib, cfg, fn, xf.data_ptr(), len(lens), dso, dfo, rows + 2, None, want)
    assert rc == 0, lib.ss_last_error_string()
    rc, iname = _packed(torch, lib, cfg, fn, pcm.data_ptr(), len(lens), dso, dfo, rows + 2, scale, got)
    assert rc == 0, lib.ss_last_error_string()
    torch.cuda.synchronize()
    for g, w in zip(got, want):
        assert not torch.isnan(w[:rows]).any() and torch.isnan(w[rows:]).all()
        assert _same_bits(g, w), (g[:rows] != w[:rows]).sum().item()
    assert lib.ss_config_device_status(cfg.handle) == 0
    return fname, iname, pcm, [g[:rows] for g in got]


@pytest.mark.gpu
@pytest.mark.parametrize("scale", SCALES)
def test_headline_packed_form_device_host_and_list(ss, sslib, scale):
    import torch

    cfg = _cfg(ss)
    fname, iname, pcm, (dev,) = _check_packed(torch, ss, sslib, cfg, "mfcc", LENS, scale)
    assert fname == b"ss_mfcc_c256v<10,exact,bank421,sym>" and iname == b"ss_mfcc_c256vi<10,exact,bank421,sym>"
    fname, iname, _, (dfeat, den) = _check_packed(torch, ss, sslib, cfg, "mfe", LENS, scale)
    assert fname.startswith(b"ss_front_generic_varlen<") and iname == fname.replace(b"_varlen<", b"_varleni<")
    # the Python front: device tensors stay on the device, numpy in gives numpy out (the host form: int16 over the link)
    xf = pcm.to(torch.float32) * scale
    want, fo_w = ss.mfcc_packed(xf, LENS, 16000)
    got, fo_g = ss.mfcc_packed(pcm, LENS, 16000, pcm_scale=scale)
    assert got.is_cuda and torch.equal(fo_g, fo_w) and _same_bits(got, want) and _same_bits(got, dev)
    host, fo_h = ss.mfcc_packed(pcm.cpu().numpy(), LENS, 16000, pcm_scale=scale)
    assert isinstance(host, np.ndarray) and np.array_equal(fo_h, fo_w.cpu().numpy())
    assert np.array_equal(host.view(np.int32), want.cpu().numpy().view(np.int32))
    hf, he, _ = ss.mfe_packed(pcm.cpu().numpy(), LENS, 16000, pcm_scale=scale)
    gf, ge, _ = ss.mfe_packed(pcm, LENS, 16000, pcm_scale=scale)
    assert _same_bits(gf, dfeat) and _same_bits(ge, den)
    assert np.array_equal(hf.view(np.int32), dfeat.cpu().numpy().view(np.int32))
    assert np.array_equal(he.view(np.int32), den.cpu().numpy().view(np.int32))
    so = np.concatenate([[0], np.cumsum(LENS)])
    clips = [pcm[int(so[b]):int(so[b + 1])] for b in range(len(LENS))]
    fo = fo_h.tolist()
    for lst in (ss.mfcc_list(clips, 16000, pcm_scale=scale), ss.mfcc_list([c.cpu().numpy() for c in clips], 16000, pcm_scale=scale)):
        assert len(lst) == len(LENS)
        for b, f in enumerate(lst):
            f = f.cpu().numpy() if hasattr(f, "is_cuda") else f
            assert np.array_equal(f.view(np.int32), host[fo[b]:fo[b + 1]].view(np.int32)), b
    # the list with its two frameless clips: both forms refuse it alike, on the host before anything runs
    n_all = int(np.sum(ISSUE_LENS))
    so_all = np.concatenate([[0], np.cumsum(ISSUE_LENS)]).astype(np.int64)
    p_all, out = np.zeros(n_all, np.int16), np.full((64, 13), 7.0, np.float32)
    rc_i = sslib.ss_mfcc_packed_i16(cfg.handle, p_all.ctypes.data, len(ISSUE_LENS), so_all.ctypes.data, scale, out.ctypes.data)
    rc_f = sslib.ss_mfcc_packed(cfg.handle, p_all.astype(np.float32).ctypes.data, len(ISSUE_LENS), so_all.ctypes.data, out.ctypes.data)
    assert rc_i == rc_f == SS_ERR_SHORT_SIGNAL and np.all(out == 7.0)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(GENERIC))
def test_generic_kernel_batch_and_packed_forms(ss, sslib, sslab, name):
    import torch

    from speechsauce_amd import _lib
    from test_frame_stream_packed import _sizes

    kw = GENERIC[name]
    scale = 2.0 ** -15
    cfg = _cfg(ss, **kw)
    _, flen, step, _ = _sizes(sslib, cfg.params)
    # packed form on the product library: every one of these configurations runs the generic varlen build
    lens = _lens_for(flen, step)
    for fn in ("mfcc", "mfe"):
        fname, iname, _, _ = _check_packed(torch, ss, sslib, cfg, fn, lens, scale, seed=31)
        assert fname.startswith(b"ss_front_generic_varlen<") and iname == fname.replace(b"_varlen<", b"_varleni<"), (fname, iname)
    if name == "chirpz":
        assert iname.endswith(b",chirpz>")
    # batch form, 2 clips at an odd ld, on the generic kernel (forced where the float call would run a dedicated build)
    n = flen + 5 * step + 1
    clips = _three_clips(torch, n, 32)[[0, 2]]
    with _lib.use_library(sslab):
        sslab.ss_debug_force_generic(1)
        try:
            lcfg = _cfg(ss, **kw)
            for fn in ("mfcc", "mfe"):
                B, ld = 2, n + 1
                buf = _random_pcm(torch, B * ld + 4, 33)
                for b in range(B):
                    buf[b * ld: b * ld + n] = clips[b]
                xf = buf.to(torch.float32) * scale
                T = lcfg.num_frames(n)
                want, got = _outs(torch, lcfg, B * T, fn), _outs(torch, lcfg, B * T, fn)
                rc, fname = _batch(torch, sslab, lcfg, fn, xf.data_ptr(), B, n, ld, None, want)
                assert rc == 0, sslab.ss_last_error_string()
                rc, iname = _batch(torch, sslab, lcfg, fn, buf.data_ptr(), B, n, ld, scale, got)
                assert rc == 0, sslab.ss_last_error_string()
                torch.cuda.synchronize()
                assert fname.startswith(b"ss_front_generic<") and iname == fname.replace(b"ss_front_generic<", b"ss_front_generic_i16<")
                for g, w in zip(got, want):
                    assert not torch.isnan(w).any() and _same_bits(g, w), (fn, (g != w).sum().item())
        finally:
            sslab.ss_debug_force_generic(0)
    # and on the product library, whatever kernel the float call picks there: the same bits
    _check_batch(torch, sslib, cfg, "mfcc", clips, scale, cfg.num_frames(n))


@pytest.mark.gpu
def test_fallback_runs_the_float_kernel_behind_one_conversion(ss, sslib):
    import torch

    cfg = _cfg(ss, fft_points=1024)
    n = 1120
    for fn in ("mfcc", "mfe"):
        for fname, iname in _check_batch(torch, sslib, cfg, fn, _three_clips(torch, n, 41), 2.0 ** -15, cfg.num_frames(n)):
            assert not fname.startswith(b"ss_front_generic") and iname == fname, (fname, iname)  # a dedicated kernel without a PCM build
    # packed: the float call runs the generic varlen build, which has a PCM build (see the module docstring)
    fname, iname, _, _ = _check_packed(torch, ss, sslib, cfg, "mfcc", LENS, 2.0 ** -15, seed=42)
    assert fname.startswith(b"ss_front_generic_varlen<") and iname == fname.replace(b"_varlen<", b"_varleni<")
    # the 512-point sub-shapes left on the fallback: fused pre-emphasis, centred frames
    for kw in (dict(preemph_coef=0.97), dict(framing="center", dct_norm="ortho")):
        c2 = _cfg(ss, **kw)
        for fname, iname in _check_batch(torch, sslib, c2, "mfcc", _three_clips(torch, n, 43), 1.0, c2.num_frames(n)):
            assert not fname.startswith(b"ss_front_generic") and iname == fname, (kw, fname, iname)


@pytest.mark.gpu
def test_host_pipeline_moves_int16_and_equals_the_device_form(ss, sslib):
    import torch

    cfg = _cfg(ss)
    scale = 2.0 ** -15
    for B, n in ((1, 16000), (600, 16000)):  # the mapped small-call path; 19 MB of int16: two chunks
        T = cfg.num_frames(n)
        pcm = _random_pcm(torch, B * n, 50 + B).view(B, n)
        (dev,) = _outs(torch, cfg, B * T, "mfcc")
        rc, _ = _batch(torch, sslib, cfg, "mfcc", pcm.data_ptr(), B, n, n, scale, (dev,))
        assert rc == 0
        torch.cuda.synchronize()
        h = pcm.cpu().numpy()
        out = np.full((B * T, 13), np.nan, np.float32)
        assert sslib.ss_mfcc_batch_i16(cfg.handle, h.ctypes.data, B, n, n, scale, out.ctypes.data) == 0, sslib.ss_last_error_string()
        assert np.array_equal(out.view(np.int32), dev.cpu().numpy().view(np.int32)), B
        if B == 1:
            feat, en = np.empty((T, 40), np.float32), np.empty(T, np.float32)
            assert sslib.ss_mfe_batch_i16(cfg.handle, h.ctypes.data, B, n, n, scale, feat.ctypes.data, en.ctypes.data) == 0
            wf, we = ss.mfe(torch.from_numpy(h[0]).cuda().float() * scale, 16000)
            assert np.array_equal(feat.view(np.int32), wf.cpu().numpy().view(np.int32))
            assert np.array_equal(en.view(np.int32), we.cpu().numpy().view(np.int32))
            got = ss.mfcc(h[0], 16000, pcm_scale=scale)
            assert isinstance(got, np.ndarray) and np.array_equal(got.view(np.int32), out.view(np.int32))
            gb = ss.mfcc_batch(pcm, 16000, pcm_scale=scale)
            assert gb.is_cuda and _same_bits(gb.reshape(-1, 13), dev)
            fb, eb = ss.mfe_batch(pcm, 16000, pcm_scale=scale)
            assert _same_bits(fb[0], wf) and _same_bits(eb[0], we)


@pytest.mark.gpu
def test_bad_arguments_are_rejected_before_anything_runs(ss, sslib):
    import torch

    cfg = _cfg(ss)
    n, B = 1120, 2
    T = cfg.num_frames(n)
    pcm = _random_pcm(torch, B * n, 60)
    xf = pcm.to(torch.float32)
    rc, fname = _batch(torch, sslib, cfg, "mfcc", xf.data_ptr(), B, n, n, None, _outs(torch, cfg, B * T, "mfcc"))
    assert rc == 0  # a float call first: the name a rejected call must leave in place
    so, fo, dso, dfo = _packed_tables(torch, ss, cfg, [n, n])
    for fn in ("mfcc", "mfe"):
        outs = _outs(torch, cfg, B * T, fn, fill=12345.0)
        for scale, ld, ptr in ((3.0, n, pcm.data_ptr()), (0.0, n, pcm.data_ptr()), (2.0 ** -15, n - 1, pcm.data_ptr()), (2.0 ** -15, n, None),
                               (float("nan"), n, pcm.data_ptr()), (2.0 ** 65, n, pcm.data_ptr())):
            rc, name = _batch(torch, sslib, cfg, fn, ptr, B, n, ld, scale, outs)
            assert rc == SS_ERR_ARG and name == fname, (scale, ld, ptr)
        for scale, ptr in ((3.0, pcm.data_ptr()), (0.0, pcm.data_ptr()), (2.0 ** -15, None)):
            rc, name = _packed(torch, sslib, cfg, fn, ptr, 2, dso, dfo, B * T, scale, outs)
            assert rc == SS_ERR_ARG and name == fname, (scale, ptr)
        torch.cuda.synchronize()
        assert all(bool((o == 12345.0).all()) for o in outs)
    h, out = pcm.cpu().numpy(), np.full((B * T, 13), 12345.0, np.float32)
    for scale, ld, ptr in ((3.0, n, h.ctypes.data), (0.0, n, h.ctypes.data), (1.0, n - 1, h.ctypes.data), (1.0, n, None)):
        assert sslib.ss_mfcc_batch_i16(cfg.handle, ptr, B, n, ld, scale, out.ctypes.data) == SS_ERR_ARG
    assert sslib.ss_mfcc_packed_i16(cfg.handle, h.ctypes.data, 2, so.ctypes.data, 3.0, out.ctypes.data) == SS_ERR_ARG
    assert b"scale" in sslib.ss_last_error_string()
    assert np.all(out == 12345.0)
    for s in (2.0 ** 64, 2.0 ** -64):  # the ends of the range are in it
        rc, _ = _batch(torch, sslib, cfg, "mfcc", pcm.data_ptr(), B, n, n, s, _outs(torch, cfg, B * T, "mfcc"))
        assert rc == 0
    # an empty batch is the float form's: nothing to do, no buffers needed
    assert sslib.ss_mfcc_batch_i16_device(cfg.handle, None, 0, n, n, 1.0, None, None) == 0
    assert sslib.ss_mfcc_packed_i16_device(cfg.handle, None, 0, None, 1.0, None, 0, None, None) == 0
    torch.cuda.synchronize()
    assert sslib.ss_config_device_status(cfg.handle) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", ["headline", "generic"])
def test_bad_packed_tables_are_contained(ss, sslib, kernel):
    """tests/test_packed.py's bad-table test on ss_mfcc_packed_i16_device: the error word, the guard bands, the clips that stay."""
    import torch

    kw = {} if kernel == "headline" else dict(preemph_coef=0.97, preemph_shift=1)
    scale = 2.0 ** -15
    lens = np.array([1601, 800, 481, 1200], dtype=np.int64)
    cfg = _cfg(ss, **kw)  # a fresh config: its error word is its own
    so, fo, dso, dfo = _packed_tables(torch, ss, cfg, lens)
    pcm = _random_pcm(torch, int(so[-1]), 70)
    xf = pcm.to(torch.float32) * scale
    rows = int(fo[-1])
    good = torch.full((rows, 13), float("nan"), device="cuda")
    rc, fname = _packed(torch, sslib, cfg, "mfcc", xf.data_ptr(), 4, dso, dfo, rows, None, (good,))
    assert rc == 0
    torch.cuda.synchronize()
    assert sslib.ss_config_device_status(cfg.handle) == 0
    good = good.cpu().numpy()
    SENT, pad = 12345.0, 64

    def run(fo_bad, total):
        block = torch.full(((total + 2 * pad) * 13,), SENT, device="cuda")
        d = torch.from_numpy(np.asarray(fo_bad, dtype=np.int64)).cuda()
        rc, iname = _packed(torch, sslib, cfg, "mfcc", pcm.data_ptr(), 4, dso, d, total, scale, (block[pad * 13:],))
        assert rc == 0  # the check is the kernel's: asynchronous
        assert iname != fname and (b"c256vi" in iname if kernel == "headline" else b"ss_front_generic_varleni" in iname)
        torch.cuda.synchronize()
        return block.cpu().numpy()

    # clip 1 claims one row too many; the clips behind it start one row late but are consistent in themselves
    bad = fo.copy()
    bad[2:] += 1
    blk = run(bad, int(bad[-1]))
    assert sslib.ss_config_device_status(cfg.handle) == SS_ERR_DEVICE  # read and cleared
    assert sslib.ss_config_device_status(cfg.handle) == 0
    assert np.all(blk[:pad * 13] == SENT) and np.all(blk[-pad * 13:] == SENT)
    body = blk[pad * 13:-pad * 13].reshape(-1, 13)
    assert np.array_equal(body[:fo[1]].view(np.int32), good[:fo[1]].view(np.int32))  # clip 0
    assert np.all(body[bad[1]:bad[2]] == SENT)                                        # clip 1 skipped
    for b in (2, 3):                                                                  # clips 2, 3: one row later
        assert np.array_equal(body[bad[b]:bad[b + 1]].view(np.int32), good[fo[b]:fo[b + 1]].view(np.int32)), b
    # total_frames smaller than the clips' rows: the last clip is skipped; the next call on the config reports the error
    blk = run(fo, rows - 3)
    nxt = torch.empty((rows, 13), device="cuda")
    rc, _ = _packed(torch, sslib, cfg, "mfcc", pcm.data_ptr(), 4, dso, dfo, rows, scale, (nxt,))
    assert rc == SS_ERR_DEVICE  # from the next call, which launches nothing
    assert sslib.ss_config_device_status(cfg.handle) == 0  # (cleared by the call that reported it)
    assert np.all(blk[:pad * 13] == SENT) and np.all(blk[-pad * 13:] == SENT)
    body = blk[pad * 13:-pad * 13].reshape(-1, 13)
    assert np.array_equal(body[:fo[3]].view(np.int32), good[:fo[3]].view(np.int32))
    assert np.all(body[fo[3]:] == SENT)


@pytest.mark.gpu
def test_graph_capture_replays_over_new_samples_and_new_tables(ss, sslib):
    import torch

    cfg = _cfg(ss)
    scale = 2.0 ** -15
    table_sets = [[1601, 777, 641, 3201, 2000], [480, 3201, 1601, 2000, 1098], [2000, 2000, 639, 481, 3201], [999, 1601, 3201, 641, 1778]]
    n = max(sum(t) for t in table_sets)
    tabs = [_packed_tables(torch, ss, cfg, t) for t in table_sets]
    total = max(int(t[1][-1]) for t in tabs)
    dso, dfo = tabs[0][2].clone(), tabs[0][3].clone()
    pcm = _random_pcm(torch, n, 80)
    out = torch.full((total, 13), 5.0, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):  # warm-up off the capture
        rc, _ = _packed(torch, sslib, cfg, "mfcc", pcm.data_ptr(), 5, dso, dfo, total, scale, (out,), stream=s.cuda_stream)
        assert rc == 0
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        rc, name = _packed(torch, sslib, cfg, "mfcc", pcm.data_ptr(), 5, dso, dfo, total, scale, (out,),
                           stream=torch.cuda.current_stream().cuda_stream)
    assert rc == 0 and name == b"ss_mfcc_c256vi<10,exact,bank421,sym>"
    for k in (1, 2, 3):
        pcm.copy_(_random_pcm(torch, n, 80 + k))
        dso.copy_(tabs[k][2])
        dfo.copy_(tabs[k][3])
        out.fill_(5.0)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        eager = torch.full_like(out, 5.0)
        rc, _ = _packed(torch, sslib, cfg, "mfcc", pcm.data_ptr(), 5, dso, dfo, total, scale, (eager,))
        assert rc == 0
        xf = pcm.to(torch.float32) * scale
        want = torch.full_like(out, 5.0)
        rc, _ = _packed(torch, sslib, cfg, "mfcc", xf.data_ptr(), 5, dso, dfo, total, None, (want,))
        assert rc == 0
        torch.cuda.synchronize()
        rows = int(tabs[k][1][-1])
        assert _same_bits(out, eager) and _same_bits(out, want), k
        assert not (out[:rows] == 5.0).all() and bool((out[rows:] == 5.0).all()), k
    cfg.device_status()
