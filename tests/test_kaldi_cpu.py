"""The Kaldi-compatible front end (ss_kaldi_* in include/speechsauce_amd.h), host side: no device.

This file holds the numpy restatement of the header's specification -- ``ref_window``, ``ref_bank``, ``ref_dct``, ``ref_fbank``,
``ref_mfcc``, in f64 unless asked otherwise -- which tests/test_kaldi.py imports as the reference of the GPU tests, and checks the
host-only entry points against it: defaults, sizes, frame counts, packed offsets, the three tables, every validation rule, the exports
and the mirrors.  The last test records that the specification is well-posed in f32: the restatement run in f32 against itself in f64."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "speechsauce_amd.h")
EPS = float(np.float32(1.1920929e-7))
SS_OK, SS_ERR_SHORT_SIGNAL, SS_ERR_BAD_CONFIG, SS_ERR_ARG, SS_ERR_HIP, SS_ERR_UNSUPPORTED, SS_ERR_DEVICE = range(7)
WINDOWS = ("povey", "hanning", "hamming", "rectangular", "blackman")

# torchaudio.compliance.kaldi's defaults
DEFAULTS = dict(sample_rate=16000, frame_length_ms=25.0, frame_shift_ms=10.0, num_mel_bins=23, num_ceps=13, low_freq=20.0, high_freq=0.0,
                preemph_coef=0.97, cepstral_lifter=22.0, window_type="povey", blackman_coeff=0.42, remove_dc_offset=1, use_power=1,
                use_energy=0, raw_energy=1, energy_floor=1.0, input_scale=1.0, dither=0.0)


def kp(**kw):
    """The parameters of one configuration as a dict (names of ss_kaldi_params, window_type by name)."""
    bad = set(kw) - set(DEFAULTS)
    assert not bad, bad
    return {**DEFAULTS, **kw}


# ---- the specification, restated ------------------------------------------------------------------------------------------

def ref_sizes(p):
    flen = int(p["sample_rate"] * 0.001 * float(np.float32(p["frame_length_ms"])))
    shift = int(p["sample_rate"] * 0.001 * float(np.float32(p["frame_shift_ms"])))
    padded = 1
    while padded < flen:
        padded *= 2
    return flen, shift, padded


def ref_num_frames(p, n):
    flen, shift, _ = ref_sizes(p)
    return 0 if n < flen else 1 + (n - flen) // shift


def ref_window(p):
    flen = ref_sizes(p)[0]
    a = 2.0 * np.pi * np.arange(flen, dtype=np.float64) / (flen - 1)
    kind, b = p["window_type"], float(np.float32(p["blackman_coeff"]))
    if kind == "povey":
        return (0.5 - 0.5 * np.cos(a)) ** 0.85
    if kind == "hanning":
        return 0.5 - 0.5 * np.cos(a)
    if kind == "hamming":
        return 0.54 - 0.46 * np.cos(a)
    if kind == "rectangular":
        return np.ones(flen)
    assert kind == "blackman"
    return b - 0.5 * np.cos(a) + (0.5 - b) * np.cos(2.0 * a)


def _mel(f):
    return 1127.0 * np.log(1.0 + np.asarray(f, np.float64) / 700.0)


def ref_bank(p):
    """[num_mel_bins x N/2] dense, f64"""
    sr, M = float(p["sample_rate"]), int(p["num_mel_bins"])
    N = ref_sizes(p)[2]
    low, high = float(np.float32(p["low_freq"])), float(np.float32(p["high_freq"]))
    if high <= 0.0:
        high = 0.5 * sr + high
    mlow = float(_mel(low))
    delta = (float(_mel(high)) - mlow) / (M + 1)
    mu = _mel(np.arange(N // 2) * sr / N)
    bank = np.zeros((M, N // 2))
    for b in range(M):
        left, centre, right = mlow + b * delta, mlow + (b + 1) * delta, mlow + (b + 2) * delta
        inside = (mu > left) & (mu < right)
        up = (mu - left) / (centre - left)
        down = (right - mu) / (right - centre)
        bank[b] = np.where(inside, np.where(mu <= centre, up, down), 0.0)
    return bank


def ref_dct(p):
    """[num_ceps x num_mel_bins], the lifter folded in, f64"""
    M, Cc, Q = int(p["num_mel_bins"]), int(p["num_ceps"]), float(np.float32(p["cepstral_lifter"]))
    k = np.arange(Cc, dtype=np.float64)[:, None]
    b = np.arange(M, dtype=np.float64)[None, :]
    D = np.sqrt(2.0 / M) * np.cos(np.pi / M * (b + 0.5) * k)
    D[0, :] = np.sqrt(1.0 / M)
    lift = np.ones(Cc) if Q == 0.0 else 1.0 + 0.5 * Q * np.sin(np.pi * np.arange(Cc) / Q)
    return D * lift[:, None]


def ref_fbank(x, p, dtype=np.float64):
    """x [L] -> (fbank [T x num_mel_bins], log_energy [T]) in `dtype` arithmetic (tables formed in f64, rounded once to f32)."""
    flen, shift, N = ref_sizes(p)
    T = ref_num_frames(p, len(x))
    dt = np.dtype(dtype).type
    w = ref_window(p).astype(np.float32).astype(dtype)
    bank = ref_bank(p).astype(np.float32).astype(dtype)
    x = np.asarray(x, np.float32).astype(dtype)
    s = np.stack([x[t * shift:t * shift + flen] for t in range(T)]) if T else np.zeros((0, flen), dtype)
    scale = dt(np.float32(p["input_scale"]))
    if scale != 1:
        s = s * scale
    if p["remove_dc_offset"]:
        s = s - (s.sum(axis=1, dtype=dtype) / dt(flen))[:, None]
    energy = (s * s).sum(axis=1, dtype=dtype)
    c = dt(np.float32(p["preemph_coef"]))
    y = s
    if c != 0:
        prev = np.concatenate([s[:, :1], s[:, :-1]], axis=1)
        y = s - c * prev
    y = y * w[None, :]
    if not p["raw_energy"]:
        energy = (y * y).sum(axis=1, dtype=dtype)
    pad = np.zeros((T, N), dtype)
    pad[:, :flen] = y
    X = np.fft.rfft(pad.astype(np.float64), axis=1)[:, :N // 2]  # (numpy transforms in f64: the spectrum is rounded to `dtype` next)
    P = (X.real.astype(dtype) ** 2 + X.imag.astype(dtype) ** 2)
    if not p["use_power"]:
        P = np.sqrt(P)
    e = (P @ bank.T).astype(dtype)
    fb = np.log(np.maximum(e, dt(EPS)))
    le = np.log(np.maximum(energy, dt(EPS)))
    floor = float(np.float32(p["energy_floor"]))
    if floor > 0.0:
        le = np.maximum(le, dt(np.log(floor)))
    return fb.astype(dtype), le.astype(dtype)


def ref_mfcc(x, p, dtype=np.float64):
    """x [L] -> [T x num_ceps]"""
    fb, le = ref_fbank(x, p, dtype)
    D = ref_dct(p).astype(np.float32).astype(dtype)
    c = (fb @ D.T).astype(dtype)
    if p["use_energy"]:
        c[:, 0] = le
    return c


def block_metric(got, want):
    return float(np.abs(np.asarray(got, np.float64) - np.asarray(want, np.float64)).max() / np.abs(want).max())


# ---- the library's side ---------------------------------------------------------------------------------------------------

def make_kaldi_params(sslib, **kw):
    from speechsauce_amd._lib import KALDI_WINDOW, SsKaldiParams

    p = kp(**kw)
    sp = SsKaldiParams()
    assert sslib.ss_kaldi_params_default(C.byref(sp), int(p["sample_rate"])) == SS_OK
    for name, value in p.items():
        if name == "sample_rate":
            continue
        setattr(sp, name, KALDI_WINDOW[value] if name == "window_type" else value)
    return sp


def lib_sizes(sslib, sp):
    a, b, c = C.c_size_t(), C.c_size_t(), C.c_size_t()
    rc = sslib.ss_kaldi_sizes(C.byref(sp), C.byref(a), C.byref(b), C.byref(c))
    return rc, (a.value, b.value, c.value)


def test_defaults_are_torchaudios(sslib):
    from speechsauce_amd._lib import KALDI_WINDOW, SsKaldiParams

    sp = SsKaldiParams()
    assert sslib.ss_kaldi_params_default(C.byref(sp), 16000) == SS_OK
    assert sp.struct_size == C.sizeof(SsKaldiParams) == 4 * len(SsKaldiParams._fields_) == 76
    for name, value in DEFAULTS.items():
        got = getattr(sp, name)
        want = KALDI_WINDOW[value] if name == "window_type" else value
        assert got == pytest.approx(want, rel=1e-7), name
    assert sslib.ss_kaldi_params_default(None, 16000) == SS_ERR_ARG
    assert sslib.ss_kaldi_params_validate(C.byref(sp)) == SS_OK


# the frame lengths of tests/test_kaldi_builds.py: the smallest and the largest of every NE class of the kernel (live input pairs
# 10 / 13 / 16 for flen <= 320 / 416 / 512) beside the everyday ones.  id -> (sample_rate, frame_length_ms, flen, shift, NE)
FRAME_LENGTHS = {"257": (16000, 16.0625, 257, 160, 10), "320": (16000, 20.0, 320, 160, 10), "321": (16000, 20.0625, 321, 160, 13),
                 "400": (16000, 25.0, 400, 160, 13), "416": (16000, 26.0, 416, 160, 13), "417": (16000, 26.0625, 417, 160, 16),
                 "511": (16000, 31.9375, 511, 160, 16), "512": (16000, 32.0, 512, 160, 16), "275": (11025, 25.0, 275, 110, 10)}


@pytest.mark.parametrize("sr,fl,fs,want", [(16000, 25.0, 10.0, (400, 160, 512)), (16000, 20.0, 10.0, (320, 160, 512)),
                                           (16000, 32.0, 10.0, (512, 160, 512)), (11025, 25.0, 10.0, (275, 110, 512)),
                                           (16000, 25.0, 10.0625, (400, 161, 512))] +
                         [(sr, fl, 10.0, (flen, shift, 512)) for sr, fl, flen, shift, _ in FRAME_LENGTHS.values()])
def test_sizes(sslib, sr, fl, fs, want):
    sp = make_kaldi_params(sslib, sample_rate=sr, frame_length_ms=fl, frame_shift_ms=fs)
    assert lib_sizes(sslib, sp) == (SS_OK, want)
    assert ref_sizes(kp(sample_rate=sr, frame_length_ms=fl, frame_shift_ms=fs)) == want


@pytest.mark.parametrize("sr", [8000, 44100])
def test_other_padded_sizes_are_unsupported(sslib, sr):
    sp = make_kaldi_params(sslib, sample_rate=sr)
    assert lib_sizes(sslib, sp)[0] == SS_ERR_UNSUPPORTED
    assert sslib.ss_kaldi_params_validate(C.byref(sp)) == SS_ERR_UNSUPPORTED


@pytest.mark.parametrize("cfg", [dict(), dict(sample_rate=11025), dict(frame_shift_ms=10.0625), dict(frame_length_ms=20.0, frame_shift_ms=30.0)])
def test_frame_counts_and_packed_offsets(sslib, cfg):
    p = kp(**cfg)
    sp = make_kaldi_params(sslib, **cfg)
    flen, shift, _ = ref_sizes(p)
    t = C.c_size_t()
    assert sslib.ss_kaldi_num_frames(C.byref(sp), flen - 1, C.byref(t)) == SS_ERR_SHORT_SIGNAL
    for n, want in ((flen, 1), (flen + shift - 1, 1), (flen + shift, 2), (flen + 16 * shift + 3, 17)):
        assert sslib.ss_kaldi_num_frames(C.byref(sp), n, C.byref(t)) == SS_OK
        assert t.value == want == ref_num_frames(p, n)
    lens = [flen, flen + shift, flen + 5 * shift - 1, flen + 1, 3 * flen + 7]
    so = np.zeros(len(lens) + 1, np.int64)
    so[1:] = np.cumsum(lens)
    fo = np.full_like(so, -1)
    assert sslib.ss_kaldi_packed_frame_offsets(C.byref(sp), len(lens), so.ctypes.data, fo.ctypes.data) == SS_OK
    want = [0]
    for n in lens:
        want.append(want[-1] + ref_num_frames(p, n))
    assert fo.tolist() == want
    # bad tables: a first offset that is not 0, a decreasing pair; a clip shorter than one frame is the short-signal status
    bad = so.copy()
    bad[0] = 1
    assert sslib.ss_kaldi_packed_frame_offsets(C.byref(sp), len(lens), bad.ctypes.data, fo.ctypes.data) == SS_ERR_ARG
    bad = so.copy()
    bad[2] = bad[1] - 1
    assert sslib.ss_kaldi_packed_frame_offsets(C.byref(sp), len(lens), bad.ctypes.data, fo.ctypes.data) == SS_ERR_ARG
    short = np.array([0, flen, 2 * flen - 1], np.int64)
    assert sslib.ss_kaldi_packed_frame_offsets(C.byref(sp), 2, short.ctypes.data, fo.ctypes.data) == SS_ERR_SHORT_SIGNAL
    assert sslib.ss_kaldi_packed_frame_offsets(C.byref(sp), 2, None, fo.ctypes.data) == SS_ERR_ARG


@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("sr,fl", [(16000, 25.0), (11025, 25.0), (16000, 32.0)])
def test_window_table(sslib, window, sr, fl):
    cfg = dict(sample_rate=sr, frame_length_ms=fl, window_type=window, blackman_coeff=0.42 if sr == 16000 else 0.38)
    sp = make_kaldi_params(sslib, **cfg)
    want = ref_window(kp(**cfg))
    got = np.full(len(want), np.nan, np.float32)
    assert sslib.ss_kaldi_window(C.byref(sp), got.ctypes.data) == SS_OK
    assert np.abs(got.astype(np.float64) - want).max() <= 2.0 ** -23


BANKS = [(16000, 80, 20.0, 0.0), (16000, 23, 20.0, 0.0), (11025, 40, 20.0, 0.0), (16000, 80, 0.0, -400.0)]


def lib_bank(sslib, sp):
    got = np.full((sp.num_mel_bins, 256), np.nan, np.float32)
    assert sslib.ss_kaldi_mel_bank(C.byref(sp), got.ctypes.data) == SS_OK
    return got


@pytest.mark.parametrize("sr,M,low,high", BANKS)
def test_mel_bank_table(sslib, sr, M, low, high):
    cfg = dict(sample_rate=sr, num_mel_bins=M, low_freq=low, high_freq=high)
    got = lib_bank(sslib, make_kaldi_params(sslib, **cfg))
    want = ref_bank(kp(**cfg))
    assert np.abs(got.astype(np.float64) - want).max() <= 1e-6
    assert ((got != 0) == (want.astype(np.float32) != 0)).all()


def test_mel_bank_shapes_of_record(sslib):
    b80 = lib_bank(sslib, make_kaldi_params(sslib, num_mel_bins=80))
    taps = (b80 != 0).sum(axis=1)
    assert int(taps.sum()) == 501 and taps.min() == 1 and taps.max() == 16
    b23 = lib_bank(sslib, make_kaldi_params(sslib, num_mel_bins=23))
    assert int((b23 != 0).sum(axis=1).max()) == 52
    sp = make_kaldi_params(sslib, num_mel_bins=128, low_freq=0.0, high_freq=0.0)
    assert sslib.ss_kaldi_mel_bank(C.byref(sp), np.zeros((128, 256), np.float32).ctypes.data) == SS_ERR_UNSUPPORTED


@pytest.mark.parametrize("M,Cc", [(23, 13), (80, 20), (40, 32)])
@pytest.mark.parametrize("lifter", [22.0, 0.0])
def test_dct_table(sslib, M, Cc, lifter):
    cfg = dict(num_mel_bins=M, num_ceps=Cc, cepstral_lifter=lifter)
    sp = make_kaldi_params(sslib, **cfg)
    got = np.full((Cc, M), np.nan, np.float32)
    assert sslib.ss_kaldi_dct(C.byref(sp), got.ctypes.data) == SS_OK
    assert np.abs(got.astype(np.float64) - ref_dct(kp(**cfg))).max() <= 1e-6


@pytest.mark.parametrize("cfg,want", [
    (dict(num_mel_bins=2), SS_ERR_BAD_CONFIG),
    (dict(low_freq=-1.0), SS_ERR_BAD_CONFIG),
    (dict(low_freq=4000.0, high_freq=4000.0), SS_ERR_BAD_CONFIG),       # high <= low
    (dict(low_freq=20.0, high_freq=-7990.0), SS_ERR_BAD_CONFIG),         # resolved high = 10 <= low
    (dict(high_freq=8000.5), SS_ERR_BAD_CONFIG),                         # above sample_rate / 2
    (dict(frame_length_ms=0.1), SS_ERR_BAD_CONFIG),                      # flen = 1 < 2
    (dict(frame_shift_ms=0.05), SS_ERR_BAD_CONFIG),                      # shift = 0 < 1
    (dict(num_mel_bins=23, num_ceps=24), SS_ERR_BAD_CONFIG),
    (dict(input_scale=0.0), SS_ERR_BAD_CONFIG),
    (dict(input_scale=-1.0), SS_ERR_BAD_CONFIG),
    (dict(input_scale=float("inf")), SS_ERR_BAD_CONFIG),
    (dict(input_scale=float("nan")), SS_ERR_BAD_CONFIG),
    (dict(energy_floor=-0.5), SS_ERR_BAD_CONFIG),
    (dict(frame_length_ms=16.0), SS_ERR_UNSUPPORTED),                    # 256 samples pad to 256
    (dict(frame_length_ms=32.0625), SS_ERR_UNSUPPORTED),                 # 513 samples pad to 1024
    (dict(num_mel_bins=81), SS_ERR_UNSUPPORTED),
    (dict(num_mel_bins=80, num_ceps=33), SS_ERR_UNSUPPORTED),
    (dict(dither=1.0), SS_ERR_UNSUPPORTED),
    (dict(frame_shift_ms=40.0), SS_OK),                                  # a shift beyond the frame length is fine
    (dict(num_mel_bins=3, num_ceps=3), SS_OK),
    (dict(energy_floor=0.0), SS_OK),
])
def test_validation_rules(sslib, cfg, want):
    sp = make_kaldi_params(sslib, **cfg)
    assert sslib.ss_kaldi_params_validate(C.byref(sp)) == want, sslib.ss_last_error_string()
    h = C.c_void_p()
    if want != SS_OK:  # create refuses the same parameters with the same status, before it looks for a device
        assert sslib.ss_kaldi_config_create(C.byref(sp), C.byref(h)) == want and not h.value


def test_struct_size_is_checked(sslib):
    sp = make_kaldi_params(sslib)
    sp.struct_size -= 4
    assert sslib.ss_kaldi_params_validate(C.byref(sp)) == SS_ERR_ARG
    assert sslib.ss_kaldi_params_validate(None) == SS_ERR_ARG


NEW_SYMBOLS = ["ss_kaldi_params_default", "ss_kaldi_params_validate", "ss_kaldi_sizes", "ss_kaldi_num_frames", "ss_kaldi_packed_frame_offsets",
               "ss_kaldi_window", "ss_kaldi_mel_bank", "ss_kaldi_dct", "ss_kaldi_config_create", "ss_kaldi_config_destroy",
               "ss_kaldi_config_params", "ss_kaldi_config_device_status", "ss_kaldi_fbank_device", "ss_kaldi_fbank", "ss_kaldi_mfcc_device",
               "ss_kaldi_mfcc", "ss_kaldi_fbank_packed_device", "ss_kaldi_fbank_packed", "ss_kaldi_mfcc_packed_device", "ss_kaldi_mfcc_packed"]


def test_exports_and_mirrors(sslib):
    import subprocess

    from speechsauce_amd import _lib

    header = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(ss_kaldi_[a-z0-9_]+)\s*\(", header))
    assert declared == set(NEW_SYMBOLS)
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name in NEW_SYMBOLS:
        assert name in exported, f"{name} is not exported"
        assert name in _lib.PROTOTYPES, f"{name} has no ctypes prototype"
    assert sslib.ss_abi_version() == 7 == _lib.ABI_VERSION
    assert "#define SS_ABI_VERSION 7" in open(HEADER).read()
    # the structure's mirrors: the header's field list, the ctypes structure, the Rust shim's #[repr(C)] structure
    body = re.search(r"typedef struct ss_kaldi_params \{(.*?)\} ss_kaldi_params;", header, flags=re.S).group(1)
    kinds = {"uint32_t": C.c_uint32, "int32_t": C.c_int32, "float": C.c_float}
    fields = [(n, kinds[t]) for t, n in re.findall(r"(\w+)\s+(\w+)\s*;", body)]
    assert fields == list(_lib.SsKaldiParams._fields_) and len(fields) == 19
    rs = open(os.path.join(ROOT, "mfcc-rust_amd", "rust-shim", "src", "lib.rs")).read()
    rbody = re.search(r"pub struct KaldiParams \{(.*?)\n\}", rs, flags=re.S).group(1)
    rkinds = {"u32": C.c_uint32, "i32": C.c_int32, "f32": C.c_float}
    assert [(n, rkinds[t]) for n, t in re.findall(r"pub (\w+):\s*(\w+)\s*,", rbody)] == fields


def test_python_front_rejects_what_is_out_of_scope():
    import speechsauce_amd as ss

    x = np.zeros(4000, np.float32)
    for kw in (dict(dither=1.0), dict(snip_edges=False), dict(htk_compat=True), dict(subtract_mean=True), dict(vtln_warp=1.1), dict(channel=0),
               dict(vtln_low=100.0)):
        with pytest.raises(ValueError):
            ss.kaldi_fbank(x, **kw)
        with pytest.raises(ValueError):
            ss.kaldi_mfcc(x, **kw)
    with pytest.raises(TypeError):
        ss.kaldi_fbank(x, no_such_argument=1)
    with pytest.raises(ValueError):
        ss.kaldi_fbank(x, window_type="kaiser")
    with pytest.raises(TypeError):
        ss.kaldi_fbank(x.astype(np.float64))


# ---- well-posedness record: the restatement in f32 against the restatement in f64 on the GPU tests' inputs --------------------

def gpu_case_signal(seed, n, kind):
    """The three input families of tests/test_kaldi.py."""
    rng = np.random.default_rng(seed)
    if kind == "unit":
        return (rng.standard_normal(n) * 0.1).astype(np.float32)
    if kind == "scaled":
        return ((rng.standard_normal(n) * 0.1).astype(np.float32) * np.float32(32768.0)).astype(np.float32)
    assert kind == "int16"
    return rng.integers(-32768, 32768, n).astype(np.float32)


@pytest.mark.parametrize("kind", ["unit", "scaled"])
def test_the_specification_is_well_posed_in_f32(kind):
    """Seed 0, 3000 samples; recorded bounds: fbank-80 <= 2.4e-6 (block metric), MFCC column 0 <= 5.6e-7, columns 1.. <= 1.3e-6.
    This restatement measures 1.8e-6 / 2.9e-7 / 4.1e-7 at scale 1 and 7.3e-7 / 1.8e-7 / 7.1e-7 at scale 32768."""
    x = gpu_case_signal(0, 3000, kind)
    p80 = kp(num_mel_bins=80)
    fb = block_metric(ref_fbank(x, p80, np.float32)[0], ref_fbank(x, p80)[0])
    p23 = kp(num_mel_bins=23, num_ceps=13)
    c32, c64 = ref_mfcc(x, p23, np.float32), ref_mfcc(x, p23)
    c0, ck = block_metric(c32[:, 0], c64[:, 0]), block_metric(c32[:, 1:], c64[:, 1:])
    print(f"f32 restatement vs f64, {kind}: fbank-80 {fb:.3g}, mfcc column 0 {c0:.3g}, columns 1.. {ck:.3g}")
    assert fb < 1e-5 and c0 < 1e-5 and ck < 1e-5


# ---- the shapes of tests/test_kaldi_loop.py: which calls reach the kernel's persistent loop, which stay one quad per wave ---------

KALDI_WAVES = 12  # waves per workgroup of ss_kaldi_c256; a quad is four consecutive rows of the flat frame list
LOOP_T = 5        # frames per clip of the dense loop tests: no multiple of four, so quads straddle clips


def kaldi_grid(quads, cus):
    """cu_capped_grid(quads, 12, cus) of ss_launch_plan.h: one workgroup per CU, fewer where there is no quad for every wave"""
    return min(-(-quads // KALDI_WAVES), cus)


def workgroup_quads(quads, cus):
    """[q_lo, q_hi) of every workgroup, as the kernel's prologue computes them"""
    grid = kaldi_grid(quads, cus)
    return [(quads * b // grid, quads * (b + 1) // grid) for b in range(grid)]


def loop_dense_clips(cus, T=LOOP_T):
    """clips of T frames in a BIG dense call: at least 3 * 12 * cus + 5 quads, so every wave goes round the loop at least twice more"""
    return -(-4 * (3 * KALDI_WAVES * cus + 5) // T) + 1


def covered_clips(cus, T=LOOP_T):
    """clips of T frames in a COVERED dense call: at most 12 * cus quads, one per wave -- what the small-shape tests hold to f64"""
    return 4 * KALDI_WAVES * cus // T


def loop_packed_frames(cus, seed=0):
    """T_b of the clips of a BIG packed call: runs of one-frame clips (a quad over four clips), 1 .. 7 frames otherwise (offset_seek's
    steps), a clip of about 98 frames now and then (behind it the next claim is past the steps: offset_seek's binary search)"""
    rng = np.random.default_rng(seed)
    Ts, rows, want = [], 0, 4 * (3 * KALDI_WAVES * cus + 5)
    while rows < want:
        block = [1] * 9 + rng.integers(1, 8, 40).tolist() + [int(rng.integers(95, 102))] + rng.integers(1, 8, 7).tolist()
        Ts += block
        rows += sum(block)
    if rows % 4 == 0:
        Ts.append(3)
    return Ts


def packed_chunks(Ts, cus):
    """consecutive runs [i0, i1) of clips with at most 12 * cus quads each: the COVERED calls a big packed call is compared with"""
    cap, runs, i0, rows = 4 * KALDI_WAVES * cus, [], 0, 0
    for i, T in enumerate(Ts):
        if rows + T > cap:
            runs.append((i0, i))
            i0, rows = i, 0
        rows += T
    runs.append((i0, len(Ts)))
    return runs


@pytest.mark.parametrize("cus", [64, 256, 304])
def test_loop_test_shapes_reach_the_loop(cus):
    """Every shape of tests/test_kaldi_loop.py: in a big call each workgroup owns at least 3 x 12 quads -- a first quad and two further
    claims for each of its waves -- and in the calls it is compared with no workgroup owns more than 12: one quad per wave, no claim
    taken, the regime of tests/test_kaldi.py and tests/test_kaldi_builds.py."""
    def quads_of(rows):
        return -(-rows // 4)

    def check(big_rows, covered_rows):
        quads = quads_of(big_rows)
        assert quads >= 3 * KALDI_WAVES * cus + 5 and big_rows % 4 != 0
        spans = [hi - lo for lo, hi in workgroup_quads(quads, cus)]
        assert len(spans) == cus and min(spans) >= 3 * KALDI_WAVES
        assert len(covered_rows) >= 2  # the big call is more than one covered call
        for rows in covered_rows:
            assert rows > 0 and max(hi - lo for lo, hi in workgroup_quads(quads_of(rows), cus)) <= KALDI_WAVES

    B, Bc = loop_dense_clips(cus), covered_clips(cus)
    check(B * LOOP_T, [min(Bc, B - i) * LOOP_T for i in range(0, B, Bc)])
    Ts = loop_packed_frames(cus)
    assert Ts.count(1) > 9 and max(Ts) >= 95 and {2, 3, 4, 5, 6, 7} <= set(Ts)
    check(sum(Ts), [sum(Ts[i0:i1]) for i0, i1 in packed_chunks(Ts, cus)])
    # the equal-length clips of the dense case, packed: the same rows
    check(B * LOOP_T, [(i1 - i0) * LOOP_T for i0, i1 in packed_chunks([LOOP_T] * B, cus)])
