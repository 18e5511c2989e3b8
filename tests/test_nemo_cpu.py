"""The NeMo / Parakeet log-mel front end without a device: tests/nemo_model.py (the numpy restatement of the ss_nemo_* comment of
include/speechsauce_amd.h) against the torch.stft wording of transformers' ParakeetFeatureExtractor lines, the library's host
helpers (window, mel bank, frame counts, packed offsets, validation) against the restatement, the structure's three mirrors, and
the f32 restatement's own score against f64 on the inputs of tests/test_nemo.py -- the yardstick the kernel's score is read against."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import nemo_model as nm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "speechsauce_amd.h")
SS_OK, SS_ERR_BAD_CONFIG, SS_ERR_ARG, SS_ERR_HIP, SS_ERR_UNSUPPORTED, SS_ERR_DEVICE = 0, 2, 3, 4, 5, 6
BAR = 1e-4  # the project's: max|got - want| / max|want| over a block


def make_nemo_params(sslib, n_mels=80, **kw):
    from speechsauce_amd._lib import SsNemoParams

    p = SsNemoParams()
    assert sslib.ss_nemo_params_default(C.byref(p), n_mels) == SS_OK
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def test_defaults_are_the_extractors(sslib):
    p = make_nemo_params(sslib, 128)
    assert p.struct_size == C.sizeof(type(p)) == 40
    assert (p.sample_rate, p.n_fft, p.win_length, p.hop_length, p.n_mels, p.normalize) == (16000, 512, 400, 160, 128, 1)
    assert p.preemph == np.float32(0.97) and p.log_guard == 2.0 ** -24 and p.norm_eps == np.float32(1e-5)
    assert sslib.ss_nemo_params_validate(C.byref(p)) == SS_OK


@pytest.mark.parametrize("n_mels", nm.GPU_BANDS)
@pytest.mark.parametrize("L", [320, 3000, 16000])
def test_restatement_against_the_extractors_lines(n_mels, L):
    """features() in f64 against the extractor's text run by torch in f32 (its STFT centres the window in the 512-point frame: a
    phase, which the power spectrum drops; it yields one frame more than features_lengths, which the text masks out)"""
    x = nm.make_input(L, 7 + L)
    worst = {}
    for normalize in (False, True):
        want = nm.features(x, n_mels, normalize)
        got = nm.extractor_wording(x, n_mels, normalize=normalize)
        assert got.shape == want.shape == (L // 160, n_mels)
        worst[normalize] = nm.block_metric(got, want)
    print(f"nemo restatement vs torch.stft wording, {L} samples, {n_mels} bands: log-mel {worst[False]:.3g}, normalised {worst[True]:.3g}")
    assert worst[False] <= BAR and worst[True] <= BAR


def test_preemphasis_of_a_constant_clip():
    """the first sample keeps 1.0, the rest become 0.03, the tail (beyond the clip) is zero: the restatement's frames of a 560-sample
    clip of ones, window taken out"""
    y = nm.preemphasized(np.ones(560, np.float32))
    assert y[0] == 1.0 and np.allclose(y[1:], 1.0 - nm.PREEMPH, rtol=0, atol=1e-15)
    assert np.array_equal(nm.preemphasized(np.ones(560, np.float32), 0.0), np.ones(560))
    # frame 2 of 3 covers clip samples 120 .. 519; frame 0 starts 200 samples in front of the clip, and nothing follows sample 559
    P = nm.power(np.ones(560, np.float32))
    assert P.shape == (3, 257) and np.isfinite(P).all()


@pytest.mark.parametrize("W", [400, 320, 512, 258])
def test_window_table(sslib, W):
    w = np.empty(W, np.float32)
    assert sslib.ss_nemo_window(C.byref(make_nemo_params(sslib, win_length=W)), w.ctypes.data) == SS_OK
    assert np.abs(w.astype(np.float64) - nm.window(W)).max() <= 2.0 ** -23
    assert w[0] == 0.0 and abs(w[-1]) <= 2.0 ** -23 and np.array_equal(w, w[::-1])  # symmetric: torch.hann_window(W, periodic=False)


@pytest.mark.parametrize("n_mels", [80, 128, 3, 1])
def test_mel_bank_table(sslib, n_mels):
    bank = np.empty((n_mels, nm.BINS), np.float32)
    assert sslib.ss_nemo_mel_bank(C.byref(make_nemo_params(sslib, n_mels)), bank.ctypes.data) == SS_OK
    want = nm.mel_bank(n_mels)
    assert np.abs(bank.astype(np.float64) - want).max() <= 1e-6
    assert np.array_equal(bank != 0, want.astype(np.float32) != 0)
    assert (bank[:, 256] == 0).all()  # the Nyquist bin has weight 0


def test_mel_bank_shapes_of_record(sslib):
    """what the kernel's eight slots per lane were sized for: 504 taps of 1 .. 12 per band at 128 bands, 500 of 2 .. 18 at 80, no band
    empty, every band's taps one run of bins"""
    for n_mels, total, lo, hi in ((128, 504, 1, 12), (80, 500, 2, 18)):
        bank = np.empty((n_mels, nm.BINS), np.float32)
        assert sslib.ss_nemo_mel_bank(C.byref(make_nemo_params(sslib, n_mels)), bank.ctypes.data) == SS_OK
        taps = (bank != 0).sum(axis=1)
        assert (int(taps.sum()), int(taps.min()), int(taps.max())) == (total, lo, hi)
        for row in bank:
            nz = np.flatnonzero(row)
            assert nz.size and nz[-1] - nz[0] + 1 == nz.size


LENS = [0, 159, 160, 161, 399, 400, 3000]


def test_frame_counts_and_packed_offsets(sslib):
    p = make_nemo_params(sslib)
    t = C.c_size_t(99)
    for L in LENS:
        assert sslib.ss_nemo_num_frames(C.byref(p), L, C.byref(t)) == SS_OK and t.value == nm.num_frames(L) == L // 160
    assert [nm.num_frames(L) for L in LENS] == [0, 0, 1, 1, 2, 2, 18]
    so = np.concatenate([[0], np.cumsum(LENS)]).astype(np.int64)
    fo = np.full_like(so, -1)
    assert sslib.ss_nemo_packed_frame_offsets(C.byref(p), len(LENS), so.ctypes.data, fo.ctypes.data) == SS_OK
    assert fo.tolist() == np.concatenate([[0], np.cumsum([L // 160 for L in LENS])]).tolist()
    bad = so.copy()
    bad[3] = bad[2] - 1
    assert sslib.ss_nemo_packed_frame_offsets(C.byref(p), len(LENS), bad.ctypes.data, fo.ctypes.data) == SS_ERR_ARG
    bad = so.copy()
    bad[0] = 1
    assert sslib.ss_nemo_packed_frame_offsets(C.byref(p), len(LENS), bad.ctypes.data, fo.ctypes.data) == SS_ERR_ARG
    import speechsauce_amd as ss

    assert [ss.nemo_num_frames(L) for L in LENS] == [L // 160 for L in LENS]


NAN, INF = float("nan"), float("inf")
VALIDATION = [
    (dict(), SS_OK),
    (dict(n_mels=128), SS_OK), (dict(n_mels=1), SS_OK), (dict(win_length=258), SS_OK), (dict(win_length=512), SS_OK),
    (dict(normalize=0), SS_OK), (dict(preemph=0.0), SS_OK), (dict(norm_eps=0.0), SS_OK),
    (dict(sample_rate=8000), SS_ERR_UNSUPPORTED), (dict(sample_rate=22050), SS_ERR_UNSUPPORTED),
    (dict(n_fft=400), SS_ERR_UNSUPPORTED), (dict(n_fft=1024), SS_ERR_UNSUPPORTED),
    (dict(hop_length=128), SS_ERR_UNSUPPORTED), (dict(hop_length=161), SS_ERR_UNSUPPORTED),
    (dict(n_mels=129), SS_ERR_UNSUPPORTED), (dict(n_mels=256), SS_ERR_UNSUPPORTED),
    (dict(n_mels=0), SS_ERR_BAD_CONFIG),
    (dict(win_length=401), SS_ERR_BAD_CONFIG), (dict(win_length=256), SS_ERR_BAD_CONFIG), (dict(win_length=514), SS_ERR_BAD_CONFIG),
    (dict(win_length=0), SS_ERR_BAD_CONFIG),
    (dict(preemph=-0.5), SS_ERR_BAD_CONFIG), (dict(preemph=NAN), SS_ERR_BAD_CONFIG), (dict(preemph=INF), SS_ERR_BAD_CONFIG),
    (dict(log_guard=0.0), SS_ERR_BAD_CONFIG), (dict(log_guard=-1e-8), SS_ERR_BAD_CONFIG), (dict(log_guard=NAN), SS_ERR_BAD_CONFIG),
    (dict(log_guard=INF), SS_ERR_BAD_CONFIG),
    (dict(norm_eps=-1e-5), SS_ERR_BAD_CONFIG), (dict(norm_eps=NAN), SS_ERR_BAD_CONFIG), (dict(norm_eps=INF), SS_ERR_BAD_CONFIG),
    (dict(normalize=2), SS_ERR_BAD_CONFIG),
    (dict(struct_size=36), SS_ERR_ARG), (dict(struct_size=44), SS_ERR_ARG),
]


@pytest.mark.parametrize("cfg,want", VALIDATION, ids=[",".join(f"{k}={v}" for k, v in c.items()) or "default" for c, _ in VALIDATION])
def test_validation_rules(sslib, cfg, want):
    p = make_nemo_params(sslib, **cfg)
    assert sslib.ss_nemo_params_validate(C.byref(p)) == want
    if want != SS_OK:  # every host helper and the handle refuse what validate refuses, before a device is looked for
        h, t = C.c_void_p(), C.c_size_t()
        assert sslib.ss_nemo_config_create(C.byref(p), C.byref(h)) == want and not h.value
        assert sslib.ss_nemo_num_frames(C.byref(p), 1600, C.byref(t)) == want
    assert sslib.ss_nemo_params_validate(None) == SS_ERR_ARG


NEW_SYMBOLS = ["ss_nemo_params_default", "ss_nemo_params_validate", "ss_nemo_num_frames", "ss_nemo_packed_frame_offsets", "ss_nemo_window",
               "ss_nemo_mel_bank", "ss_nemo_config_create", "ss_nemo_config_destroy", "ss_nemo_config_params", "ss_nemo_config_device_status",
               "ss_nemo_log_mel_device", "ss_nemo_log_mel", "ss_nemo_log_mel_packed_device", "ss_nemo_log_mel_packed"]


def test_exports_and_mirrors(sslib):
    import subprocess

    from speechsauce_amd import _lib

    text = open(HEADER).read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert set(re.findall(r"\b(ss_nemo_[a-z0-9_]+)\s*\(", header)) == set(NEW_SYMBOLS)
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name in NEW_SYMBOLS:
        assert name in exported, f"{name} is not exported"
        assert name in _lib.PROTOTYPES, f"{name} has no ctypes prototype"
    assert sslib.ss_abi_version() == 7 == _lib.ABI_VERSION and "#define SS_ABI_VERSION 7" in text  # entry points only
    # the structure's mirrors: the header's field list, the ctypes structure, the Rust shim's #[repr(C)] structure
    body = re.search(r"typedef struct ss_nemo_params \{(.*?)\} ss_nemo_params;", header, flags=re.S).group(1)
    kinds = {"uint32_t": C.c_uint32, "int32_t": C.c_int32, "float": C.c_float}
    fields = [(n, kinds[t]) for t, n in re.findall(r"(\w+)\s+(\w+)\s*;", body)]
    assert fields == list(_lib.SsNemoParams._fields_) and len(fields) == 10 and all(C.sizeof(k) == 4 for _, k in fields)
    rs = open(os.path.join(ROOT, "mfcc-rust_amd", "rust-shim", "src", "lib.rs")).read()
    rbody = re.search(r"pub struct SsNemoParams \{(.*?)\n\}", rs, flags=re.S).group(1)
    rkinds = {"u32": C.c_uint32, "i32": C.c_int32, "f32": C.c_float}
    assert [(n, rkinds[t]) for n, t in re.findall(r"pub (\w+):\s*(\w+)\s*,", rbody)] == fields
    for name in NEW_SYMBOLS:
        if name not in ("ss_nemo_params_validate", "ss_nemo_window", "ss_nemo_mel_bank", "ss_nemo_config_params"):
            assert re.search(rf"\bfn {name}\(", rs), f"{name} has no signature in the Rust shim"
    hpp = open(os.path.join(ROOT, "include", "speechsauce_amd.hpp")).read()
    assert "ss_nemo_config_create" in hpp and "ss_nemo_log_mel_packed_device" in hpp
    assert text.count("SS_NEMO_NORM_NONE 0") == 1 and text.count("SS_NEMO_NORM_PER_FEATURE 1") == 1


def test_python_front_argument_rules():
    import speechsauce_amd as ss

    with pytest.raises(ValueError, match="all_features"):
        ss.nemo_log_mel(np.zeros(1600, np.float32), normalize="all_features")
    with pytest.raises(TypeError):
        ss.nemo_log_mel(np.zeros(1600, np.float64))
    with pytest.raises(ValueError):
        ss.nemo_log_mel_packed(np.zeros(1600, np.float32), [1000, 1000])
    with pytest.raises(ValueError, match="device_tables"):
        ss.nemo_log_mel_packed(np.zeros(1600, np.float32), None, device_tables=(None, None, 0))
    with pytest.raises(ValueError, match="no clips"):
        ss.nemo_log_mel_list([])
    with pytest.raises(ss.SpeechSauceError) as e:
        ss.nemo_log_mel(np.zeros(1600, np.float32), win_length=401)
    assert e.value.status == SS_ERR_BAD_CONFIG
    with pytest.raises(ss.SpeechSauceError) as e:
        ss.nemo_log_mel(np.zeros(1600, np.float32), n_mels=129)
    assert e.value.status == SS_ERR_UNSUPPORTED


def test_null_arguments(sslib):
    p = make_nemo_params(sslib)
    h = C.c_void_p()
    assert sslib.ss_nemo_config_create(None, C.byref(h)) == SS_ERR_ARG
    assert sslib.ss_nemo_config_device_status(None) == SS_ERR_ARG
    assert sslib.ss_nemo_config_params(None, C.byref(p)) == SS_ERR_ARG
    assert sslib.ss_nemo_log_mel_device(None, None, 1, 1600, 1600, None, None) == SS_ERR_ARG
    assert sslib.ss_nemo_log_mel(None, None, 1, 1600, 1600, None) == SS_ERR_ARG
    assert sslib.ss_nemo_log_mel_packed_device(None, None, 1, None, None, 10, None, None) == SS_ERR_ARG
    assert sslib.ss_nemo_log_mel_packed(None, None, 1, None, None) == SS_ERR_ARG
    assert sslib.ss_nemo_window(C.byref(p), None) == SS_ERR_ARG and sslib.ss_nemo_mel_bank(C.byref(p), None) == SS_ERR_ARG
    sslib.ss_nemo_config_destroy(None)


@pytest.mark.parametrize("n_mels", nm.GPU_BANDS)
def test_the_specification_is_well_posed_in_f32(n_mels):
    """The yardstick: the restatement with every array in f32 against f64 on the GPU tests' inputs.  A kernel that scores much worse
    than this on the same input has lost precision somewhere; one that scores the same is as good as f32 gets."""
    raw = norm = 0.0
    for L in nm.GPU_LENS:
        x = nm.gpu_clip(L)
        r = nm.block_metric(nm.features_f32(x, n_mels, False), nm.features(x, n_mels, False))
        raw = max(raw, r)
        line = f"nemo f32 yardstick, {L} samples, {n_mels} bands: log-mel {r:.3g}"
        if L // 160 >= 2:
            n = nm.block_metric(nm.features_f32(x, n_mels, True), nm.features(x, n_mels, True))
            norm = max(norm, n)
            line += f", normalised {n:.3g}"
        print(line)
    assert raw <= BAR and norm <= BAR


def test_loop_test_shape_reaches_the_loop():
    """64 clips of 200 frames: more quads than 12 waves on each of 256 CUs, so on any device up to that size the grid is one workgroup
    per CU and waves go round the loop again (tests/test_nemo.py::test_dense_loop asserts it for the device's own CU count)"""
    assert nm.loop_quads() == 3200 > nm.WAVES * 256
