"""The Kaldi front end over a pool of stream states (ss_kstream_* in include/speechsauce_amd.h), host side: no device.

The exports and the mirrors, the size and row-offset helpers, the loud failures of the host forms and the Python classes without a
device, and -- in numpy f64, on the restatement of tests/test_kaldi_cpu.py -- the contract the GPU tests of tests/test_kaldi_stream.py
then hold the kernel to: the rows of zeros(S) ++ stream from row D on are the rows of the stream itself, and a model of the pool
(state ++ chunk, advance) gives the same rows and the same final state however the stream is cut into calls."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from test_kaldi_cpu import (HEADER, KALDI_WAVES, ROOT, SS_ERR_ARG, SS_ERR_UNSUPPORTED, SS_OK, gpu_case_signal, kaldi_grid, kp, make_kaldi_params,
                            ref_fbank, ref_sizes, workgroup_quads)

STREAM_SYMBOLS = ["ss_kstream_state_len", "ss_kstream_row_offsets", "ss_kstream_fbank_packed_device", "ss_kstream_mfcc_packed_device",
                  "ss_kstream_fbank_packed_i16_device", "ss_kstream_mfcc_packed_i16_device", "ss_kstream_fbank_packed", "ss_kstream_mfcc_packed",
                  "ss_kstream_fbank_packed_i16", "ss_kstream_mfcc_packed_i16"]

# id -> (configuration, flen, shift, NE, D, S): the shapes of the issue, every size checked against ss_kaldi_sizes below
SHAPES = {
    "16k_25_10": (dict(), 400, 160, 13, 2, 320),
    "16k_20_10": (dict(frame_length_ms=20.0), 320, 160, 10, 1, 160),
    "16k_32_10": (dict(frame_length_ms=32.0), 512, 160, 16, 3, 480),
    "11k_25_10": (dict(sample_rate=11025), 275, 110, 10, 2, 220),                                 # odd frame length
    "16k_25_10.1": (dict(frame_shift_ms=10.0625), 400, 161, 13, 2, 322),                           # odd shift
    "16k_20_10.1": (dict(frame_length_ms=20.0, frame_shift_ms=10.0625), 320, 161, 10, 1, 161),     # odd S: pairs straddle the boundary
    "16k_25_30": (dict(frame_shift_ms=30.0), 400, 480, 13, 0, 0),                                  # no state: NULL pool
}
# the standard call: 9 entries, a run of three zero-row entries inside one quad, quads that straddle entries; 12 rows, and 13
HOPS = [0, 1, 1, 3, 0, 0, 0, 5, 2]
HOPS_13 = [0, 1, 1, 3, 0, 0, 0, 5, 3]
SLOTS = [11, 2, 7, 0, 15, 4, 9, 1, 6]  # non-monotone, distinct, in a 16-row pool
POOL = 16


def state_len(sslib, sp):
    S, D = C.c_size_t(), C.c_size_t()
    rc = sslib.ss_kstream_state_len(C.byref(sp), C.byref(S), C.byref(D))
    return rc, S.value, D.value


def row_offsets(sslib, sp, so):
    so = np.asarray(so, np.int64)
    ro = np.full(so.size, -1, np.int64)
    rc = sslib.ss_kstream_row_offsets(C.byref(sp), so.size - 1, so.ctypes.data, ro.ctypes.data)
    return rc, ro


def loop_rows(cus):
    """rows of the persistent-loop call of tests/test_kaldi_stream.py"""
    return 4 * (3 * KALDI_WAVES * cus + 5) + 1


def loop_hops(cus, n_entries=64, seed=0):
    """the hop counts of its 64 entries: uneven, a few of them zero, summing to loop_rows(cus)"""
    rng = np.random.default_rng(seed)
    w = rng.integers(1, 8, n_entries).astype(np.int64)
    w[[5, 6, 40]] = 0
    hops = w * (loop_rows(cus) // int(w.sum()))
    hops[-1] += loop_rows(cus) - int(hops.sum())
    return hops.tolist()


def test_exports_and_mirrors(sslib):
    """Fails on a library without the pool: the symbols are declared, exported, prototyped and mirrored."""
    from speechsauce_amd import _lib

    header = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(ss_kstream_[a-z0-9_]+)\s*\(", header))
    assert declared == set(STREAM_SYMBOLS)
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name in STREAM_SYMBOLS:
        assert name in exported, f"{name} is not exported"
        assert name in _lib.PROTOTYPES, f"{name} has no ctypes prototype"
    assert sslib.ss_abi_version() == 7 == _lib.ABI_VERSION
    # the ctypes prototypes have the header's argument counts, and so have the Rust externs (host forms and the two helpers)
    rs = open(os.path.join(ROOT, "mfcc-rust_amd", "rust-shim", "src", "lib.rs")).read()
    ckind = {"size_t": "usize", "float": "f32", "int64_t": "i64", "int32_t": "i32", "int16_t": "i16", "ss_kaldi_params": "KaldiParams",
             "ss_kaldi_config": "c_void"}
    for name in STREAM_SYMBOLS:
        args = re.search(r"\bint " + name + r"\s*\((.*?)\)\s*;", header, flags=re.S).group(1).split(",")
        assert len(args) == len(_lib.PROTOTYPES[name][1]), name
        if name.endswith("_device"):
            continue
        m = re.search(r"\bfn " + name + r"\s*\((.*?)\)\s*->\s*c_int;", rs, flags=re.S)
        assert m, f"{name} has no Rust extern"
        rargs = [a.split(":")[1].strip() for a in m.group(1).split(",")]
        assert len(rargs) == len(args), name
        for c_arg, r_arg in zip(args, rargs):
            words = c_arg.replace("*", " * ").split()
            base = next(w for w in words if w in ckind)
            want = ("*const " if "const" in words else "*mut ") + ckind[base] if "*" in words else ckind[base]
            assert r_arg == want, (name, c_arg.strip(), r_arg)
    hpp = open(os.path.join(ROOT, "include", "speechsauce_amd.hpp")).read()
    for name in STREAM_SYMBOLS:
        if not name.endswith("_device"):
            assert name + "(" in hpp, f"{name} is not wrapped in speechsauce_amd.hpp"
            assert name + "(" in rs.split("impl KaldiFrontEnd")[1], f"{name} is not wrapped on KaldiFrontEnd"
    import speechsauce_amd as ss

    assert {"KaldiFbankStreamPool", "KaldiMfccStreamPool"} <= set(ss.__all__)


@pytest.mark.parametrize("name", list(SHAPES))
def test_state_len(sslib, name):
    cfg, flen, shift, _, D, S = SHAPES[name]
    sp = make_kaldi_params(sslib, **cfg)
    a, b, c = C.c_size_t(), C.c_size_t(), C.c_size_t()
    assert sslib.ss_kaldi_sizes(C.byref(sp), C.byref(a), C.byref(b), C.byref(c)) == SS_OK
    assert (a.value, b.value, c.value) == (flen, shift, 512) == ref_sizes(kp(**cfg))
    assert D == -(-flen // shift) - 1 and S == D * shift
    assert state_len(sslib, sp) == (SS_OK, S, D)


def test_state_len_and_row_offsets_rejections(sslib):
    sp = make_kaldi_params(sslib)
    S, D = C.c_size_t(), C.c_size_t()
    assert sslib.ss_kstream_state_len(None, C.byref(S), C.byref(D)) == SS_ERR_ARG
    assert sslib.ss_kstream_state_len(C.byref(sp), None, C.byref(D)) == SS_ERR_ARG
    assert sslib.ss_kstream_state_len(C.byref(sp), C.byref(S), None) == SS_ERR_ARG
    other = make_kaldi_params(sslib, sample_rate=8000)  # ss_kaldi_params_validate's codes apply first
    assert state_len(sslib, other)[0] == SS_ERR_UNSUPPORTED == sslib.ss_kaldi_params_validate(C.byref(other))
    assert row_offsets(sslib, other, [0, 80])[0] == SS_ERR_UNSUPPORTED
    so = np.asarray([0] + np.cumsum(np.asarray(HOPS) * 160).tolist(), np.int64)
    rc, ro = row_offsets(sslib, sp, so)
    assert rc == SS_OK and ro.tolist() == [0] + np.cumsum(HOPS).tolist()
    assert row_offsets(sslib, sp, [0])[0] == SS_OK  # no entries
    for bad in ([160, 320], [0, 320, 160], [0, 160, 330], [0, 160 * (2 ** 31)]):
        rc, ro = row_offsets(sslib, sp, bad)
        assert rc == SS_ERR_ARG, bad
    assert row_offsets(sslib, sp, [0, 160, 330])[0] == SS_ERR_ARG and b"entry 1" in sslib.ss_last_error_string()
    ro = np.zeros(2, np.int64)
    assert sslib.ss_kstream_row_offsets(C.byref(sp), 1, None, ro.ctypes.data) == SS_ERR_ARG
    assert sslib.ss_kstream_row_offsets(C.byref(sp), 1, ro.ctypes.data, None) == SS_ERR_ARG
    odd = make_kaldi_params(sslib, frame_shift_ms=10.0625)
    assert row_offsets(sslib, odd, [0, 161, 161, 483])[1].tolist() == [0, 1, 1, 3]


def test_host_forms_fail_loudly_without_a_handle(sslib):
    """The argument rules that need no device: a null handle on every entry point, and nothing is written."""
    x = np.zeros(320, np.float32)
    pcm = np.zeros(320, np.int16)
    so = np.asarray([0, 320], np.int64)
    sl = np.zeros(1, np.int32)
    pool = np.full((4, 320), 3.0, np.float32)
    out = np.full((2, 80), -5.0, np.float32)
    en = np.full(2, -5.0, np.float32)
    f, p, o, e = x.ctypes.data, pool.ctypes.data, out.ctypes.data, en.ctypes.data
    assert sslib.ss_kstream_fbank_packed(None, f, 1, so.ctypes.data, sl.ctypes.data, 4, p, o, e) == SS_ERR_ARG
    assert sslib.ss_kstream_mfcc_packed(None, f, 1, so.ctypes.data, sl.ctypes.data, 4, p, o) == SS_ERR_ARG
    assert sslib.ss_kstream_fbank_packed_i16(None, pcm.ctypes.data, 1, so.ctypes.data, sl.ctypes.data, 4, 1.0, p, o, e) == SS_ERR_ARG
    assert sslib.ss_kstream_mfcc_packed_i16(None, pcm.ctypes.data, 1, so.ctypes.data, sl.ctypes.data, 4, 1.0, p, o) == SS_ERR_ARG
    assert sslib.ss_kstream_fbank_packed_device(None, f, 1, so.ctypes.data, so.ctypes.data, 2, sl.ctypes.data, 4, p, o, e, None) == SS_ERR_ARG
    assert sslib.ss_kstream_mfcc_packed_i16_device(None, f, 1, so.ctypes.data, so.ctypes.data, 2, sl.ctypes.data, 4, 1.0, p, o, None) == SS_ERR_ARG
    assert (pool == 3.0).all() and (out == -5.0).all() and (en == -5.0).all()


def test_python_classes_fail_loudly():
    import speechsauce_amd as ss

    for cls in (ss.KaldiFbankStreamPool, ss.KaldiMfccStreamPool):
        pool = cls(4, num_mel_bins=23)
        assert (pool.state_len, pool.delay_rows, pool.hop, pool.pool_streams) == (320, 2, 160, 4)
        assert pool.state is None
        pool.reset([1])  # nothing to zero yet
        x = np.zeros(480, np.float32)
        with pytest.raises(ValueError, match="named twice"):
            pool(x, [160, 320], [1, 1])
        with pytest.raises(ValueError, match="outside the pool"):
            pool(x, [160, 320], [1, 4])
        with pytest.raises(ValueError, match="multiple of the hop"):
            pool(x, [161, 319], [1, 2])
        with pytest.raises(ValueError, match="multiple of the hop"):
            pool(x, [0, 161, 480], [1, 2])  # the same entries as sample offsets
        with pytest.raises(ValueError):
            pool(x, [160, 160], [1, 2])  # the lengths do not cover the buffer
        with pytest.raises(ValueError):
            pool(x, [160, 320], [1])
        with pytest.raises(ValueError, match="power of two"):
            pool(np.zeros(480, np.int16), [160, 320], [1, 2], pcm_scale=3.0)
        with pytest.raises(TypeError):
            pool(x, [160, 320], [1, 2], pcm_scale=1.0)  # float chunks with a PCM scale
        with pytest.raises(TypeError):
            pool(x.astype(np.float64), [160, 320], [1, 2])
        assert pool.state is None  # nothing was allocated, nothing written
        with pytest.raises(ValueError):
            cls(0)
        with pytest.raises(ValueError):
            cls(4, dither=1.0)
        with pytest.raises(ValueError):
            cls(4, snip_edges=False)
        with pytest.raises(TypeError):
            cls(4, no_such_argument=1)
        with pytest.raises(ss.SpeechSauceError) as err:
            cls(4, sample_frequency=8000)
        assert err.value.status == SS_ERR_UNSUPPORTED
    assert ss.KaldiFbankStreamPool(2, frame_shift=30.0).state_len == 0


@pytest.mark.parametrize("name", list(SHAPES))
def test_rows_behind_the_zero_prefix_are_the_streams_own(name):
    """f64: ref_fbank(zeros(S) ++ s) rows D.. are exactly ref_fbank(s) -- every per-frame stage is frame-local, and a stream of K hops
    has exactly K - D offline frames."""
    cfg, flen, shift, _, D, S = SHAPES[name]
    p = kp(**cfg, num_mel_bins=40, energy_floor=0.0)
    for kind in ("unit", "scaled", "int16"):
        K = 9
        s = gpu_case_signal(11, K * shift, kind)
        fb, le = rows_ref(np.concatenate([np.zeros(S, np.float32), s]), p)
        own, own_le = rows_ref(s, p)
        assert fb.shape[0] == K and own.shape[0] == K - D
        np.testing.assert_array_equal(fb[D:], own)
        np.testing.assert_array_equal(le[D:], own_le)


def rows_ref(x, p):
    """ref_fbank of every frame of x on its own -> (fbank [T x M], log_energy [T]).  (One frame per call: the restatement's mel
    product is a BLAS call whose last bits depend on how many rows it is handed, and this file compares blocks of different row
    counts for equality.)"""
    flen, shift, _ = ref_sizes(p)
    T = 0 if len(x) < flen else 1 + (len(x) - flen) // shift
    one = [ref_fbank(x[t * shift:t * shift + flen], p) for t in range(T)]
    return np.concatenate([o[0] for o in one]), np.concatenate([o[1] for o in one])


def pool_model(stream, cuts, p, S, shift):
    """The pool in numpy: per call the rows of state ++ chunk, then the advance -> (all rows, all log energies, final state)"""
    state = np.zeros(S, np.float32)
    rows, les, at = [], [], 0
    for hops in cuts:
        chunk = stream[at:at + hops * shift]
        at += hops * shift
        both = np.concatenate([state, chunk])
        if hops:
            fb, le = rows_ref(both, p)
            assert fb.shape[0] == hops
            rows.append(fb)
            les.append(le)
        state = both[both.size - S:]
    assert at == stream.size
    return np.concatenate(rows), np.concatenate(les), state


@pytest.mark.parametrize("name", list(SHAPES))
def test_the_pool_model_does_not_depend_on_the_cuts(name):
    cfg, flen, shift, _, D, S = SHAPES[name]
    p = kp(**cfg, num_mel_bins=40, energy_floor=0.0)
    K = 14
    stream = gpu_case_signal(21, K * shift, "unit")
    rng = np.random.default_rng(5)
    ragged = []
    while sum(ragged) < K:
        ragged.append(min(int(rng.integers(0, 6)), K - sum(ragged)))
    want, want_le = rows_ref(np.concatenate([np.zeros(S, np.float32), stream]), p)
    results = [pool_model(stream, cuts, p, S, shift) for cuts in ([1] * K, ragged, [K])]
    for rows, le, state in results:
        np.testing.assert_array_equal(rows, want)
        np.testing.assert_array_equal(le, want_le)
        np.testing.assert_array_equal(state, np.concatenate([np.zeros(S, np.float32), stream])[K * shift:])


@pytest.mark.parametrize("cus", [64, 256, 304])
def test_the_loop_shape_reaches_the_loop(cus):
    """The row count of the persistent-loop test gives every workgroup more quads than waves: each wave claims again."""
    rows = loop_rows(cus)
    quads = -(-rows // 4)
    assert rows % 4 == 1 and quads == 3 * KALDI_WAVES * cus + 6
    assert kaldi_grid(quads, cus) == cus
    spans = [hi - lo for lo, hi in workgroup_quads(quads, cus)]
    assert len(spans) == cus and min(spans) >= 3 * KALDI_WAVES > KALDI_WAVES
    hops = loop_hops(cus)
    assert len(hops) == 64 and sum(hops) == rows and hops.count(0) == 3 and min(hops) >= 0
