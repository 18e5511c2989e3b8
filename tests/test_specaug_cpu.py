"""SpecAugment of packed rows (ss_specaug_* / ss_mask_spans_*), the part that needs no device: the numpy restatement
(tests/specaug_model.py) against the header's known answers and worked pin, ss_specaug_spans against the restatement bit for bit,
the uniformity of the draws, every argument error of every form, the symbols in every mirror and the Python front's argument rules."""
import ctypes as C
import itertools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from specaug_model import FREQ_BASE, KNOWN, PIN, apply_ref, chi2, clip, draw, philox, spans_ref, time_bound, u32

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"ss_specaug_spans": 12, "ss_specaug_plan_packed_device": 13, "ss_mask_spans_packed_device": 11, "ss_mask_spans_packed": 10,
         "ss_specaug_packed_device": 16, "ss_specaug_packed": 15}
ERR_ARG = 3
LENS = [0, 1, 2, 63, 64, 65, 7, 300]
# (cols, (n_time, n_freq), width, ratio, clip_base, epoch): the grid the device test walks too
GRID = list(itertools.product((1, 13, 80), ((0, 0), (1, 0), (0, 1), (2, 2), (16, 16)), (0, 1, 10, 1000), (1.0, 0.2, 0.0), (0, 5),
                              (0, 2 ** 32 - 1, 2 ** 32)))
SEED = 0x9E3779B97F4A7C15  # both halves of the key are used


def _table(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


def _spans(sslib, rng, clip_base, ro, total_rows, cols, n_time, max_tw, ratio, n_freq, max_fw):
    """ss_specaug_spans into a table with a spare pair behind it"""
    words = np.array(rng, np.uint64)
    n = len(ro) - 1
    out = np.full((n * (n_time + n_freq) + 1, 2), -99, np.int32)
    ro = np.ascontiguousarray(ro, np.int64)
    rc = sslib.ss_specaug_spans(words.ctypes.data, clip_base, n, ro.ctypes.data, total_rows, cols, n_time, max_tw, ratio, n_freq, max_fw, out.ctypes.data)
    assert rc == 0, sslib.ss_last_error_string()
    assert (out[-1] == -99).all() and words.tolist() == [int(v) for v in rng]  # nothing behind the table, the block is read only
    return out[:-1].reshape(n, n_time + n_freq, 2)


def test_philox_known_answers():
    for ctr, key, want in KNOWN:
        assert tuple(int(v) for v in philox(ctr, key)) == want
    # on arrays, element for element
    got = philox(tuple(np.array([k[0][i] for k in KNOWN], np.uint64) for i in range(4)), KNOWN[0][1])
    assert tuple(int(v[0]) for v in got) == KNOWN[0][2]


def test_known_answers_through_the_library(sslib):
    """ss_specaug_spans runs csrc/ss_philox.h.  With seed 0, epoch 0 and clip 0, time mask 0 is drawn from the first known answer:
    u0 = 6627e8d5, u1 = e169c58d.  The library is then held to the restatement on counters and keys with every word in use (clip id,
    mask index, both halves of epoch and seed); the two known answers whose mask index no call can form go through the header in
    test_known_answers_through_the_header."""
    ro = np.array([0, 2 ** 31 - 1], np.int64)
    for seed, epoch, base in ((0, 0, 0), (2 ** 64 - 1, 2 ** 64 - 1, 2 ** 32 - 3), (0x299F31D0A4093822, 0x0370734413198A2E, 0x243F6A88)):
        got = _spans(sslib, (seed, epoch), base, ro, 2 ** 31 - 1, 2 ** 31 - 1, 16, 2 ** 31 - 1, 1.0, 16, 2 ** 31 - 1)
        for k in range(32):
            idx = k if k < 16 else FREQ_BASE + k - 16
            u0, u1, _, _ = (int(v) for v in philox((base, idx, epoch & 0xFFFFFFFF, epoch >> 32), (seed & 0xFFFFFFFF, seed >> 32)))
            width = (u0 * 2 ** 31) >> 32  # bound = extent = 2^31 - 1
            assert got[0, k].tolist() == [(u1 * (2 ** 31 - 1 - width + 1)) >> 32, width], (seed, k)
        if seed == 0:
            width = (0x6627E8D5 * 2 ** 31) >> 32
            assert got[0, 0].tolist() == [(0xE169C58D * (2 ** 31 - width)) >> 32, width]


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_known_answers_through_the_header(tmp_path):
    """tools/hosttest/test_philox.cpp: the three known answers from ss_philox.h itself, a stand-alone host program under ASan + UBSan"""
    exe = str(tmp_path / "test_philox")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "mfcc-rust_amd", "csrc"),
           os.path.join(ROOT, "tools", "hosttest", "test_philox.cpp"), "-o", exe]
    subprocess.run(cmd, check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout[-4000:] + r.stderr[-4000:]


def test_the_worked_pin(sslib):
    ro = _table([200, 200, 200])
    want = np.array(PIN, np.int32)
    assert np.array_equal(spans_ref((2026, 0), 0, ro, 600, 80, 2, 40, 1.0, 0, 0), want)
    assert np.array_equal(_spans(sslib, (2026, 0), 0, ro, 600, 80, 2, 40, 1.0, 0, 0), want)
    # ... whatever the clips' offsets: each clip alone, and behind a spacer
    for b in range(3):
        assert np.array_equal(_spans(sslib, (2026, 0), b, [0, 200], 200, 80, 2, 40, 1.0, 0, 0)[0], want[b])
        assert np.array_equal(_spans(sslib, (2026, 0), b - 1 if b else 0, [0, 7, 207] if b else [0, 200, 207], 207, 80, 2, 40, 1.0, 0, 0)[1 if b else 0], want[b])


def test_the_time_bound_is_one_f64_product_truncated():
    # float32(0.2) is 0.20000000298...: 5 rows give floor(1.0000000149) = 1, and float32(0.1) * 10 = 1.0000000149 too
    assert time_bound(np.array([0, 1, 4, 5, 10, 300]), 1000, 0.2).tolist() == [0, 0, 0, 1, 2, 60]
    assert time_bound(np.array([10, 20]), 1000, 0.1).tolist() == [1, 2] and time_bound(np.array([10, 20]), 1, 1.0).tolist() == [1, 1]
    assert time_bound(np.array([7]), 1000, 0.0).tolist() == [0]


def test_spans_equal_the_restatement_over_the_grid(sslib):
    ro = _table(LENS)
    total = int(ro[-1])
    seen_widths = set()
    for cols, (nt, nf), width, ratio, base, epoch in GRID:
        got = _spans(sslib, (SEED, epoch), base, ro, total, cols, nt, width, ratio, nf, width)
        want = spans_ref((SEED, epoch), base, ro, total, cols, nt, width, ratio, nf, width)
        assert got.dtype == want.dtype and np.array_equal(got, want), (cols, nt, nf, width, ratio, base, epoch)
        # every span lies inside its extent, and no width is above its bound
        T = np.array(LENS)[:, None]
        t, f = got[:, :nt], got[:, nt:]
        assert (t >= 0).all() and (t[:, :, 0] + t[:, :, 1] <= T).all() and (t[:, :, 1] <= np.minimum(width, np.floor(np.float64(np.float32(ratio)) * T))).all()
        assert (f >= 0).all() and (f[:, :, 0] + f[:, :, 1] <= cols).all() and (f[:, :, 1] <= min(width, cols)).all()
        seen_widths.update(got[:, :, 1].reshape(-1).tolist())
    assert max(seen_widths) == 300 and len(seen_widths) > 50  # width 1000 is capped by the longest clip; the draws are spread
    # epochs 2^32 - 1 and 2^32 differ in both counter words, clip_base shifts the ids
    a = _spans(sslib, (SEED, 2 ** 32 - 1), 0, ro, total, 80, 2, 10, 1.0, 2, 10)
    assert not np.array_equal(a, _spans(sslib, (SEED, 2 ** 32), 0, ro, total, 80, 2, 10, 1.0, 2, 10))
    assert not np.array_equal(a, _spans(sslib, (SEED, 2 ** 32 - 1), 5, ro, total, 80, 2, 10, 1.0, 2, 10))
    assert not np.array_equal(a, _spans(sslib, (SEED + 2 ** 32, 2 ** 32 - 1), 0, ro, total, 80, 2, 10, 1.0, 2, 10))


def test_bad_segments_have_no_spans(sslib):
    #               good | reversed | empty | good | past the end | reversed | reversed, ends below 0 | starts below 0 | good
    bad = np.array([0, 4, 2, 2, 6, 13, 12, -1, 3, 6], np.int64)
    got = _spans(sslib, (7, 1), 0, bad, 12, 13, 2, 5, 1.0, 2, 5)
    assert np.array_equal(got, spans_ref((7, 1), 0, bad, 12, 13, 2, 5, 1.0, 2, 5))
    for b in range(9):
        assert (got[b] == (-1, 0)).all() == (b in (1, 4, 5, 6, 7)), b
    clean = _spans(sslib, (7, 1), 8, [0, 3], 3, 13, 2, 5, 1.0, 2, 5)
    assert np.array_equal(got[8], clean[0])  # a good clip's spans do not depend on its neighbours


def test_draws_are_uniform():
    """Seed 2026, 4096 clips of 200 rows, 2 masks, width <= 40: the widths over their 41 values and start / (T - width + 1) over 20
    bins, against the 99.9 % quantiles of chi-square with 40 and 19 degrees of freedom (the restatement gives 37.4 and 24.9)."""
    n = 4096
    s = spans_ref((2026, 0), 0, np.arange(n + 1) * 200, n * 200, 80, 2, 40, 1.0, 0, 0)
    width, start = s[:, :, 1].reshape(-1), s[:, :, 0].reshape(-1)
    w2 = chi2(np.bincount(width, minlength=41), width.size / 41)
    s2 = chi2(np.bincount((start / (200 - width + 1) * 20).astype(int), minlength=20), start.size / 20)
    print("width chi2", w2, "start chi2", s2)
    assert w2 < 73.4 and s2 < 43.8


def test_draws_are_uniform_through_the_library(sslib):
    n = 4096
    ro = np.arange(n + 1, dtype=np.int64) * 200
    got = _spans(sslib, (2026, 0), 0, ro, n * 200, 80, 2, 40, 1.0, 0, 0)
    assert np.array_equal(got, spans_ref((2026, 0), 0, ro, n * 200, 80, 2, 40, 1.0, 0, 0))


def test_the_restatement_of_the_masking():
    cols, lens = 5, [4, 0, 6]
    ro = _table(lens)
    bits = u32(clip(cols, 10, seed=3)).copy()
    spans = np.array([[[1, 2], [3, 1], [0, 1], [4, 1]], [[0, 0]] * 4, [[5, 1], [4, 3], [2, 2], [3, 2]]], np.int32)  # clip 2: (4, 3) ends past its 6 rows
    out = apply_ref(bits, ro, 10, spans, 2, 2, 0xABCD)
    m = np.zeros((10, cols), bool)
    m[1:3] = m[3] = True
    m[0:4, 0] = m[0:4, 4] = True
    m[4 + 5] = True
    m[4:10, 2:5] = True
    assert (out[m] == 0xABCD).all() and np.array_equal(out[~m], bits[~m]) and not (bits == 0xABCD).any()
    # a bad segment and rows in no clip are untouched; `out` given: only covered rows are written
    held = np.full_like(bits, 7)
    got = apply_ref(bits, [0, 2, 1, 1], 10, np.zeros((3, 1, 2), np.int32), 1, 0, 0xABCD, out=held)
    assert np.array_equal(got[:2], bits[:2]) and (got[2:] == 7).all()
    s, w = draw(1, 2, np.arange(50), 0, np.full(50, 9), np.full(50, 9))
    assert ((s >= 0) & (w >= 0) & (w <= 9) & (s + w <= 9)).all() and len(set(w.tolist())) > 5


def test_symbols_are_declared_exported_and_prototyped(sslib):
    from speechsauce_amd import _lib

    header_text = open(os.path.join(ROOT, "include", "speechsauce_amd.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header_text, flags=re.S)
    shim = open(os.path.join(ROOT, "mfcc-rust_amd", "rust-shim", "src", "lib.rs")).read()
    externs = re.search(r'extern "C" \{(.*?)\n\}', shim, flags=re.S).group(1)
    hpp = open(os.path.join(ROOT, "include", "speechsauce_amd.hpp")).read()
    for name, arity in NAMES.items():
        decl = re.search(r"^int %s\(([^;]*?)\);" % name, header, flags=re.M | re.S)
        assert decl and len(decl.group(1).split(",")) == arity, name
        assert "uint64_t *" in decl.group(1) or "mask_spans" in name, name  # rng crosses the ABI as a pointer
        assert "void *stream" in decl.group(1) if name.endswith("_device") else "stream" not in decl.group(1), name
        ext = re.search(r"fn %s\((.*?)\)\s*->\s*c_int;" % name, externs, flags=re.S)
        assert ext and len(ext.group(1).split(",")) == arity, name
        assert name in _lib.PROTOTYPES, name
        fn = getattr(sslib, name)  # exported by the library (ss_exports.map lets every ss_* symbol out)
        assert fn.restype is C.c_int and len(fn.argtypes) == len(_lib.PROTOTYPES[name][1]) == arity, name
        assert name.endswith("_device") or name + "(" in hpp, name  # the C++ mirror wraps the host forms
    assert sorted(n for n in _lib.PROTOTYPES if "specaug" in n or "mask_spans" in n) == sorted(NAMES)
    assert "ss_*;" in open(os.path.join(ROOT, "mfcc-rust_amd", "csrc", "ss_exports.map")).read()
    assert re.search(r"#define SS_ABI_VERSION 7\b", header_text) and sslib.ss_abi_version() == 7 and _lib.ABI_VERSION == 7  # entry points only
    for fn in ("try_spec_augment_spans", "try_mask_spans_packed", "try_spec_augment_packed"):
        assert "pub fn %s(" % fn in shim, fn
    for fn in ("spec_augment_plan_packed_device", "mask_spans_packed_device", "spec_augment_packed_device"):
        assert "pub unsafe fn %s(" % fn in shim, fn
    mk = open(os.path.join(ROOT, "mfcc-rust_amd", "csrc", "Makefile")).read()
    assert re.search(r"^PLAIN\s*:=.*\bss_specaug\b", mk, flags=re.M) and re.search(r"^HDRS\s*:=.*\bss_philox\.h\b", mk, flags=re.M)


def test_argument_errors_are_decided_before_the_device_is_touched(sslib):
    """Every call here is rejected (or has nothing to do) on the host: none of the pointers is ever handed to the device, so host
    arrays stand in for device buffers.  On a host without a device a call that got past its checks would return SS_ERR_HIP (4)."""
    cols, rows, nt, nf = 13, 12, 2, 2
    vec = np.ones((rows, cols), np.float32)
    out = np.full((rows, cols), -5.0, np.float32)
    spans = np.full((2, nt + nf, 2), -7, np.int32)
    rng = np.array([2026, 9], np.uint64)
    off = np.array([0, 3, 12], np.int64)
    v, o, s, g, r = vec.ctypes.data, out.ctypes.data, spans.ctypes.data, rng.ctypes.data, off.ctypes.data

    def plan(rng=g, base=0, n=2, ro=r, total=rows, cols=cols, nt=nt, tw=10, ratio=1.0, nf=nf, fw=10, spans=s, **_):
        return sslib.ss_specaug_plan_packed_device(rng, base, n, ro, total, cols, nt, tw, ratio, nf, fw, spans, None)

    def host_spans(rng=g, base=0, n=2, ro=r, total=rows, cols=cols, nt=nt, tw=10, ratio=1.0, nf=nf, fw=10, spans=s, **_):
        return sslib.ss_specaug_spans(rng, base, n, ro, total, cols, nt, tw, ratio, nf, fw, spans)

    def mask_dev(vec=v, n=2, ro=r, total=rows, cols=cols, spans=s, nt=nt, nf=nf, value=0.0, out=o, **_):
        return sslib.ss_mask_spans_packed_device(vec, n, ro, total, cols, spans, nt, nf, value, out, None)

    def mask_host(vec=v, n=2, ro=r, total=rows, cols=cols, spans=s, nt=nt, nf=nf, value=0.0, out=o, **_):
        return sslib.ss_mask_spans_packed(vec, n, ro, total, cols, spans, nt, nf, value, out)

    def aug_dev(vec=v, n=2, ro=r, total=rows, cols=cols, rng=g, base=0, nt=nt, tw=10, ratio=1.0, nf=nf, fw=10, value=0.0, out=o, spans=s):
        return sslib.ss_specaug_packed_device(vec, n, ro, total, cols, rng, base, nt, tw, ratio, nf, fw, value, out, spans, None)

    def aug_host(vec=v, n=2, ro=r, total=rows, cols=cols, rng=g, base=0, nt=nt, tw=10, ratio=1.0, nf=nf, fw=10, value=0.0, out=o, spans=s):
        return sslib.ss_specaug_packed(vec, n, ro, total, cols, rng, base, nt, tw, ratio, nf, fw, value, out, spans)

    draws, masks = (plan, host_spans, aug_dev, aug_host), (mask_dev, mask_host, aug_dev, aug_host)
    for call in set(draws + masks):
        what = call.__name__
        assert call(n=0) == 0, what  # an empty call is SS_OK, also without a device and whatever else is passed
        assert call(n=0, cols=0, nt=99, ratio=7.0, spans=None) == 0, what
        for name in ("ro", "spans") + (("rng",) if call in draws else ()) + (("vec", "out") if call in masks else ()):
            assert call(**{name: None}) == ERR_ARG and b"null" in sslib.ss_last_error_string(), (what, name)
        assert call(cols=0) == ERR_ARG and b"cols" in sslib.ss_last_error_string(), what
        for name in ("nt", "nf"):
            assert call(**{name: 17}) == ERR_ARG and call(**{name: 1 << 40}) == ERR_ARG and b"16" in sslib.ss_last_error_string(), (what, name)
        for name in ("n", "total", "cols") + (("tw", "fw") if call in draws else ()):
            assert call(**{name: 1 << 31}) == ERR_ARG and call(**{name: 1 << 40}) == ERR_ARG, (what, name)
        if call in draws:
            for ratio in (-0.001, 1.001, float("nan"), float("inf"), -float("inf")):
                assert call(ratio=ratio) == ERR_ARG and b"time_ratio" in sslib.ss_last_error_string(), (what, ratio)
            assert call(base=(1 << 32) - 1) == ERR_ARG and call(base=(1 << 32) + 5) == ERR_ARG and call(base=1 << 63) == ERR_ARG, what
            assert b"clip_base" in sslib.ss_last_error_string()
        if call in masks:
            for value in (float("nan"), float("inf"), -0.0):  # any mask value is legal: the rejection is the other argument's
                assert call(value=value, cols=0) == ERR_ARG, what
            # out == vec is in place (these calls get past the overlap rule and fail on the null table); a partial overlap is not
            assert call(out=v, ro=None) == ERR_ARG and b"null" in sslib.ss_last_error_string(), what
            for shift in (4, 4 * (rows * cols - 1), -4, -4 * (rows * cols - 1)):
                assert call(out=v + shift) == ERR_ARG and b"partly overlaps" in sslib.ss_last_error_string(), (what, shift)
            assert call(out=o + 2) == ERR_ARG and b"aligned" in sslib.ss_last_error_string(), what
            for name, at in (("spans", v), ("spans", v + 4 * (rows * cols - 1)), ("spans", o), ("spans", o - 4 * (2 * (nt + nf) * 2 - 1))):
                assert call(**{name: at}) == ERR_ARG and b"spans overlaps" in sslib.ss_last_error_string(), (what, name)
    for call in (aug_dev, aug_host):
        for at in (v, v + 4 * rows * cols - 8, v - 8, o, o + 8):
            assert call(rng=at) == ERR_ARG and b"rng overlaps" in sslib.ss_last_error_string(), call.__name__
        assert call(rng=s + 8) == ERR_ARG and b"rng overlaps spans" in sslib.ss_last_error_string()
        assert call(rng=g + 4) == ERR_ARG and b"aligned" in sslib.ss_last_error_string()
    assert plan(rng=s + 8) == ERR_ARG and b"rng overlaps spans" in sslib.ss_last_error_string()
    # no masks at all: the spans table has no entries and may be null; the rejection is the other argument's
    assert mask_dev(nt=0, nf=0, spans=None, cols=0) == ERR_ARG and b"cols" in sslib.ss_last_error_string()
    assert host_spans(nt=0, nf=0, spans=None) == 0
    # the host forms' table errors name the first bad clip
    for call in (mask_host, aug_host):
        for bad, where in (([1, 2, 12], b"clip 0"), ([0, 4, 3], b"clip 1"), ([0, 2, 13], b"clip 1")):
            b = np.array(bad, np.int64)
            assert call(ro=b.ctypes.data) == ERR_ARG and where in sslib.ss_last_error_string(), bad
    assert (out == -5.0).all() and (vec == 1.0).all() and rng.tolist() == [2026, 9]  # nothing was written by any of it ...
    assert host_spans() == 0 and not (spans == -7).any()                              # ... until a call was valid


def _has_gpu():
    try:
        import torch

        return torch.cuda.is_available()
    except Exception:
        return False


@pytest.mark.skipif(_has_gpu(), reason="checks the no-device failure mode")
def test_python_front_fails_loudly_without_a_device(sslib):
    import speechsauce_amd as ss
    from speechsauce_amd import SpeechSauceError

    x = np.zeros((6, 13), np.float32)
    for call in (lambda: ss.mask_spans_packed(x, [0, 2, 6], np.zeros((2, 2, 2), np.int32), 1, 1),
                 lambda: ss.spec_augment_packed(x, [0, 2, 6], np.array([1, 0], np.uint64)), lambda: ss.spec_augment_packed(x, [0, 2, 6], (1, 0), out=x)):
        with pytest.raises(SpeechSauceError) as e:
            call()
        assert e.value.status == 4  # SS_ERR_HIP: there is no CPU path


def test_python_front_spans_and_argument_rules(sslib):
    import speechsauce_amd as ss

    for name in ("spec_augment_spans", "mask_spans_packed", "spec_augment_packed", "SpecAugment"):
        assert name in ss.__all__ and hasattr(ss, name)
    ro = _table(LENS)
    want = spans_ref((SEED, 3), 5, ro, int(ro[-1]), 80, 2, 100, 1.0, 2, 27)
    for rng in ((SEED, 3), [SEED, 3], np.array([SEED, 3], np.uint64)):
        got = ss.spec_augment_spans(rng, ro, 80, clip_base=5)  # the defaults are the LibriSpeech policy
        assert got.dtype == np.int32 and got.shape == (len(LENS), 4, 2) and np.array_equal(got, want)
    assert np.array_equal(ss.spec_augment_spans((SEED, 3), list(ro), 13, 1, 10, 0.2, 3, 4, 0), spans_ref((SEED, 3), 0, ro, int(ro[-1]), 13, 1, 10, 0.2, 3, 4))
    bad = [0, 4, 2, 9]
    assert np.array_equal(ss.spec_augment_spans((1, 1), bad, 13, total_rows=8), spans_ref((1, 1), 0, bad, 8, 13, 2, 100, 1.0, 2, 27))
    assert ss.spec_augment_spans((1, 1), [0], 13).shape == (0, 4, 2) and ss.spec_augment_spans((1, 1), ro, 13, 0, freq_masks=0).shape == (len(LENS), 0, 2)
    z = np.zeros((4, 13), np.float32)
    sp = np.zeros((1, 4, 2), np.int32)
    for kw in (dict(time_masks=17), dict(freq_masks=-1), dict(time_width=-1), dict(freq_width=1 << 31), dict(time_ratio=1.5), dict(time_ratio=float("nan")),
               dict(clip_base=-1)):
        with pytest.raises(ValueError):
            ss.spec_augment_spans((1, 0), [0, 4], 13, **kw)
        with pytest.raises(ValueError):
            ss.spec_augment_packed(z, [0, 4], (1, 0), **kw)
    for rng in (None, 5, (1, 2, 3), "ab"):
        with pytest.raises(TypeError):
            ss.spec_augment_spans(rng, [0, 4], 13)
    with pytest.raises(ValueError):
        ss.spec_augment_spans((-1, 0), [0, 4], 13)
    with pytest.raises(ValueError):
        ss.spec_augment_spans((1, 0), [0, 4], 0)
    with pytest.raises(ValueError):
        ss.mask_spans_packed(z, [0, 4], sp, 17, 0)
    with pytest.raises(ValueError):
        ss.mask_spans_packed(z, [0, 4], sp, 2, 1)  # three pairs wanted, four given
    with pytest.raises(TypeError):
        ss.mask_spans_packed(z, [0, 4], sp.astype(np.int64), 2, 2)
    with pytest.raises(TypeError):
        ss.mask_spans_packed(z.astype(np.float64), [0, 4], sp, 2, 2)
    for out in (np.zeros((4, 12), np.float32), np.zeros((4, 13), np.float64), np.zeros((8, 13), np.float32)[::2]):
        with pytest.raises(ValueError):
            ss.mask_spans_packed(z, [0, 4], sp, 2, 2, out=out)
    for bad_off in ([1, 4], [0, 3, 2], [0, 5]):
        with pytest.raises(ValueError):
            ss.mask_spans_packed(z, bad_off, np.zeros((len(bad_off) - 1, 4, 2), np.int32), 2, 2)
    # nothing for the device to do: no clips
    out, spans = ss.spec_augment_packed(np.zeros((0, 13), np.float32), [0], (1, 0))
    assert out.shape == (0, 13) and spans.shape == (0, 4, 2)
    assert ss.mask_spans_packed(np.zeros((0, 13), np.float32), [0, 0], sp, 2, 2).shape == (0, 13)
