"""Noise mixing and gain perturbation of packed clips (ss_noise_*), the part that needs no device: ss_noise_draws against the numpy
restatement (tests/noise_mix_model.py) on every draw field, the header's worked pin, the restatement's own semantics (the SNR it
achieves, its energy order, its fmaf), every argument error of every form, the symbols and the structure in every mirror and the
Python front's argument rules."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest

import noise_mix_model as m

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"ss_noise_draws": 14, "ss_noise_mix_work_bytes": 3, "ss_noise_plan_packed_device": 19, "ss_noise_plan_packed_i16_device": 21,
         "ss_noise_apply_packed_device": 11, "ss_noise_apply_packed": 10, "ss_noise_apply_packed_i16_device": 13, "ss_noise_apply_packed_i16": 12,
         "ss_noise_mix_packed_device": 20, "ss_noise_mix_packed": 17, "ss_noise_mix_packed_i16_device": 22, "ss_noise_mix_packed_i16": 19}
ERR_ARG = 3
SEED = 0x9E3779B97F4A7C15  # both halves of the key are used
LENS = [0, 1, 3, 255, 256, 257, 2047, 2048, 2049, 4097, 40000]
# noise banks: none, one clip, five (among them an empty one), and a table with a reversed clip and one that ends past the bank
BANKS = {0: ([0], 0), 1: ([0, 1000], 1000), 5: ([0, 1, 8, 8, 1008, 51009], 51009), "bad": ([0, 7, 3, 3, 1003, 1010], 1005)}


def _draws(sslib, rng, base, so, total, no, total_noise, prob, snr, gain):
    """ss_noise_draws into a table with a spare row behind it"""
    words = np.array(rng, np.uint64)
    so, no = np.ascontiguousarray(so, np.int64), np.ascontiguousarray(no, np.int64)
    n = len(so) - 1
    plan = np.zeros(n + 1, m.ROW)
    plan[-1] = (-99,) * 8
    rc = sslib.ss_noise_draws(words.ctypes.data, base, n, so.ctypes.data, total, len(no) - 1, no.ctypes.data, total_noise, prob, snr[0], snr[1], gain[0],
                              gain[1], plan.ctypes.data)
    assert rc == 0, sslib.ss_last_error_string()
    assert plan[-1].tolist() == (-99,) * 8 and words.tolist() == [int(v) for v in rng]  # nothing behind the table, the block is read only
    return plan[:-1]


def _same_draws(got, want):
    for f in m.ROW.names:  # the draw fields as bits; the gains and energies stay zero
        assert np.array_equal(np.ascontiguousarray(got[f]).view(np.uint8), np.ascontiguousarray(want[f]).view(np.uint8)), f


def test_draws_equal_the_restatement(sslib):
    so = m.table(LENS)
    total = int(so[-1])
    seen = set()
    for (key, (no, total_noise)), prob, epoch, base in itertools.product(BANKS.items(), (0.0, 0.5, 1.0), (0, 2 ** 32 - 1, 2 ** 32), (0, 5)):
        got = _draws(sslib, (SEED, epoch), base, so, total, no, total_noise, prob, (5.0, 25.5), (-3.0, 6.0))
        want = m.draws_ref((SEED, epoch), base, so, total, no, total_noise, prob, (5.0, 25.5), (-3.0, 6.0))
        _same_draws(got, want)
        mixed = got["noise_clip"] >= 0
        assert (got["noise_clip"][~mixed] == -1).all() and (got["start"][~mixed] == 0).all()
        if prob == 0.0 or key == 0:
            assert not mixed.any()
        if prob == 1.0 and key in (1, 5):  # only the empty noise clip is turned down
            assert (mixed | (want["noise_clip"] == -1)).all() and mixed.sum() >= (len(LENS) if key == 1 else 1)
        lens = np.diff(np.asarray(no))[got["noise_clip"][mixed]]
        assert (lens > 0).all() and (got["start"][mixed] < lens).all() and (got["start"][mixed] >= 0).all()
        assert ((got["snr_db"] >= 5.0) & (got["snr_db"] <= 25.5) & (got["gain_db"] >= -3.0) & (got["gain_db"] <= 6.0)).all()
        seen.update((key, int(c)) for c in got["noise_clip"])
    assert {(5, 0), (5, 1), (5, 3), (5, 4), ("bad", 0), ("bad", 3)} <= seen
    assert not {(5, 2), ("bad", 1), ("bad", 2), ("bad", 4)} & seen  # empty, reversed, (empty,) past the bank's end
    # a range of one value is that value, and gain (0, 0) is exactly 0
    got = _draws(sslib, (SEED, 1), 0, so, total, *BANKS[5], 1.0, (20.0, 20.0), (0.0, 0.0))
    assert (got["snr_db"] == 20.0).all() and (got["gain_db"].view(np.uint32) == 0).all()
    # epochs 2^32 - 1 and 2^32 differ in both counter words; clip_base shifts the ids; both halves of the seed are key words
    a = _draws(sslib, (SEED, 2 ** 32 - 1), 0, so, total, *BANKS[5], 1.0, (10.0, 30.0), (-6.0, 6.0))
    for other in (((SEED, 2 ** 32), 0), ((SEED, 2 ** 32 - 1), 5), ((SEED + 2 ** 32, 2 ** 32 - 1), 0), ((SEED + 1, 2 ** 32 - 1), 0)):
        assert not np.array_equal(a, _draws(sslib, other[0], other[1], so, total, *BANKS[5], 1.0, (10.0, 30.0), (-6.0, 6.0)))


def test_a_shard_draws_what_the_whole_batch_draws(sslib):
    """clips [B, C] at clip_base 1 equal clips 1 and 2 of [A, B, C] at clip_base 0, whatever their offsets"""
    args = ((7, 3), *BANKS[5], 0.5, (10.0, 30.0), (-6.0, 6.0))
    for seed in range(8):
        rng = (seed, 3)
        whole = _draws(sslib, rng, 0, [0, 100, 5000, 5007], 5007, *args[1:])
        shard = _draws(sslib, rng, 1, [0, 4900, 4907], 4907, *args[1:])
        _same_draws(shard, whole[1:])
        alone = _draws(sslib, rng, 2, [3, 10], 10, *args[1:])
        _same_draws(alone, whole[2:])


def test_the_worked_pin(sslib):
    a = m.PIN_ARGS
    want = [(3, 24801, 28.130686, -3.0997949), (0, 4033, 14.968082, -1.3559483), (-1, 0, 11.51598, 4.993896)]
    for got in (m.draws_ref(a["rng"], a["clip_base"], a["so"], a["total"], a["no"], a["total_noise"], a["prob"], a["snr"], a["gain"]),
                _draws(sslib, a["rng"], a["clip_base"], a["so"], a["total"], a["no"], a["total_noise"], a["prob"], a["snr"], a["gain"])):
        assert [(int(r["noise_clip"]), int(r["start"]), r["snr_db"], r["gain_db"]) for r in got] == [(c, s, np.float32(x), np.float32(g)) for c, s, x, g in want]
    header = open(os.path.join(ROOT, "include", "speechsauce_amd.h")).read()
    assert "(3, 24801, 28.130686, -3.0997949) | (0, 4033, 14.968082, -1.3559483) | (-1, 0, 11.51598, 4.993896)" in header


def test_bad_speech_segments_are_marked(sslib):
    #              good | reversed | empty | good | past the end | reversed | reversed, ends below 0 | starts below 0 | good
    bad = np.array([0, 4, 2, 2, 6, 13, 12, -1, 3, 6], np.int64)
    got = _draws(sslib, (7, 1), 0, bad, 12, *BANKS[5], 1.0, (10.0, 30.0), (0.0, 0.0))
    _same_draws(got, m.draws_ref((7, 1), 0, bad, 12, *BANKS[5], 1.0, (10.0, 30.0), (0.0, 0.0)))
    assert [int(c) == -2 for c in got["noise_clip"]] == [b in (1, 4, 5, 6, 7) for b in range(9)]
    assert (got["start"][got["noise_clip"] == -2] == 0).all()
    clean = _draws(sslib, (7, 1), 8, [0, 3], 3, *BANKS[5], 1.0, (10.0, 30.0), (0.0, 0.0))
    _same_draws(clean, got[8:])  # a good clip's draws do not depend on its neighbours


def test_the_restatement_of_the_energy_order():
    """One chunk of 2048 through a scalar loop that follows the header word for word; sizes around the partials and the chunks
    against a scalar loop too; the order matters (the values are chosen so that another order gives other bits)."""
    rng = np.random.default_rng(5)
    for L in (1, 255, 256, 257, 2047, 2048, 2049, 4097):
        v = (rng.standard_normal(L) * 10.0 ** rng.uniform(-3, 3, L)).astype(np.float32)
        total = 0.0
        for k in range(0, L, m.CHUNK):
            sq = [float(np.float64(t) * np.float64(t)) for t in v[k:k + m.CHUNK]]
            p = [0.0] * m.LANES
            for i, s in enumerate(sq):  # lane i % 256 adds its samples in ascending order
                p[i % m.LANES] = p[i % m.LANES] + s
            h = m.LANES // 2
            while h >= 1:
                for lane in range(h):
                    p[lane] = p[lane] + p[lane + h]
                h //= 2
            total = total + p[0]
        assert np.float64(total).view(np.uint64) == np.float64(m.energy(v)).view(np.uint64), L
    differ = 0
    for _ in range(20):  # the order is part of the result: the reversed clip adds the same squares in another order
        v = (rng.standard_normal(4097) * 10.0 ** rng.uniform(-3, 3, 4097)).astype(np.float32)
        differ += m.energy(v) != m.energy(v[::-1])
    assert differ > 0
    assert m.energy(np.zeros(0, np.float32)) == 0.0


def test_the_restatement_reaches_the_drawn_snr():
    """For a mixed clip 10 log10(sum (speech_gain x)^2 / sum (out - speech_gain x)^2) in f64 equals snr_db.  What separates the two:
    the f32 rounding of the two gains (2^-24 relative each, 20 log10(1 + 2^-24) = 5.2e-7 dB) and the rounding of every output sample
    (2^-24 of |out|, random in sign, against a noise term that is 10 .. 30 dB below the speech: it averages out over a clip).
    Measured on this restatement over the 30 clips of the seeds below (257 .. 40000 samples): at most 3.3e-6 dB.  The bar is ten times
    that, 3.3e-5 dB, which is tighter than 0.01 dB."""
    lens = [257, 2047, 2048, 4097, 40000]
    so = m.table(lens)
    total = int(so[-1])
    no, total_noise = [0, 1, 8, 1008, 51009], 51009  # no empty clip: every draw mixes
    worst, mixed = 0.0, 0
    for seed in range(6):
        x = m.speech(lens, seed)
        nz = m.speech([total_noise], 100 + seed, 0.03)
        plan = m.plan_ref(x, (seed, 0), 0, so, total, nz, no, total_noise, 1.0, (10.0, 30.0), (-6.0, 6.0))
        out = m.mix_ref(x, so, total, nz, no, total_noise, plan, np.zeros_like(x))
        for b, row in enumerate(plan):
            assert row["noise_clip"] >= 0 and row["noise_gain"] > 0
            seg = slice(int(so[b]), int(so[b + 1]))
            s = (row["speech_gain"] * x[seg]).astype(np.float64)
            snr = 10.0 * np.log10(np.sum(s ** 2) / np.sum((out[seg].astype(np.float64) - s) ** 2))
            worst, mixed = max(worst, abs(snr - np.float64(row["snr_db"]))), mixed + 1
    print("clips", mixed, "worst |snr - snr_db|", worst, "dB")
    assert mixed == 30 and worst <= 3.3e-5


def test_the_restatement_of_the_mix():
    x = np.arange(1, 11, dtype=np.float32)
    nz = np.array([100.0, 200.0, 300.0, -1.0], np.float32)
    no = [0, 3, 3, 4]
    plan = np.zeros(4, m.ROW)
    plan[0] = (0, 2, 0, 0, 2.0, 0.5, 0, 0)   # noise 300 100 200 300 ..
    plan[1] = (-1, 0, 0, 0, 3.0, 0.0, 0, 0)  # gain alone
    plan[2] = (1, 0, 0, 0, 1.0, 1.0, 0, 0)   # an empty noise clip: not mixed
    plan[3] = (-2, 0, 0, 0, 0.0, 0.0, 0, 0)  # untouched
    out = m.mix_ref(x, [0, 4, 6, 8, 10], 10, nz, no, 4, plan, np.full(10, -7.0, np.float32))
    assert out.tolist() == [152.0, 54.0, 106.0, 158.0, 15.0, 18.0, 7.0, 8.0, -7.0, -7.0]
    plan[0]["start"] = 3  # out of range for a clip of three samples: not mixed
    assert m.mix_ref(x, [0, 4, 6, 8, 10], 10, nz, no, 4, plan, np.zeros(10, np.float32))[:4].tolist() == [2.0, 4.0, 6.0, 8.0]
    assert m.gains(np.float32(0), np.float32(20), 4.0, 1.0, True) == (np.float32(1.0), np.float32(0.2))
    assert m.gains(np.float32(0), np.float32(20), 0.0, 1.0, True)[1] == 0 and m.gains(np.float32(6), np.float32(20), 4.0, 1.0, False)[1] == 0
    assert m.adjacent_f32([1.0, 1.0, 0.0], [np.nextafter(np.float32(1), np.float32(2)), 1.0, -0.0]).all() and not m.adjacent_f32([1.0], [1.000001]).any()


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
        assert "void *stream" in decl.group(1) if name.endswith("_device") else "stream" not in decl.group(1), name
        assert ("x_scale" in decl.group(1) and "noise_scale" in decl.group(1) and "const int16_t *" in decl.group(1)) == ("_i16" in name), name
        assert "double" not in decl.group(1), name  # the dB bounds and prob cross the ABI as floats
        ext = re.search(r"fn %s\((.*?)\)\s*->\s*c_int;" % name, externs, flags=re.S)
        assert ext and len(ext.group(1).split(",")) == arity, name
        assert name in _lib.PROTOTYPES, name
        fn = getattr(sslib, name)  # exported by the library (ss_exports.map lets every ss_* symbol out)
        assert fn.restype is C.c_int and len(fn.argtypes) == len(_lib.PROTOTYPES[name][1]) == arity, name
        assert name.endswith("_device") or name + "(" in hpp, name  # the C++ mirror wraps the host forms
    assert sorted(n for n in _lib.PROTOTYPES if "ss_noise" in n) == sorted(NAMES)
    assert re.search(r"#define SS_ABI_VERSION 7\b", header_text) and sslib.ss_abi_version() == 7 and _lib.ABI_VERSION == 7  # entry points only
    for fn in ("try_noise_draws", "try_noise_mix_work_bytes", "try_noise_apply_packed", "try_noise_apply_packed_i16", "try_noise_mix_packed",
               "try_noise_mix_packed_i16"):
        assert "pub fn %s(" % fn in shim, fn
    for fn in ("noise_plan_packed_device", "noise_plan_packed_i16_device", "noise_apply_packed_device", "noise_apply_packed_i16_device",
               "noise_mix_packed_device", "noise_mix_packed_i16_device"):
        assert "pub unsafe fn %s(" % fn in shim, fn
    mk = open(os.path.join(ROOT, "mfcc-rust_amd", "csrc", "Makefile")).read()
    assert re.search(r"^PLAIN\s*:=.*\bss_noise\b", mk, flags=re.M)


def test_the_plan_row_has_one_layout_in_every_mirror():
    import speechsauce_amd as ss
    from speechsauce_amd import _lib

    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "speechsauce_amd.h")).read(), flags=re.S)
    body = re.search(r"typedef struct ss_noise_plan_row \{(.*?)\} ss_noise_plan_row;", header, flags=re.S).group(1)
    fields = re.findall(r"(\w+)\s+(\w+)\s*;", body)
    assert fields == [("int32_t", "noise_clip"), ("int32_t", "start"), ("float", "snr_db"), ("float", "gain_db"), ("float", "speech_gain"),
                      ("float", "noise_gain"), ("double", "speech_energy"), ("double", "noise_energy")]
    offsets = [0, 4, 8, 12, 16, 20, 24, 32]
    c_kind = {"int32_t": C.c_int32, "float": C.c_float, "double": C.c_double}
    assert [(n, t) for n, t in _lib.SsNoisePlanRow._fields_] == [(n, c_kind[t]) for t, n in fields]
    assert C.sizeof(_lib.SsNoisePlanRow) == 40 and C.alignment(_lib.SsNoisePlanRow) == 8
    np_kind = {"int32_t": np.int32, "float": np.float32, "double": np.float64}
    for dt in (ss.NOISE_PLAN_DTYPE, m.ROW):
        assert dt.itemsize == 40 and list(dt.names) == [n for _, n in fields]
        assert [dt.fields[n][1] for _, n in fields] == offsets and [dt.fields[n][0] for t, n in fields] == [np.dtype(np_kind[t]) for t, _ in fields]
    assert [getattr(_lib.SsNoisePlanRow, n).offset for _, n in fields] == offsets
    shim = open(os.path.join(ROOT, "mfcc-rust_amd", "rust-shim", "src", "lib.rs")).read()
    rs = re.search(r"#\[repr\(C\)\]\s*#\[derive\([^)]*\)\]\s*pub struct NoisePlanRow \{(.*?)\n\}", shim, flags=re.S).group(1)
    rust_kind = {"int32_t": "i32", "float": "f32", "double": "f64"}
    assert re.findall(r"pub (\w+):\s*(\w+)\s*,", rs) == [(n, rust_kind[t]) for t, n in fields]
    hpp = open(os.path.join(ROOT, "include", "speechsauce_amd.hpp")).read()
    assert "using NoisePlanRow = ss_noise_plan_row;" in hpp and "sizeof(NoisePlanRow) == 40 && alignof(NoisePlanRow) == 8" in hpp


def test_work_bytes(sslib):
    n = C.c_size_t(7)
    for clips, total in ((0, 0), (1, 0), (1, 2047), (1, 2048), (16, 16 * 960000), (1024, 10 ** 8), (2 ** 31 - 1, 2 ** 31 - 1)):
        assert sslib.ss_noise_mix_work_bytes(clips, total, C.byref(n)) == 0 and n.value == 16 * (total // 2048 + clips), (clips, total)
    assert sslib.ss_noise_mix_work_bytes(1, 1, None) == ERR_ARG and b"null" in sslib.ss_last_error_string()
    assert sslib.ss_noise_mix_work_bytes(2 ** 31, 1, C.byref(n)) == ERR_ARG and sslib.ss_noise_mix_work_bytes(1, 2 ** 31, C.byref(n)) == ERR_ARG


def test_argument_errors_are_decided_before_the_device_is_touched(sslib):
    """Every call here is rejected (or has nothing to do) on the host: none of the pointers is ever handed to the device, so host
    arrays stand in for device buffers.  On a host without a device a call that got past its checks would return SS_ERR_HIP (4)."""
    total, total_noise = 12, 9
    xs = np.ones(total, np.float32)
    out = np.full(total, -5.0, np.float32)
    bank = np.ones(total_noise, np.float32)
    plan = np.zeros(2, m.ROW)
    plan["noise_clip"] = -7
    work = np.zeros(8, np.float64)  # 16 * (12 // 2048 + 2) = 32 bytes wanted
    rng = np.array([2026, 9], np.uint64)
    so_, no_ = np.array([0, 3, 12], np.int64), np.array([0, 4, 9], np.int64)
    x, o, z, p, w, g, so, no = (a.ctypes.data for a in (xs, out, bank, plan, work, rng, so_, no_))
    S = [0.5, 10.0, 30.0, -6.0, 6.0]

    def sc(kw):
        return [kw.get("prob", S[0]), kw.get("snr_lo", S[1]), kw.get("snr_hi", S[2]), kw.get("gain_lo", S[3]), kw.get("gain_hi", S[4])]

    def head(kw, i16):
        scales = ([kw.get("x_scale", 1.0)], [kw.get("noise_scale", 2.0 ** -15)]) if i16 else ([], [])
        return [kw.get("x", x), *scales[0], kw.get("n", 2), kw.get("so", so), kw.get("total", total), kw.get("bank", z), *scales[1], kw.get("n_noise", 2),
                kw.get("no", no), kw.get("total_noise", total_noise)]

    def draws(**kw):
        return sslib.ss_noise_draws(kw.get("rng", g), kw.get("base", 0), kw.get("n", 2), kw.get("so", so), kw.get("total", total), kw.get("n_noise", 2),
                                    kw.get("no", no), kw.get("total_noise", total_noise), *sc(kw), kw.get("plan", p))

    def form(name, i16, device):
        fn = getattr(sslib, f"ss_noise_{name}_packed{'_i16' if i16 else ''}{'_device' if device else ''}")

        def call(**kw):
            tail = [None] if device else []
            if name == "apply":
                return fn(*head(kw, i16), kw.get("plan", p), kw.get("out", o), *tail)
            scratch = [kw.get("work", w), kw.get("work_bytes", 64)] if device else []
            outs = [kw.get("out", o)] if name == "mix" else []
            return fn(*head(kw, i16), kw.get("rng", g), kw.get("base", 0), *sc(kw), *outs, kw.get("plan", p), *scratch, *tail)

        call.__name__ = fn.__name__
        call.i16, call.device, call.kind = i16, device, name
        return call

    forms = [form("plan", i16, True) for i16 in (False, True)] + [form(k, i16, dev) for k in ("apply", "mix") for i16 in (False, True) for dev in (True, False)]
    assert len(forms) == 10
    assert draws(n=0) == 0 and draws(n=0, prob=7.0, plan=None, so=None) == 0
    for name in ("rng", "so", "plan", "no"):
        assert draws(**{name: None}) == ERR_ARG and b"null" in sslib.ss_last_error_string(), name
    for call in forms + [draws]:
        what = call.__name__
        drawn = call is draws or call.kind in ("plan", "mix")
        if drawn:
            for prob in (-0.001, 1.001, float("nan"), float("inf")):
                assert call(prob=prob) == ERR_ARG and b"prob" in sslib.ss_last_error_string(), (what, prob)
            for kw in (dict(snr_lo=30.5), dict(snr_hi=float("inf")), dict(snr_lo=float("nan")), dict(snr_lo=-float("inf"))):
                assert call(**kw) == ERR_ARG and b"snr_lo_db" in sslib.ss_last_error_string(), (what, kw)
            for kw in (dict(gain_lo=6.5), dict(gain_hi=float("inf")), dict(gain_hi=float("nan"))):
                assert call(**kw) == ERR_ARG and b"gain_lo_db" in sslib.ss_last_error_string(), (what, kw)
            assert call(base=(1 << 32) - 1) == ERR_ARG and call(base=(1 << 32) + 5) == ERR_ARG and call(base=1 << 63) == ERR_ARG, what
            assert b"clip_base" in sslib.ss_last_error_string()
        for name in ("n", "total", "n_noise", "total_noise"):
            assert call(**{name: 1 << 31}) == ERR_ARG and call(**{name: 1 << 40}) == ERR_ARG, (what, name)
    for call in forms:
        what = call.__name__
        assert call(n=0) == 0 and call(n=0, prob=7.0, x=None, plan=None, so=None) == 0, what  # an empty call is SS_OK, whatever else is passed
        names = ("x", "so", "plan", "bank", "no") + (("out",) if call.kind != "plan" else ()) + (("rng",) if call.kind != "apply" else ())
        for name in names + (("work",) if call.device and call.kind != "apply" else ()):
            assert call(**{name: None}) == ERR_ARG and b"null" in sslib.ss_last_error_string(), (what, name)
        # no bank at all: the bank and its table may be null; the rejection is the other argument's
        assert call(n_noise=0, bank=None, no=None, so=None) == ERR_ARG and b"null" in sslib.ss_last_error_string(), what
        assert call(n_noise=0, bank=None, no=None, total=1 << 31) == ERR_ARG and b"2^31" in sslib.ss_last_error_string(), what
        step = 2 if call.i16 else 4
        assert call(x=x + 1) == ERR_ARG and b"aligned" in sslib.ss_last_error_string(), what
        assert call(bank=z + 1) == ERR_ARG and b"aligned" in sslib.ss_last_error_string(), what
        for name in ("so", "no", "plan"):
            assert call(**{name: {"so": so, "no": no, "plan": p}[name] + 4}) == ERR_ARG and b"8-byte" in sslib.ss_last_error_string(), (what, name)
        if call.i16:
            for kw in (dict(x_scale=3.0), dict(noise_scale=0.0), dict(x_scale=float("nan")), dict(noise_scale=2.0 ** 65)):
                assert call(**kw) == ERR_ARG and b"power of two" in sslib.ss_last_error_string(), (what, kw)
        if call.kind != "apply":
            assert call(rng=g + 4) == ERR_ARG and b"8-byte" in sslib.ss_last_error_string(), what
            assert call(rng=x) == ERR_ARG and b"rng overlaps" in sslib.ss_last_error_string(), what
            assert call(rng=p + 8) == ERR_ARG and b"rng overlaps plan" in sslib.ss_last_error_string(), what
            if call.device:
                assert call(work_bytes=31) == ERR_ARG and b"work_bytes" in sslib.ss_last_error_string(), what
                assert call(work=w + 4) == ERR_ARG and b"8-byte" in sslib.ss_last_error_string(), what
                assert call(work=p) == ERR_ARG and b"work overlaps plan" in sslib.ss_last_error_string(), what
                assert call(work=x + 8) == ERR_ARG and b"work overlaps" in sslib.ss_last_error_string(), what
        if call.kind != "plan":
            assert call(out=o + 2) == ERR_ARG and b"aligned" in sslib.ss_last_error_string(), what
            # out == x is in place for the float form alone (that call gets past the overlap rule and fails on the null table)
            if call.i16:
                assert call(out=x) == ERR_ARG and b"partly overlaps" in sslib.ss_last_error_string(), what
            else:
                assert call(out=x, so=None) == ERR_ARG and b"null" in sslib.ss_last_error_string(), what
            for shift in (4, step * (total - 1) // 4 * 4, -4, -4 * (total - 1)):  # out is 4-byte aligned; the samples span step * total bytes
                assert call(out=x + shift) == ERR_ARG and b"partly overlaps" in sslib.ss_last_error_string(), (what, shift)
            for name, at in (("bank", o + 4), ("plan", o), ("plan", o + 8), ("bank", o - step * (total_noise - 1))):
                assert call(**{name: at}) == ERR_ARG and name.encode() + b" overlaps" in sslib.ss_last_error_string(), (what, name)
        for name, at in (("bank", x + step), ("plan", x), ("plan", x + 8)):
            assert call(**{name: at}) == ERR_ARG and name.encode() + b" overlaps" in sslib.ss_last_error_string(), (what, name)
        assert call(plan=z + 8) == ERR_ARG and b"plan overlaps bank" in sslib.ss_last_error_string(), what
        if not call.device:  # the host forms' table errors name the first bad clip, and hold the bank's table to the same rules
            for bad, where in (([1, 2, 12], b"clip 0"), ([0, 4, 3], b"clip 1"), ([0, 2, 13], b"clip 1")):
                t = np.array(bad, np.int64)
                assert call(so=t.ctypes.data) == ERR_ARG and where in sslib.ss_last_error_string(), bad
            for bad, where in (([1, 4, 9], b"noise_offsets[0]"), ([0, 5, 4], b"noise clip 1"), ([0, 4, 10], b"total_noise")):
                t = np.array(bad, np.int64)
                assert call(no=t.ctypes.data) == ERR_ARG and where in sslib.ss_last_error_string(), bad
    assert (out == -5.0).all() and (xs == 1.0).all() and rng.tolist() == [2026, 9] and (plan["noise_clip"] == -7).all() and not work.any()  # nothing was written ...
    assert draws(n_noise=0, no=None) == 0 and (plan["noise_clip"] == -1).all()  # without a bank its table may be null
    assert draws() == 0 and not (plan["noise_clip"] == -7).any()                                                                            # ... until a call was valid


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

    x, bank = np.zeros(6, np.float32), np.ones(5, np.float32)
    plan = np.zeros(2, ss.NOISE_PLAN_DTYPE)
    for call in (lambda: ss.noise_mix_packed(x, [2, 4], bank, [5], np.array([1, 0], np.uint64)), lambda: ss.noise_apply_packed(x, [2, 4], bank, [5], plan),
                 lambda: ss.noise_mix_packed(x.astype(np.int16), [2, 4], bank.astype(np.int16), [5], (1, 0), pcm_scale=1.0, noise_pcm_scale=0.5)):
        with pytest.raises(SpeechSauceError) as e:
            call()
        assert e.value.status == 4  # SS_ERR_HIP: there is no CPU path


def test_python_front_draws_and_argument_rules(sslib):
    import speechsauce_amd as ss

    for name in ("NOISE_PLAN_DTYPE", "noise_plan_rows", "noise_draws", "noise_plan_packed", "noise_apply_packed", "noise_mix_packed", "NoiseMix"):
        assert name in ss.__all__ and hasattr(ss, name)
    bank_lens = np.diff(BANKS[5][0])
    want = m.draws_ref((SEED, 3), 5, m.table(LENS), sum(LENS), *BANKS[5], 0.5, (10.0, 30.0), (0.0, 0.0))
    for rng in ((SEED, 3), [SEED, 3], np.array([SEED, 3], np.uint64)):
        got = ss.noise_draws(rng, LENS, bank_lens, prob=0.5, clip_base=5)  # the defaults: 10 .. 30 dB, no gain perturbation
        assert got.dtype == ss.NOISE_PLAN_DTYPE and got.shape == (len(LENS),)
        _same_draws(got, want)
    bad = [0, 4, 2, 9]
    _same_draws(ss.noise_draws((1, 1), None, None, 1.0, (0, 5), (-1, 1), sample_offsets=bad, noise_offsets=BANKS["bad"][0], total_samples=8, total_noise=1005),
                m.draws_ref((1, 1), 0, bad, 8, *BANKS["bad"], 1.0, (0.0, 5.0), (-1.0, 1.0)))
    assert ss.noise_draws((1, 1), [], bank_lens).shape == (0,) and (ss.noise_draws((1, 1), LENS, [])["noise_clip"] == -1).all()
    x, bank = np.zeros(4, np.float32), np.ones(5, np.float32)
    for kw in (dict(prob=1.5), dict(prob=float("nan")), dict(snr_db=(30, 10)), dict(gain_db=(0, float("inf"))), dict(clip_base=-1), dict(clip_base=2 ** 32 + 1)):
        with pytest.raises(ValueError):
            ss.noise_draws((1, 0), [4], [5], **kw)
        with pytest.raises(ValueError):
            ss.noise_mix_packed(x, [4], bank, [5], (1, 0), **kw)
    for kw in (dict(snr_db=10), dict(gain_db=(1, 2, 3)), dict(snr_db="ab")):
        with pytest.raises(TypeError):
            ss.noise_draws((1, 0), [4], [5], **kw)
    for rng in (None, 5, (1, 2, 3), "ab"):
        with pytest.raises(TypeError):
            ss.noise_draws(rng, [4], [5])
    with pytest.raises(ValueError):
        ss.noise_draws((1, 0), [4], [5], sample_offsets=[0, 4])  # lengths or a table, not both
    with pytest.raises(TypeError):
        ss.noise_mix_packed(x.astype(np.float64), [4], bank, [5], (1, 0))
    with pytest.raises(TypeError):
        ss.noise_mix_packed(x, [4], bank.astype(np.int16), [5], (1, 0))
    with pytest.raises(ValueError):  # no mixed float / PCM form
        ss.noise_mix_packed(x, [4], bank.astype(np.int16), [5], (1, 0), noise_pcm_scale=1.0)
    with pytest.raises(ValueError):
        ss.noise_mix_packed(x.astype(np.int16), [4], bank.astype(np.int16), [5], (1, 0), pcm_scale=3.0, noise_pcm_scale=1.0)
    with pytest.raises(ValueError):
        ss.noise_mix_packed(x, [5], bank, [5], (1, 0))  # the lengths sum past the signal
    with pytest.raises(ValueError):
        ss.noise_mix_packed(x, [4], bank, [6], (1, 0))
    with pytest.raises(ValueError):
        ss.noise_mix_packed(x, [4], bank, [5], (1, 0), device_tables=np.array([0, 4]))  # device tables go with a device signal
    for out in (np.zeros(5, np.float32), np.zeros(4, np.float64), np.zeros(8, np.float32)[::2]):
        with pytest.raises(ValueError):
            ss.noise_mix_packed(x, [4], bank, [5], (1, 0), out=out)
    with pytest.raises(ValueError):
        ss.noise_apply_packed(x, [4], bank, [5], np.zeros(2, ss.NOISE_PLAN_DTYPE))  # one row per clip
    with pytest.raises(TypeError):
        ss.noise_plan_packed(x, [4], bank, [5], (1, 0))  # the plan alone is a device call
    # nothing for the device to do: no clips
    out, plan = ss.noise_mix_packed(np.zeros(0, np.float32), [], bank, [5], (1, 0))
    assert out.shape == (0,) and plan.shape == (0,) and plan.dtype == ss.NOISE_PLAN_DTYPE
    assert ss.noise_apply_packed(np.zeros(0, np.float32), [], bank, [5], plan).shape == (0,)
    rows = ss.noise_plan_rows(np.zeros((3, 5), np.int64))
    assert rows.shape == (3,) and rows.dtype == ss.NOISE_PLAN_DTYPE
