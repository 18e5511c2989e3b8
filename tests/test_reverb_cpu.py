"""The host side of the reverberation stage (ss_reverb_* of include/speechsauce_amd.h), no device needed: the draws against the numpy
restatement (tests/reverb_model.py), the bank's normalisation, peaks, limits and partition spectra, every argument error of every
form, and the symbols and the plan row in the header, the library, the C++ mirror, the ctypes table and the Rust shim.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import reverb_model as m

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"ss_reverb_bank_create": 7, "ss_reverb_bank_info": 5, "ss_reverb_bank_rir": 6, "ss_reverb_bank_spectrum": 4, "ss_reverb_draws": 8,
         "ss_reverb_plan_packed_device": 9, "ss_reverb_apply_packed_device": 8, "ss_reverb_apply_packed": 7, "ss_reverb_apply_packed_i16_device": 9,
         "ss_reverb_apply_packed_i16": 8, "ss_reverb_packed_device": 11, "ss_reverb_packed": 10, "ss_reverb_packed_i16_device": 12,
         "ss_reverb_packed_i16": 11}
ERR_ARG = 3
SEED = 0x9E3779B97F4A7C15  # both halves of the key are used


def _bank(sslib, hs, normalize=1, align=1):
    """-> (handle, return code); the caller destroys the handle"""
    packed = np.concatenate([np.asarray(h, np.float32) for h in hs] + [np.zeros(0, np.float32)])
    off = m.table([len(h) for h in hs])
    h = C.c_void_p()
    rc = sslib.ss_reverb_bank_create(packed.ctypes.data, len(hs), off.ctypes.data, packed.size, normalize, align, C.byref(h))
    return h, rc


def _rir(sslib, h, c):
    n, peak = C.c_size_t(), C.c_size_t()
    assert sslib.ss_reverb_bank_rir(h, c, None, 0, C.byref(n), C.byref(peak)) == 0
    taps = np.empty(n.value, np.float32)
    assert sslib.ss_reverb_bank_rir(h, c, taps.ctypes.data, taps.size, C.byref(n), C.byref(peak)) == 0
    return taps, peak.value


@pytest.fixture(scope="module")
def pin_bank(sslib):
    hs = []
    for c, p in enumerate(m.PIN_PEAKS):
        h = (np.random.default_rng(c).standard_normal(200) * 0.1).astype(np.float32)
        h[p] = 1.0
        hs.append(h)
    h, rc = _bank(sslib, hs)
    assert rc == 0
    yield h
    sslib.ss_reverb_bank_destroy(h)


def _draws(sslib, bank, rng, base, so, total, prob):
    so = np.asarray(so, np.int64)
    plan = np.zeros(len(so) - 1, m.ROW)
    plan["rir"] = -9
    words = np.array(rng, np.uint64)
    rc = sslib.ss_reverb_draws(words.ctypes.data, base, len(plan), so.ctypes.data, total, bank, prob, plan.ctypes.data)
    assert rc == 0, sslib.ss_last_error_string()
    return plan


def test_draws_equal_the_restatement(sslib, pin_bank):
    lens = [0, 1, 511, 512, 5000, 16000, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3]
    so = m.table(lens)
    seen = set()
    for prob in (0.0, 0.5, 1.0):
        for epoch in (0, 2 ** 32 - 1, 2 ** 32):
            for base in (0, 5):
                got = _draws(sslib, pin_bank, (SEED, epoch), base, so, int(so[-1]), prob)
                assert got.tobytes() == m.draws_ref((SEED, epoch), base, so, int(so[-1]), m.PIN_PEAKS, prob).tobytes(), (prob, epoch, base)
                assert (prob > 0.0 or (got["rir"] == -1).all()) and (prob < 1.0 or (got["rir"] >= 0).all())
                seen.update(got["rir"].tolist())
    assert seen == {-1, 0, 1, 2, 3, 4}  # every response and the copy are drawn somewhere


def test_a_shard_draws_what_the_whole_batch_draws(sslib, pin_bank):
    whole = _draws(sslib, pin_bank, (SEED, 7), 0, m.table([300, 4000, 77]), 4377, 0.5)
    shard = _draws(sslib, pin_bank, (SEED, 7), 1, m.table([4000, 77]), 4077, 0.5)
    assert shard.tobytes() == whole[1:].tobytes()


def test_the_worked_pin(sslib, pin_bank):
    header = open(os.path.join(ROOT, "include", "speechsauce_amd.h")).read()
    got = _draws(sslib, pin_bank, (2026, 0), 0, m.table([16000] * 3), 48000, 0.5)
    assert [tuple(int(v) for v in r) for r in got] == m.PIN_ROWS
    assert " | ".join("(%d, %d)" % r for r in m.PIN_ROWS) in header and "0x30000" in header


def test_bad_speech_segments_are_marked(sslib, pin_bank):
    so = [5, 100, 90, 200, 300]  # clip 1 is reversed, clip 3 ends past the block
    got = _draws(sslib, pin_bank, (1, 1), 0, so, 250, 1.0)
    assert got["rir"][1] == -2 and got["rir"][3] == -2 and got["shift"][1] == 0 and (got["rir"][[0, 2]] >= 0).all()
    assert _draws(sslib, pin_bank, (1, 1), 0, [-1, 4], 250, 1.0)["rir"][0] == -2
    assert got.tobytes() == m.draws_ref((1, 1), 0, so, 250, m.PIN_PEAKS, 1.0).tobytes()


def test_normalisation_peaks_and_limits(sslib):
    r = np.random.default_rng(3)
    tie = np.array([0.25, -0.5, 0.5, 0.1, -0.5], np.float32)  # the first of three equal magnitudes wins
    first = np.array([-2.0, 1.0, 0.5], np.float32)
    last = np.array([0.1, 0.2, -0.9], np.float32)
    long_ = (r.standard_normal(m.MAX_TAPS) * 0.01).astype(np.float32)
    one = np.array([-0.3], np.float32)
    hs = [tie, first, last, long_, one, np.zeros(4, np.float32)]
    for mode in (0, 1, 2):
        h, rc = _bank(sslib, hs, mode, 1)
        assert rc == 0, sslib.ss_last_error_string()
        info = [C.c_size_t() for _ in range(4)]
        assert sslib.ss_reverb_bank_info(h, *(C.byref(v) for v in info)) == 0
        assert [v.value for v in info] == [len(hs), m.B, m.MAX_TAPS, sum(-(-len(x) // m.B) for x in hs)]
        for c, src in enumerate(hs):
            taps, peak = _rir(sslib, h, c)
            want, want_peak = m.normalise(src, mode)
            assert peak == want_peak and np.array_equal(taps.view(np.uint32), np.asarray(want, np.float32).view(np.uint32)), (mode, c)
        assert [_rir(sslib, h, c)[1] for c in range(3)] == [1, 0, 2]
        if mode == 1:
            assert abs(float(np.sum(_rir(sslib, h, 3)[0].astype(np.float64) ** 2)) - 1.0) < 1e-6
        if mode == 2:
            assert np.abs(_rir(sslib, h, 2)[0]).max() == 1.0
        sslib.ss_reverb_bank_destroy(h)
    # the shift of a row: the peak with align_peak, 0 without
    for align, want in ((1, 2), (0, 0)):
        h, rc = _bank(sslib, [last], 1, align)
        assert rc == 0 and _draws(sslib, h, (1, 1), 0, [0, 10], 10, 1.0)[0].tolist() == (0, want)
        sslib.ss_reverb_bank_destroy(h)
    # limits: 16385 taps, an empty and a reversed entry, a tap that is not finite, the scalars
    h, rc = _bank(sslib, [np.ones(m.MAX_TAPS + 1, np.float32)])
    assert rc == ERR_ARG and not h and b"response 0" in sslib.ss_last_error_string() and b"16385" in sslib.ss_last_error_string()
    h, rc = _bank(sslib, [one, np.zeros(0, np.float32), one])
    assert rc == ERR_ARG and b"response 1" in sslib.ss_last_error_string()
    packed, hh = np.ones(8, np.float32), C.c_void_p()
    for off, what in (([0, 5, 3, 8], b"response 1"), ([0, 4, 9], b"response 1"), ([1, 4], b"rir_offsets[0]")):
        off = np.array(off, np.int64)
        assert sslib.ss_reverb_bank_create(packed.ctypes.data, len(off) - 1, off.ctypes.data, 8, 1, 1, C.byref(hh)) == ERR_ARG and not hh
        assert what in sslib.ss_last_error_string(), off
    h, rc = _bank(sslib, [one, np.array([1.0, np.inf], np.float32)])
    assert rc == ERR_ARG and b"response 1" in sslib.ss_last_error_string() and b"finite" in sslib.ss_last_error_string()
    off = np.array([0, 8], np.int64)
    for kw in (dict(normalize=3), dict(normalize=-1), dict(align=2), dict(align=-1)):
        assert sslib.ss_reverb_bank_create(packed.ctypes.data, 1, off.ctypes.data, 8, kw.get("normalize", 1), kw.get("align", 1), C.byref(hh)) == ERR_ARG
    assert sslib.ss_reverb_bank_create(None, 1, off.ctypes.data, 8, 1, 1, C.byref(hh)) == ERR_ARG and b"null" in sslib.ss_last_error_string()
    assert sslib.ss_reverb_bank_create(packed.ctypes.data, 1, None, 8, 1, 1, C.byref(hh)) == ERR_ARG
    assert sslib.ss_reverb_bank_create(packed.ctypes.data, 1, off.ctypes.data, 8, 1, 1, None) == ERR_ARG
    assert sslib.ss_reverb_bank_create(packed.ctypes.data, 1 << 26, off.ctypes.data, 8, 1, 1, C.byref(hh)) == ERR_ARG
    # an empty bank is a bank: nothing is ever drawn from it
    h, rc = _bank(sslib, [])
    assert rc == 0 and (_draws(sslib, h, (1, 1), 0, [0, 10, 20], 20, 1.0)["rir"] == -1).all()
    sslib.ss_reverb_bank_destroy(h)
    sslib.ss_reverb_bank_destroy(None)


def test_partition_spectra_against_numpy(sslib):
    r = np.random.default_rng(11)
    hs = [np.array([1.0], np.float32), (r.standard_normal(m.B) * 0.2).astype(np.float32), (r.standard_normal(m.B + 1) * 0.2).astype(np.float32),
          m.response(3000, 1500, 1), m.response(m.MAX_TAPS, 8000, 2)]
    h, rc = _bank(sslib, hs)
    assert rc == 0
    out = np.empty(2 * m.N, np.float32)
    for c, src in enumerate(hs):
        taps, _ = _rir(sslib, h, c)
        parts = -(-len(src) // m.B)
        for p in range(parts):
            assert sslib.ss_reverb_bank_spectrum(h, c, p, out.ctypes.data) == 0
            want = m.spectrum_ref(taps, p)
            assert np.abs(out.view(np.complex64) - want).max() <= 1e-6 * np.abs(want).max(), (c, p)
        assert sslib.ss_reverb_bank_spectrum(h, c, parts, out.ctypes.data) == ERR_ARG and b"partition" in sslib.ss_last_error_string()
    assert sslib.ss_reverb_bank_spectrum(h, len(hs), 0, out.ctypes.data) == ERR_ARG and sslib.ss_reverb_bank_spectrum(h, 0, 0, None) == ERR_ARG
    n = C.c_size_t()
    assert sslib.ss_reverb_bank_rir(h, len(hs), None, 0, C.byref(n), C.byref(n)) == ERR_ARG and b"outside the bank" in sslib.ss_last_error_string()
    assert sslib.ss_reverb_bank_rir(h, 3, out.ctypes.data, 2999, C.byref(n), C.byref(n)) == ERR_ARG and b"cap" in sslib.ss_last_error_string()
    assert sslib.ss_reverb_bank_rir(h, 3, None, 0, None, C.byref(n)) == ERR_ARG and sslib.ss_reverb_bank_rir(None, 0, None, 0, C.byref(n), C.byref(n)) == ERR_ARG
    assert sslib.ss_reverb_bank_info(h, None, C.byref(n), C.byref(n), C.byref(n)) == ERR_ARG
    sslib.ss_reverb_bank_destroy(h)


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
        assert ("x_scale" in decl.group(1) and "const int16_t *" in decl.group(1)) == ("_i16" in name), name
        assert "double" not in decl.group(1), name
        ext = re.search(r"fn %s\((.*?)\)\s*->\s*c_int;" % name, externs, flags=re.S)
        assert ext and len(ext.group(1).split(",")) == arity, name
        assert name in _lib.PROTOTYPES, name
        fn = getattr(sslib, name)  # exported by the library (ss_exports.map lets every ss_* symbol out)
        assert fn.restype is C.c_int and len(fn.argtypes) == len(_lib.PROTOTYPES[name][1]) == arity, name
        assert name.endswith("_device") or name + "(" in hpp, name  # the C++ mirror wraps the host forms
    assert re.search(r"^void ss_reverb_bank_destroy\(ss_reverb_bank \*bank\);", header, flags=re.M) and "ss_reverb_bank_destroy" in hpp
    assert re.search(r"fn ss_reverb_bank_destroy\(bank: \*mut c_void\);", externs) and sslib.ss_reverb_bank_destroy.restype is None
    assert sorted(n for n in _lib.PROTOTYPES if "ss_reverb" in n) == sorted(list(NAMES) + ["ss_reverb_bank_destroy"])
    assert re.search(r"#define SS_ABI_VERSION 7\b", header_text) and sslib.ss_abi_version() == 7 and _lib.ABI_VERSION == 7  # entry points only
    for fn in ("new", "info", "rir", "spectrum", "draws", "apply_packed", "apply_packed_i16", "packed", "packed_i16"):
        assert re.search(r"impl ReverbBank \{.*?pub fn %s\(" % fn, shim, flags=re.S), fn
    for fn in ("plan_packed_device", "apply_packed_device", "apply_packed_i16_device", "packed_device", "packed_i16_device"):
        assert re.search(r"impl ReverbBank \{.*?pub unsafe fn %s\(" % fn, shim, flags=re.S), fn
    mk = open(os.path.join(ROOT, "mfcc-rust_amd", "csrc", "Makefile")).read()
    assert re.search(r"^KERNELS\s*:=.*\bss_reverb\b", mk, flags=re.M) and re.search(r"^HDRS\s*:=.*\bss_reverb\.h\b", mk, flags=re.M)


def test_the_plan_row_has_one_layout_in_every_mirror():
    import speechsauce_amd as ss

    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "speechsauce_amd.h")).read(), flags=re.S)
    body = re.search(r"typedef struct ss_reverb_plan_row \{(.*?)\} ss_reverb_plan_row;", header, flags=re.S).group(1)
    assert re.findall(r"(\w+)\s+(\w+)\s*;", body) == [("int32_t", "rir"), ("int32_t", "shift")]
    for dt in (ss.REVERB_PLAN_DTYPE, m.ROW):
        assert dt.itemsize == 8 and list(dt.names) == ["rir", "shift"] and [dt.fields[n] for n in dt.names] == [(np.dtype(np.int32), 0), (np.dtype(np.int32), 4)]
    shim = open(os.path.join(ROOT, "mfcc-rust_amd", "rust-shim", "src", "lib.rs")).read()
    rs = re.search(r"#\[repr\(C\)\]\s*#\[derive\([^)]*\)\]\s*pub struct ReverbPlanRow \{(.*?)\n\}", shim, flags=re.S).group(1)
    assert re.findall(r"pub (\w+):\s*(\w+)\s*,", rs) == [("rir", "i32"), ("shift", "i32")]
    hpp = open(os.path.join(ROOT, "include", "speechsauce_amd.hpp")).read()
    assert "using ReverbPlanRow = ss_reverb_plan_row;" in hpp and "sizeof(ReverbPlanRow) == 8" in hpp


def test_argument_errors_are_decided_before_the_device_is_touched(sslib, pin_bank):
    """Every call here is rejected (or has nothing to do) on the host: none of the pointers is ever handed to the device, so host
    arrays stand in for device buffers.  On a host without a device a call that got past its checks would return SS_ERR_HIP (4)."""
    total = 12
    xs = np.ones(total + 1, np.float32)
    out = np.full(total + 1, -5.0, np.float32)
    plan = np.zeros(3, m.ROW)
    rng = np.array([2026, 9, 0], np.uint64)
    so_ = np.array([0, 3, 12, 0], np.int64)
    x, o, p, g, so = (a.ctypes.data for a in (xs, out, plan, rng, so_))

    def draws(**kw):
        return sslib.ss_reverb_draws(kw.get("rng", g), kw.get("base", 0), kw.get("n", 2), kw.get("so", so), kw.get("total", total), kw.get("bank", pin_bank),
                                     kw.get("prob", 0.5), kw.get("plan", p))

    def plan_device(**kw):
        return sslib.ss_reverb_plan_packed_device(kw.get("n", 2), kw.get("so", so), kw.get("total", total), kw.get("bank", pin_bank), kw.get("rng", g),
                                                  kw.get("base", 0), kw.get("prob", 0.5), kw.get("plan", p), None)

    plan_device.kind, plan_device.i16, plan_device.device = "plan", False, True

    def form(name, i16, device):
        fn = getattr(sslib, f"ss_reverb_{name}packed{'_i16' if i16 else ''}{'_device' if device else ''}")

        def call(**kw):
            head = [kw.get("x", x), *([kw.get("x_scale", 2.0 ** -15)] if i16 else []), kw.get("n", 2), kw.get("so", so), kw.get("total", total),
                    kw.get("bank", pin_bank)]
            tail = [None] if device else []
            if name == "apply_":
                return fn(*head, kw.get("plan", p), kw.get("out", o), *tail)
            return fn(*head, kw.get("rng", g), kw.get("base", 0), kw.get("prob", 0.5), kw.get("out", o), kw.get("plan", p), *tail)

        call.__name__ = fn.__name__
        call.i16, call.device, call.kind = i16, device, name
        return call

    forms = [form(k, i16, dev) for k in ("apply_", "") for i16 in (False, True) for dev in (True, False)]
    assert len(forms) == 8
    assert draws(n=0) == 0 and draws(n=0, prob=7.0, plan=None, so=None, bank=None) == 0
    for name in ("rng", "so", "plan", "bank"):
        assert draws(**{name: None}) == ERR_ARG and b"null" in sslib.ss_last_error_string(), name
    for call in forms + [plan_device, draws]:
        what = call.__name__
        if call is draws or call.kind != "apply_":
            for prob in (-0.001, 1.001, float("nan"), float("inf")):
                assert call(prob=prob) == ERR_ARG and b"prob" in sslib.ss_last_error_string(), (what, prob)
            assert call(base=(1 << 32) - 1) == ERR_ARG and call(base=(1 << 32) + 5) == ERR_ARG and call(base=1 << 63) == ERR_ARG, what
            assert b"clip_base" in sslib.ss_last_error_string()
        for name in ("n", "total"):
            assert call(**{name: 1 << 31}) == ERR_ARG and call(**{name: 1 << 40}) == ERR_ARG, (what, name)
            assert b"2^31" in sslib.ss_last_error_string()
    for call in forms + [plan_device]:
        what = call.__name__
        assert call(n=0) == 0 and call(n=0, prob=7.0, x=None, plan=None, so=None, bank=None) == 0, what  # an empty call is SS_OK, whatever else is passed
        names = ("so", "plan", "bank") + (("x", "out") if call.kind != "plan" else ()) + (("rng",) if call.kind != "apply_" else ())
        for name in names:
            assert call(**{name: None}) == ERR_ARG and b"null" in sslib.ss_last_error_string(), (what, name)
        # alignment: the table, the plan and rng to 8 bytes, the samples and out to their element
        for name, base_ptr in (("so", so), ("plan", p)) + ((("rng", g),) if call.kind != "apply_" else ()):
            assert call(**{name: base_ptr + 4}) == ERR_ARG and b"8-byte" in sslib.ss_last_error_string(), (what, name)
        if call.kind != "plan":
            assert call(out=o + 2) == ERR_ARG and b"aligned" in sslib.ss_last_error_string(), what
            assert call(x=x + (1 if call.i16 else 2)) == ERR_ARG and b"aligned" in sslib.ss_last_error_string(), what
            # overlaps: out on the samples (in place, or partly), the plan or rng on either
            assert call(out=x) == ERR_ARG and b"in place" in sslib.ss_last_error_string(), what
            assert call(out=x + 4 * 4) == ERR_ARG and call(x=o + (total - 1) * 4) == ERR_ARG, what
            assert call(plan=x + 8) == ERR_ARG and b"plan overlaps" in sslib.ss_last_error_string(), what
            assert call(plan=o + 4 * 10) == ERR_ARG and b"plan overlaps" in sslib.ss_last_error_string(), what
            if call.kind != "apply_":
                assert call(rng=x + 8) == ERR_ARG and b"rng overlaps" in sslib.ss_last_error_string(), what
                assert call(rng=p + 8) == ERR_ARG and b"rng overlaps plan" in sslib.ss_last_error_string(), what
        if call.i16:
            for scale in (0.0, -1.0, 3.0, float("nan"), float("inf"), 2.0 ** 65):
                assert call(x_scale=scale) == ERR_ARG and b"power of two" in sslib.ss_last_error_string(), (what, scale)
        if not call.device:  # the host forms check the table first
            for table, msg in (([1, 3, 12], b"offsets[0]"), ([0, 5, 3], b"clip 1"), ([0, 3, 13], b"clip 1")):
                t = np.array(table, np.int64)
                assert call(so=t.ctypes.data) == ERR_ARG and msg in sslib.ss_last_error_string(), (what, table)
    assert (out == -5.0).all() and (xs == 1.0).all() and int(rng[1]) == 9


def _has_gpu():
    try:
        import torch

        return torch.cuda.is_available()
    except Exception:
        return False


@pytest.mark.skipif(_has_gpu(), reason="checks the no-device failure mode")
def test_python_front_fails_loudly_without_a_device(sslib):
    import speechsauce_amd as ss

    bank = ss.ReverbBank(np.ones(3, np.float32), [3])
    with pytest.raises(ss.SpeechSauceError, match="no usable HIP device"):
        ss.reverb_packed(np.ones(10, np.float32), [10], bank, (1, 0))
    with pytest.raises(ss.SpeechSauceError, match="no usable HIP device"):
        ss.reverb_apply_packed(np.ones(10, np.float32), [10], bank, np.zeros(1, m.ROW))


def test_python_front_bank_draws_and_argument_rules(sslib):
    import speechsauce_amd as ss

    hs = [m.response(k, p, i) for i, (k, p) in enumerate(zip(m.RIR_LENS, m.RIR_PEAKS))]
    packed, lens = np.concatenate(hs), [h.size for h in hs]
    bank = ss.ReverbBank(packed, lens)
    assert (len(bank), bank.block, bank.max_taps, bank.n_partitions) == (len(hs), m.B, 3000, sum(-(-k // m.B) for k in lens))
    for c, (h, p) in enumerate(zip(hs, m.RIR_PEAKS)):
        taps, peak = bank.rir(c)
        assert peak == p == bank.shift(c) and np.array_equal(taps, m.normalise(h, 1)[0])
    flat = ss.ReverbBank(packed, lens, normalize="none", align_peak=False)
    assert flat.shift(6) == 0 and np.array_equal(flat.rir(6)[0], hs[6])
    spec = bank.spectrum(6, 5)
    assert spec.dtype == np.complex64 and np.abs(spec - m.spectrum_ref(bank.rir(6)[0], 5)).max() <= 1e-6 * np.abs(spec).max()
    want = m.draws_ref((9, 4), 2, m.table([100, 0, 50]), 150, m.RIR_PEAKS, 0.5)
    assert ss.reverb_draws((9, 4), [100, 0, 50], bank, 0.5, 2).tobytes() == want.tobytes()
    assert ss.reverb_draws(np.array([9, 4], np.uint64), None, bank, 0.5, 2, sample_offsets=[0, 100, 100, 150]).tobytes() == want.tobytes()
    assert ss.reverb_plan_rows(want.view(np.int32).reshape(-1, 2)).tobytes() == want.tobytes()
    x = np.ones(150, np.float32)
    with pytest.raises(ValueError, match="prob"):
        ss.reverb_draws((1, 0), [3], bank, 1.5)
    with pytest.raises(ValueError, match="clip_base"):
        ss.reverb_draws((1, 0), [3], bank, 0.5, -1)
    with pytest.raises(TypeError, match="ReverbBank"):
        ss.reverb_draws((1, 0), [3], packed, 0.5)
    with pytest.raises(ValueError, match="not both"):
        ss.reverb_draws((1, 0), [3], bank, 0.5, sample_offsets=[0, 3])
    with pytest.raises(ValueError, match="not in place"):
        ss.reverb_packed(x, [150], bank, (1, 0), out=x)
    with pytest.raises(ValueError, match="one row per clip"):
        ss.reverb_apply_packed(x, [100, 50], bank, np.zeros(3, m.ROW))
    with pytest.raises(ValueError, match="normalize"):
        ss.ReverbBank(packed, lens, normalize="rms")
    with pytest.raises(TypeError, match="float32"):
        ss.ReverbBank(packed.astype(np.float64), lens)
    with pytest.raises(ss.SpeechSauceError, match="response 1"):
        ss.ReverbBank(np.ones(m.MAX_TAPS + 2, np.float32), [1, m.MAX_TAPS + 1])
    with pytest.raises(TypeError, match="ReverbBank"):
        ss.Reverb(1, packed)
    assert ss.reverb_packed(np.zeros(0, np.float32), [], bank, (1, 0))[1].size == 0  # nothing to do: no device needed
