"""Post-processing of packed variable-length clips: ss_cmvn_packed*, ss_cmvnw_packed*, ss_power_to_db_packed*, ss_lmfe_packed* and
the Python front's cmvn_packed / cmvnw_packed / power_to_db_packed / lmfe_packed.

Clip b owns rows off[b] .. off[b+1] of one [total_rows x cols] block; per clip every result is what the one-matrix call returns for
that clip alone.  The yardstick is the oracle looped over clips (oracle.cmvn / oracle.cmvnw on block[off[b]:off[b+1]], oracle.mfe +
np.log, the numpy power_to_db formula of tests/test_new_exports.py per clip), metric max abs error over max abs expected, RTOL =
1e-4, over the whole block and per clip.

Conditioning: variance normalisation divides by a window's std and the GPU rounds the mean-subtracted values to f32 between
cmvnw's two passes, so an output of magnitude A carries a relative error of about A * 6e-8.  The parity inputs are seeded normal
data for which the ORACLE's own output stays below 160 in magnitude in every variance case (A * 6e-8 <= 1e-5, a tenth of RTOL);
the tests assert that bound on the oracle side.  Single-row clips and win = 1 give exact zeros with variance normalisation
(0 / (0 + 2^-30)) on both sides and are compared with ==.
"""
import ctypes as C
import re

import numpy as np
import pytest

from common import RTOL, rel

NEW_SYMBOLS = ["ss_cmvn_packed", "ss_cmvnw_packed", "ss_power_to_db_packed", "ss_lmfe_packed",
               "ss_cmvn_packed_device", "ss_cmvnw_packed_device", "ss_power_to_db_packed_device", "ss_lmfe_packed_device"]
ORACLE_BOUND = 160.0
# rows per clip of the parity block: 1, 2, 3, 5 (a 301-row window wraps them many times), 98 / 99 (one second), 301, 1598 (16 s),
# with empty segments between them
ROWS = [98, 0, 1, 2, 0, 0, 3, 5, 99, 301, 0, 1598, 1, 98]


def _power_to_db_ref(S, ref=1.0, amin=1e-10, top_db=80.0):
    """librosa.power_to_db restated, as in tests/test_new_exports.py"""
    S = np.asarray(S, np.float64)
    log_spec = 10.0 * np.log10(np.maximum(amin, S)) - 10.0 * np.log10(np.maximum(amin, abs(ref)))
    if top_db is not None:
        log_spec = np.maximum(log_spec, log_spec.max() - top_db)
    return log_spec


def _table(rows):
    off = np.zeros(len(rows) + 1, dtype=np.int64)
    np.cumsum(np.asarray(rows, dtype=np.int64), out=off[1:])
    return off


def _block(seed, rows, cols):
    return (np.random.default_rng(seed).standard_normal((int(sum(rows)), cols)) * 3 + 1).astype(np.float32)


def _per_clip(fn, block, off):
    """The oracle looped over clips -> f64 block."""
    want = np.zeros(block.shape, dtype=np.float64)
    for b in range(len(off) - 1):
        lo, hi = int(off[b]), int(off[b + 1])
        if hi > lo:
            want[lo:hi] = fn(block[lo:hi])
    return want


def _assert_parity(got, want, off, what):
    """whole block and every clip whose expected output is not all zero; all-zero clips compare with =="""
    got = np.asarray(got)
    assert got.shape == want.shape and got.dtype == np.float32
    errs = {"block": rel(got, want)}
    for b in range(len(off) - 1):
        lo, hi = int(off[b]), int(off[b + 1])
        if hi == lo:
            continue
        if not want[lo:hi].any():
            assert np.all(got[lo:hi] == 0.0), (what, b, "expected exact zeros")
        else:
            errs[b] = rel(got[lo:hi], want[lo:hi])
    worst = max(errs.values())
    print(f"{what}: block {errs['block']:.3e}, worst clip {worst:.3e}")
    assert worst <= RTOL, (what, errs)


# ---------------------------------------------------------------- CPU ---------------------------------------------------------

def test_new_symbols_are_declared_exported_and_prototyped(sslib):
    import os

    from speechsauce_amd import _lib

    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "speechsauce_amd.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in NEW_SYMBOLS:
        assert re.search(r"^int %s\(" % name, header, flags=re.M), f"{name} is not declared in the header"
        assert name in _lib.PROTOTYPES, f"{name} has no ctypes prototype"
        assert getattr(sslib, name, None) is not None, f"{name} is not exported"
    assert sslib.ss_abi_version() == 7
    import speechsauce_amd as ss

    for name in ("cmvn_packed", "cmvnw_packed", "power_to_db_packed", "lmfe_packed"):
        assert callable(getattr(ss, name)) and name in ss.__all__


def _no_device(sslib):
    n = C.c_int(0)
    return sslib.ss_device_count(C.byref(n)) != 0 or n.value == 0


def test_no_clips_is_ok_without_a_device(sslib):
    off = np.zeros(1, dtype=np.int64)
    assert sslib.ss_cmvn_packed(None, 0, off.ctypes.data, 0, 13, 1, None) == 0
    assert sslib.ss_cmvnw_packed(None, 0, off.ctypes.data, 0, 13, 301, 1, None) == 0
    assert sslib.ss_power_to_db_packed(None, 0, off.ctypes.data, 0, 13, 1.0, 1e-10, 80.0, None) == 0
    assert sslib.ss_cmvn_packed_device(None, 0, None, 0, 13, 1, None, None) == 0
    assert sslib.ss_cmvnw_packed_device(None, 0, None, 0, 13, 301, 1, None, None) == 0
    assert sslib.ss_power_to_db_packed_device(None, 0, None, 0, 13, 1.0, 1e-10, 80.0, None, None) == 0
    assert sslib.ss_lmfe_packed(None, None, 0, None, None) == 3  # a null config is an argument error, as for ss_mfe_packed
    assert sslib.ss_lmfe_packed_device(None, None, 0, None, None, 0, None, None, None) == 3


def test_argument_rules_are_decided_before_the_device_is_touched(sslib):
    """Every rejection below is made on the host: the same statuses come back with and without a device.  A valid call without a
    device is SS_ERR_HIP (there is no CPU fallback)."""
    x = np.ones((10, 4), dtype=np.float32)
    out = np.full((10, 4), -5.0, dtype=np.float32)
    xp, op = x.ctypes.data, out.ctypes.data

    def calls(off, total_rows=10, cols=4, win=3, vec=xp, dst=op, table=True):
        t = off.ctypes.data if table else None
        return (sslib.ss_cmvn_packed(vec, off.size - 1, t, total_rows, cols, 1, dst),
                sslib.ss_cmvnw_packed(vec, off.size - 1, t, total_rows, cols, win, 1, dst),
                sslib.ss_power_to_db_packed(vec, off.size - 1, t, total_rows, cols, 1.0, 1e-10, 80.0, dst))

    good = np.array([0, 4, 4, 10], dtype=np.int64)
    assert calls(np.array([1, 4, 10], dtype=np.int64)) == (3, 3, 3)            # off[0] != 0
    assert b"clip 0" in sslib.ss_last_error_string()
    assert calls(np.array([0, 6, 4, 10], dtype=np.int64)) == (3, 3, 3)         # a decreasing pair
    assert b"clip 1" in sslib.ss_last_error_string()
    assert calls(np.array([0, 4, 11], dtype=np.int64)) == (3, 3, 3)            # last entry past total_rows
    assert b"clip 1" in sslib.ss_last_error_string()
    assert calls(good, cols=0) == (3, 3, 3)
    assert calls(good, vec=None) == (3, 3, 3)
    assert calls(good, dst=None) == (3, 3, 3)
    assert calls(good, table=False) == (3, 3, 3)
    assert calls(good, total_rows=1 << 31) == (3, 3, 3)
    assert calls(good, cols=1 << 31) == (3, 3, 3)
    assert sslib.ss_cmvnw_packed(xp, 3, good.ctypes.data, 10, 4, 4, 0, op) == 2        # even window: SS_ERR_BAD_CONFIG
    assert sslib.ss_cmvnw_packed_device(xp, 3, good.ctypes.data, 10, 4, 300, 0, op, None) == 2
    assert sslib.ss_power_to_db_packed(xp, 3, good.ctypes.data, 10, 4, 1.0, 0.0, 80.0, op) == 3   # amin must be > 0
    # the device forms make the same host-side checks (the table itself is the kernels' business)
    assert sslib.ss_cmvn_packed_device(None, 3, good.ctypes.data, 10, 4, 1, op, None) == 3
    assert sslib.ss_cmvn_packed_device(xp, 3, None, 10, 4, 1, op, None) == 3
    assert sslib.ss_cmvn_packed_device(xp, 3, good.ctypes.data, 10, 0, 1, op, None) == 3
    assert sslib.ss_power_to_db_packed_device(xp, 3, good.ctypes.data, 10, 4, 1.0, 1e-10, 80.0, None, None) == 3
    assert np.all(out == -5.0)  # nothing was written by a rejected call
    if _no_device(sslib):
        assert calls(good) == (4, 4, 4)  # SS_ERR_HIP
        assert np.all(out == -5.0)
    # all segments empty: nothing to do, and nothing to do it on
    assert calls(np.zeros(4, dtype=np.int64)) == (0, 0, 0)


def test_python_front_rejects_bad_blocks_and_tables(sslib):
    import speechsauce_amd as ss

    off = np.array([0, 4, 10], dtype=np.int64)
    x64 = np.zeros((10, 4), dtype=np.float64)
    x32 = np.zeros((10, 4), dtype=np.float32)
    for fn in (ss.cmvn_packed, ss.cmvnw_packed, ss.power_to_db_packed):
        with pytest.raises(TypeError):
            fn(x64, off)
        with pytest.raises(TypeError):
            fn(x32, off.astype(np.float32))
        with pytest.raises(ValueError):
            fn(x32, np.array([0, 4, 11], dtype=np.int64))   # ends past the block
        with pytest.raises(ValueError):
            fn(x32, np.array([0, 6, 4, 10], dtype=np.int64))
        with pytest.raises(ValueError):
            fn(x32, np.array([1, 4, 10], dtype=np.int64))
        with pytest.raises(ValueError):
            fn(np.zeros((2, 5, 4), dtype=np.float32), off)
    with pytest.raises(ValueError):
        ss.power_to_db_packed(np.zeros(40, dtype=np.float32), off)           # a flat block needs cols
    with pytest.raises(ValueError):
        ss.power_to_db_packed(np.zeros(41, dtype=np.float32), off, cols=4)   # not a whole number of rows
    with pytest.raises(ValueError):
        ss.power_to_db_packed(x32, off, top_db=-1.0)
    with pytest.raises(TypeError):
        ss.lmfe_packed(np.zeros(16000, dtype=np.float64), [16000], 16000)
    with pytest.raises(TypeError):
        ss.lmfe_packed(np.zeros(16000, dtype=np.float32), [16000.0], 16000)


def test_parity_inputs_are_well_conditioned(oracle):
    """The oracle-side bound the GPU parity tests rely on (they assert it again on the very blocks they use)."""
    for cols in (13, 40, 80):
        block, off = _block(_SEEDS[cols], ROWS, cols), _table(ROWS)
        for win in (3, 31, 301):
            assert np.abs(_per_clip(lambda m: oracle.cmvnw(m, win, True), block, off)).max() < ORACLE_BOUND, (cols, win)
        assert np.abs(_per_clip(lambda m: oracle.cmvn(m, True), block, off)).max() < ORACLE_BOUND


# seeds of the parity blocks, one per width: picked so that the oracle's win = 3 variance case stays below ORACLE_BOUND (asserted
# above and in the parity test itself, so a change of seed cannot hide a failure)
_SEEDS = {13: 102, 40: 105, 80: 111}


# ---------------------------------------------------------------- GPU ---------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("cols", [13, 40, 80])
def test_cmvn_and_cmvnw_parity_per_clip(ss, oracle, cols):
    import torch

    block, off = _block(_SEEDS[cols], ROWS, cols), _table(ROWS)
    d, doff = torch.from_numpy(block).cuda(), torch.from_numpy(off).cuda()
    for var in (False, True):
        want = _per_clip(lambda m: oracle.cmvn(m, var), block, off)
        assert np.abs(want).max() < ORACLE_BOUND
        got = ss.cmvn_packed(d, doff, var)
        torch.cuda.synchronize()
        _assert_parity(got.cpu().numpy(), want, off, f"cmvn cols={cols} var={var}")
        host = ss.cmvn_packed(block, off, var)  # host-pointer form: the same kernels
        assert isinstance(host, np.ndarray) and np.array_equal(host, got.cpu().numpy())
        for win in (1, 3, 31, 301):
            want = _per_clip(lambda m: oracle.cmvnw(m, win, var), block, off)
            assert np.abs(want).max() < ORACLE_BOUND, (cols, win, var)
            got = ss.cmvnw_packed(d, doff, win, var)
            torch.cuda.synchronize()
            _assert_parity(got.cpu().numpy(), want, off, f"cmvnw cols={cols} win={win} var={var}")
            if win in (1, 301):
                assert np.array_equal(ss.cmvnw_packed(block, off, win, var), got.cpu().numpy())
    with pytest.raises(ss.SpeechSauceError) as e:
        ss.cmvnw_packed(d, doff, 300)
    assert e.value.status == 2


@pytest.mark.gpu
def test_packed_calls_reproduce_the_one_matrix_calls(ss):
    """Not an acceptance condition of the design (instruction selection in a new kernel is the compiler's), but the summation
    orders are the same by construction: report whether the bits agree, assert RTOL."""
    import torch

    block, off = _block(7, ROWS, 13), _table(ROWS)
    d, doff = torch.from_numpy(block).cuda(), torch.from_numpy(off).cuda()
    a = ss.cmvn_packed(d, doff, True)
    b = ss.cmvnw_packed(d, doff, 301, True)
    same = {"cmvn": True, "cmvnw": True}
    for k in range(len(ROWS)):
        lo, hi = int(off[k]), int(off[k + 1])
        if hi == lo:
            continue
        one_a, one_b = ss.cmvn(d[lo:hi], True), ss.cmvnw(d[lo:hi], 301, True)
        same["cmvn"] &= bool(torch.equal(a[lo:hi], one_a))
        same["cmvnw"] &= bool(torch.equal(b[lo:hi], one_b))
        if ROWS[k] > 1:
            assert rel(a[lo:hi].cpu().numpy(), one_a.cpu().numpy()) <= RTOL
            assert rel(b[lo:hi].cpu().numpy(), one_b.cpu().numpy()) <= RTOL
    print(f"bit-identical to the one-matrix calls: {same}")


@pytest.mark.gpu
def test_pipeline_on_device_tensors(ss, oracle):
    """mfcc_packed of 1-16 s clips -> cmvn_packed(var) -> extract_derivative_feature, and mel_spectrogram_packed ->
    power_to_db_packed, device tensors end to end with the returned offset tensors, against the per-clip oracle chain on the
    downloaded features."""
    import torch

    rng = np.random.default_rng(31)
    lens = np.concatenate([[16000, 256000, 16160], rng.integers(16000, 256001, 13)]).astype(np.int64)
    x = (rng.standard_normal(int(lens.sum())) * 0.1).astype(np.float32)
    xd = torch.from_numpy(x).cuda()
    feats, fo = ss.mfcc_packed(xd, lens, 16000)
    assert fo.is_cuda
    norm = ss.cmvn_packed(feats, fo, True)
    cube = ss.extract_derivative_feature(norm)
    torch.cuda.synchronize()
    host, off = feats.cpu().numpy(), fo.cpu().numpy()
    want = _per_clip(lambda m: oracle.cmvn(m, True), host, off)
    assert np.abs(want).max() < ORACLE_BOUND
    _assert_parity(norm.cpu().numpy(), want, off, "mfcc_packed -> cmvn_packed(var)")
    got_cube = cube.cpu().numpy()
    assert got_cube.shape == host.shape + (3,)
    for b in range(len(lens)):
        lo, hi = int(off[b]), int(off[b + 1])
        assert rel(got_cube[lo:hi], oracle.extract_derivative_feature(want[lo:hi].astype(np.float32))) <= RTOL, b
    wn = ss.cmvnw_packed(feats, fo, 301, True)
    want_w = _per_clip(lambda m: oracle.cmvnw(m, 301, True), host, off)
    assert np.abs(want_w).max() < ORACLE_BOUND
    _assert_parity(wn.cpu().numpy(), want_w, off, "mfcc_packed -> cmvnw_packed(301, var)")

    # mel (cfg3) -> dB: the flat block of [128 x R_b] pieces, cols = num_filters, offsets = the returned row offsets
    kw = dict(frame_length=0.032, frame_stride=0.032, num_filters=128, fft_length=2048, high_frequency=8000.0)
    gain = np.repeat(10.0 ** rng.uniform(-3, 0, len(lens)), lens).astype(np.float32)  # clips of different loudness
    xg = torch.from_numpy(x * gain).cuda()
    mel, ro = ss.mel_spectrogram_packed(xg, lens, 16000, **kw)
    db = ss.power_to_db_packed(mel, ro, cols=128, top_db=40.0)
    torch.cuda.synchronize()
    mel_h, ro_h, db_h = mel.cpu().numpy(), ro.cpu().numpy(), db.cpu().numpy()
    assert db_h.shape == mel_h.shape
    for b in range(len(lens)):
        lo, hi = 128 * int(ro_h[b]), 128 * int(ro_h[b + 1])
        np.testing.assert_allclose(db_h[lo:hi], _power_to_db_ref(mel_h[lo:hi], top_db=40.0), rtol=0, atol=2e-4, err_msg=str(b))
        assert rel(db_h[lo:hi], _power_to_db_ref(mel_h[lo:hi], top_db=40.0)) <= RTOL


@pytest.mark.gpu
def test_lmfe_packed_against_ln_of_the_oracle_mfe(ss, oracle):
    """lmfe_packed (device and host forms) against ln(oracle.mfe) per clip.

    Conditioning: ln turns the ABSOLUTE f32 error of mfe, a few ulps at the scale of the clip's largest energy (<= 4 * 2^-23 * fmax),
    into an error of that over f for each element, so a clip whose energies span a wide range cannot meet RTOL however good the
    kernel is.  (Measured on the MI355X: white noise alone, whose narrow low filters dip to 1e-6 of the clip's maximum, gives
    2.2e-4 from lmfe_packed AND from the one-clip ss.lmfe, with mfe itself at 1.9e-7 of the maximum.)  The input here is noise
    plus one impulse per frame, a flat floor under every bin: the ORACLE's energies stay within a factor 100 of the clip's maximum
    (asserted), so the ln error is <= 4 * 2^-23 * 100 = 4.8e-5 in absolute terms, half of RTOL * max|ln f| once max|ln f| >= 1
    (asserted)."""
    import torch

    rng = np.random.default_rng(31)
    lens = np.concatenate([[16000, 256000, 16160], rng.integers(16000, 256001, 13)]).astype(np.int64)
    so = _table(lens)
    x = (rng.standard_normal(int(lens.sum())) * 0.02).astype(np.float32)
    for b in range(len(lens)):
        clip = x[so[b]:so[b + 1]]
        clip[np.arange(clip.size) % 320 == 0] += np.float32(4.0)  # frames are 320 samples every 160: exactly one impulse in each
    lf, lfo = ss.lmfe_packed(torch.from_numpy(x).cuda(), lens, 16000)
    torch.cuda.synchronize()
    lf_h, lfo_h = ss.lmfe_packed(x, lens, 16000)
    assert lfo.is_cuda and np.array_equal(lfo.cpu().numpy(), lfo_h) and np.array_equal(lf.cpu().numpy(), lf_h)
    feat, _, fo = ss.mfe_packed(x, lens, 16000)
    assert np.array_equal(fo, lfo_h)
    p = oracle.make_params(sample_rate=16000)
    want = np.zeros(lf_h.shape, dtype=np.float64)
    for b in range(len(lens)):
        f, _ = oracle.mfe(p, x[so[b]:so[b + 1]])
        assert f.min() >= 1e-2 * f.max() and np.abs(np.log(f)).max() >= 1.0, b
        want[lfo_h[b]:lfo_h[b + 1]] = np.log(f)
    _assert_parity(lf_h, want, lfo_h, "lmfe_packed")
    # the ln is the only step after mfe_packed: within 2 ulp of numpy's f32 log of the same energies
    assert np.abs(lf_h - np.log(feat)).max() <= 2 * np.spacing(np.float32(np.abs(lf_h).max()))


@pytest.mark.gpu
def test_position_independence_bit_for_bit(ss):
    """The same clip packed first, last, and between neighbours of other lengths gives identical output bits; two runs of one
    call are identical."""
    import torch

    rng = np.random.default_rng(44)
    for rows_c, cols in ((777, 13), (5000, 40), (2, 13)):
        clip = (rng.standard_normal((rows_c, cols)) * 3 + 1).astype(np.float32)
        power = (clip ** 2 * 10.0 ** rng.uniform(-9, 1, clip.shape)).astype(np.float32)
        layouts = ([rows_c, 98, 1598], [301, 5, rows_c], [1598, 0, 3, rows_c, 0, 98, 4001], [rows_c])
        results = []
        for rows in layouts:
            k = rows.index(rows_c)
            off = _table(rows)
            blk = (np.random.default_rng(len(rows)).standard_normal((int(off[-1]), cols)) * 2).astype(np.float32)
            pw = (blk ** 2 * 1e3).astype(np.float32)  # louder neighbours
            blk[off[k]:off[k + 1]] = clip
            pw[off[k]:off[k + 1]] = power
            d, dp, doff = torch.from_numpy(blk).cuda(), torch.from_numpy(pw).cuda(), torch.from_numpy(off).cuda()
            outs = (ss.cmvn_packed(d, doff, True), ss.cmvnw_packed(d, doff, 301, True), ss.cmvnw_packed(d, doff, 31, False),
                    ss.power_to_db_packed(dp, doff, top_db=30.0))
            again = (ss.cmvn_packed(d, doff, True), ss.cmvnw_packed(d, doff, 301, True), ss.cmvnw_packed(d, doff, 31, False),
                     ss.power_to_db_packed(dp, doff, top_db=30.0))
            torch.cuda.synchronize()
            assert all(torch.equal(a, b) for a, b in zip(outs, again)), "two runs of one call differ"
            results.append([o[int(off[k]):int(off[k + 1])].cpu().numpy() for o in outs])
        for other in results[1:]:
            for name, a, b in zip(("cmvn", "cmvnw(301,var)", "cmvnw(31)", "power_to_db"), results[0], other):
                assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (name, rows_c, cols)


@pytest.mark.gpu
def test_power_to_db_floor_is_per_clip(ss):
    import torch

    rng = np.random.default_rng(52)
    rows = [200, 300]
    off = _table(rows)
    S = (rng.standard_normal((500, 64)) ** 2 * 10.0 ** rng.uniform(-5, 0, (500, 64))).astype(np.float32)
    S[:200] *= 1e-6  # the quiet clip, 60 dB below its neighbour
    d, doff = torch.from_numpy(S).cuda(), torch.from_numpy(off).cuda()
    top_db = 30.0
    got = ss.power_to_db_packed(d, doff, top_db=top_db).cpu().numpy()
    nofloor = ss.power_to_db_packed(d, doff, top_db=None).cpu().numpy()
    whole = ss.power_to_db(d, top_db=top_db).cpu().numpy()
    np.testing.assert_allclose(nofloor, _power_to_db_ref(S, top_db=None), rtol=0, atol=2e-4)
    for b in range(2):
        lo, hi = int(off[b]), int(off[b + 1])
        g = got[lo:hi]
        assert g.min() >= g.max() - top_db                                  # its own floor
        above = nofloor[lo:hi] > np.float32(nofloor[lo:hi].max() - np.float32(top_db))
        assert above.sum() > 100 and np.array_equal(g[above], nofloor[lo:hi][above])  # values above the floor are untouched
        assert np.all(g[~above] == np.float32(nofloor[lo:hi].max()) - np.float32(top_db))
        np.testing.assert_allclose(g, _power_to_db_ref(S[lo:hi], top_db=top_db), rtol=0, atol=2e-4)
    # the unpacked call on the whole block floors the quiet clip at the loud clip's level: every value of it is the floor
    quiet = whole[:200]
    assert quiet.min() == quiet.max() == np.float32(whole.max()) - np.float32(top_db)
    assert got[:200].max() - got[:200].min() > 20.0
    # host form, flat block with cols
    flat = ss.power_to_db_packed(S.reshape(-1), off, cols=64, top_db=top_db)
    assert np.array_equal(flat.reshape(500, 64), got)


@pytest.mark.gpu
def test_bad_device_table_is_contained(ss, sslib, oracle):
    """A table whose middle segment is reversed and whose last segment ends past total_rows: the valid clips are correct, every
    other element keeps the sentinel (guard bands on both sides of the block included), the calls return SS_OK (the table is the
    kernels' business) and the stream synchronises cleanly.  Documented rejection, run once."""
    import torch

    cols, total, pad = 13, 400, 64
    SENT = 12345.0
    block = _block(61, [total], cols)
    # clips 0, 1, 2 valid; 3 reversed (250 -> 180); 4, the last, ends past total_rows
    table = np.array([0, 100, 130, 250, 180, 460], dtype=np.int64)
    valid = [(0, 100), (100, 130), (130, 250)]
    d = torch.from_numpy(block).cuda()
    dt = torch.from_numpy(table).cuda()
    power = torch.from_numpy(block ** 2).cuda()

    def run(fn, src, *scalars):
        buf = torch.full(((total + 2 * pad) * cols,), SENT, device="cuda")
        rc = fn(src.data_ptr(), 5, dt.data_ptr(), total, cols, *scalars, buf[pad * cols:].data_ptr(), None)
        assert rc == 0
        torch.cuda.synchronize()
        h = buf.cpu().numpy()
        assert np.all(h[:pad * cols] == SENT) and np.all(h[-pad * cols:] == SENT)
        return h[pad * cols:-pad * cols].reshape(total, cols)

    for name, fn, src, scalars, ref in (
            ("cmvn", sslib.ss_cmvn_packed_device, d, (1,), lambda m: oracle.cmvn(m, True)),
            ("cmvnw", sslib.ss_cmvnw_packed_device, d, (31, 1), lambda m: oracle.cmvnw(m, 31, True)),
            ("power_to_db", sslib.ss_power_to_db_packed_device, power, (1.0, 1e-10, 80.0),
             lambda m: _power_to_db_ref(m.astype(np.float32) ** 2))):
        body = run(fn, src, *scalars)
        assert np.all(body[250:] == SENT), name          # rows of no valid segment
        for lo, hi in valid:
            assert rel(body[lo:hi], ref(block[lo:hi])) <= RTOL, (name, lo, hi)


@pytest.mark.gpu
def test_graph_capture_replays_on_new_data(ss, sslib, oracle):
    """cmvn_packed + cmvnw_packed(var) captured on one stream (a linear chain of launches and stream-ordered scratch), replayed
    twice on new data in the same buffers."""
    import torch

    rows = [98, 301, 5, 1598, 0, 400]
    off = _table(rows)
    total, cols = int(off[-1]), 13
    x = torch.from_numpy(_block(70, rows, cols)).cuda()
    doff = torch.from_numpy(off).cuda()
    a, b = torch.empty_like(x), torch.empty_like(x)

    def launch(stream):
        st = C.c_void_p(stream.cuda_stream)
        assert sslib.ss_cmvn_packed_device(x.data_ptr(), len(rows), doff.data_ptr(), total, cols, 1, a.data_ptr(), st) == 0
        assert sslib.ss_cmvnw_packed_device(a.data_ptr(), len(rows), doff.data_ptr(), total, cols, 31, 1, b.data_ptr(), st) == 0

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):  # warm-up off the capture
        launch(s)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        launch(torch.cuda.current_stream())
    for seed in (71, 72):
        blk = _block(seed, rows, cols)
        x.copy_(torch.from_numpy(blk).cuda())
        g.replay()
        torch.cuda.synchronize()
        want_a = _per_clip(lambda m: oracle.cmvn(m, True), blk, off)
        _assert_parity(a.cpu().numpy(), want_a, off, f"graph cmvn seed={seed}")
        want_b = _per_clip(lambda m: oracle.cmvnw(m, 31, True), a.cpu().numpy(), off)
        assert np.abs(want_b).max() < ORACLE_BOUND
        _assert_parity(b.cpu().numpy(), want_b, off, f"graph cmvnw seed={seed}")
