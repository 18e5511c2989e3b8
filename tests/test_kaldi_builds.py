"""Every build of the Kaldi-compatible kernel (ss_kaldi_c256<NE[,pow2],fbank|mfcc[,v]>, ss_kaldi512.hip: NE 10 / 13 / 16 x power /
magnitude x fbank / MFCC x dense / packed = 24) against the numpy f64 restatement of tests/test_kaldi_cpu.py, at the smallest and the
largest frame length of every NE class, on mel banks away from the defaults, on poisoned LDS, in a captured graph and on a side stream.

The calls go through the C ABI (``Front``): the Python front cannot ask for a magnitude MFCC, and every output here lies between guard
rows of a sentinel.  Bars: those of tests/test_kaldi.py (1e-4: block metric of an fbank block, MFCC column 0 and columns 1.. against
their own maxima, log energy against max|want|), on its three-row batch (unit, scaled, int16; energy_floor = 0); bit-for-bit
assertions have no tolerance.  Calls here are COVERED calls (at most one quad per wave); tests/test_kaldi_loop.py runs the loop."""
import ctypes as C

import numpy as np
import pytest

from test_kaldi import BAR, LN_EPS, batch_of_kinds, clip_len, energy_metric
from test_kaldi_cpu import (FRAME_LENGTHS, SS_OK, block_metric, kp, lib_sizes, make_kaldi_params, ref_bank, ref_fbank, ref_mfcc,
                            ref_num_frames, ref_sizes)

pytestmark = pytest.mark.gpu
SENTINEL = -7777.0
GUARD_ROWS = 8


class Guarded:
    """[rows (x cols)] of the sentinel between GUARD_ROWS guard rows in front and behind; the library is handed the interior."""

    def __init__(self, rows, cols=None):
        import torch

        self.full = torch.full((rows + 2 * GUARD_ROWS,) + ((cols,) if cols else ()), SENTINEL, dtype=torch.float32, device="cuda")
        self.rows = rows
        self.inner = self.full[GUARD_ROWS:GUARD_ROWS + rows]

    def check(self, written=True):
        """the guards are untouched; written: no interior value is the sentinel"""
        assert bool((self.full[:GUARD_ROWS] == SENTINEL).all()), "a write in front of the output block"
        assert bool((self.full[GUARD_ROWS + self.rows:] == SENTINEL).all()), "a write behind the output block"
        if written:
            assert not bool((self.inner == SENTINEL).any()), "an output value was never written"


class Front:
    """One ss_kaldi_config and its calls through the C ABI, outputs in guarded buffers.  fbank calls always ask for the log energy."""

    def __init__(self, ss, sslib, mfcc, **cfg):
        self.lib, self.mfcc, self.cfg = sslib, mfcc, cfg
        self.p = kp(**cfg)
        self.config = ss.KaldiConfig(make_kaldi_params(sslib, **cfg))  # raises on any status but SS_OK
        self.cols = int(self.p["num_ceps"] if mfcc else self.p["num_mel_bins"])

    def buffers(self, rows):
        return Guarded(rows, self.cols), (None if self.mfcc else Guarded(rows))

    def status(self):
        return self.lib.ss_kaldi_config_device_status(self.config.handle)

    def launch_dense(self, x_ptr, batch, L, ld, out, en, stream=None):
        h, s = self.config.handle, C.c_void_p(stream) if stream else None
        if self.mfcc:
            return self.lib.ss_kaldi_mfcc_device(h, x_ptr, batch, L, ld, out.inner.data_ptr(), s)
        return self.lib.ss_kaldi_fbank_device(h, x_ptr, batch, L, ld, out.inner.data_ptr(), en.inner.data_ptr(), s)

    def launch_packed(self, x_ptr, n, dso, dfo, rows, out, en, stream=None):
        h, s = self.config.handle, C.c_void_p(stream) if stream else None
        if self.mfcc:
            return self.lib.ss_kaldi_mfcc_packed_device(h, x_ptr, n, dso.data_ptr(), dfo.data_ptr(), rows, out.inner.data_ptr(), s)
        return self.lib.ss_kaldi_fbank_packed_device(h, x_ptr, n, dso.data_ptr(), dfo.data_ptr(), rows, out.inner.data_ptr(), en.inner.data_ptr(), s)

    def dense(self, x_ptr, batch, L, ld, written=True):
        """x [batch x ld] at x_ptr -> (rows [batch * T x cols], log energy [batch * T] or None), guards checked; written: and no
        sentinel left inside (False: the caller looks with `holes`)"""
        import torch

        out, en = self.buffers(batch * ref_num_frames(self.p, L))
        assert self.launch_dense(x_ptr, batch, L, ld, out, en) == SS_OK, self.lib.ss_last_error_string()
        torch.cuda.synchronize()
        for g in (out, en):
            if g is not None:
                g.check(written)
        return out.inner, (None if en is None else en.inner)

    def packed(self, x_ptr, so, fo, rows=None, written=True):
        """packed clips at x_ptr, host tables so / fo (int64, used as they stand) -> as dense(); rows: total_frames (default fo[-1])"""
        import torch

        rows = int(fo[-1]) if rows is None else rows
        out, en = self.buffers(rows)
        dso, dfo = torch.from_numpy(np.ascontiguousarray(so, np.int64)).cuda(), torch.from_numpy(np.ascontiguousarray(fo, np.int64)).cuda()
        assert self.launch_packed(x_ptr, len(so) - 1, dso, dfo, rows, out, en) == SS_OK, self.lib.ss_last_error_string()
        torch.cuda.synchronize()
        for g in (out, en):
            if g is not None:
                g.check(written)
        return out.inner, (None if en is None else en.inner)

    def kernel(self):
        return self.lib.ss_last_kernel_name().decode()

    def figures(self, got, got_e, clips):
        """worst figures of the rows of `clips` (a list of sample arrays, rows in that order) against f64: fbank -> (block metric, log
        energy), MFCC -> (column 0, columns 1..)"""
        got = got.cpu().numpy()
        got_e = None if got_e is None else got_e.cpu().numpy()
        a = b = 0.0
        row = 0
        for x in clips:
            T = ref_num_frames(self.p, len(x))
            g = got[row:row + T]
            if self.mfcc:
                want = ref_mfcc(x, self.p)
                a = max(a, block_metric(g[:, 0], want[:, 0]))
                if self.cols > 1:
                    b = max(b, block_metric(g[:, 1:], want[:, 1:]))
            else:
                want, want_e = ref_fbank(x, self.p)
                a = max(a, block_metric(g, want))
                b = max(b, energy_metric(got_e[row:row + T], want_e))
            row += T
        assert row == got.shape[0]
        return a, b


# ---- 1. the build matrix ---------------------------------------------------------------------------------------------------

BUILDS = {"pow2,fbank": (False, 1), "fbank": (False, 0), "pow2,mfcc": (True, 1), "mfcc": (True, 0)}  # tag -> (mfcc, use_power)
# what the launcher reports, typed out from its SS_KN macro: (NE, build) -> (dense, packed)
NAMES = {
    (10, "pow2,fbank"): ("ss_kaldi_c256<10,pow2,fbank>", "ss_kaldi_c256<10,pow2,fbank,v>"),
    (10, "fbank"): ("ss_kaldi_c256<10,fbank>", "ss_kaldi_c256<10,fbank,v>"),
    (10, "pow2,mfcc"): ("ss_kaldi_c256<10,pow2,mfcc>", "ss_kaldi_c256<10,pow2,mfcc,v>"),
    (10, "mfcc"): ("ss_kaldi_c256<10,mfcc>", "ss_kaldi_c256<10,mfcc,v>"),
    (13, "pow2,fbank"): ("ss_kaldi_c256<13,pow2,fbank>", "ss_kaldi_c256<13,pow2,fbank,v>"),
    (13, "fbank"): ("ss_kaldi_c256<13,fbank>", "ss_kaldi_c256<13,fbank,v>"),
    (13, "pow2,mfcc"): ("ss_kaldi_c256<13,pow2,mfcc>", "ss_kaldi_c256<13,pow2,mfcc,v>"),
    (13, "mfcc"): ("ss_kaldi_c256<13,mfcc>", "ss_kaldi_c256<13,mfcc,v>"),
    (16, "pow2,fbank"): ("ss_kaldi_c256<16,pow2,fbank>", "ss_kaldi_c256<16,pow2,fbank,v>"),
    (16, "fbank"): ("ss_kaldi_c256<16,fbank>", "ss_kaldi_c256<16,fbank,v>"),
    (16, "pow2,mfcc"): ("ss_kaldi_c256<16,pow2,mfcc>", "ss_kaldi_c256<16,pow2,mfcc,v>"),
    (16, "mfcc"): ("ss_kaldi_c256<16,mfcc>", "ss_kaldi_c256<16,mfcc,v>"),
}
SEEN = set()  # the names test_build_matrix met; test_all_24_builds_ran reads it

MATRIX = [(fid, build, 13) for fid in FRAME_LENGTHS for build in BUILDS] + \
         [(fid, build, 32) for fid in ("320", "400", "512") for build in ("pow2,mfcc", "mfcc")]  # beyond 16 cepstra: one frame length per class


def build_front(ss, sslib, fid, build, n_ceps=13, **more):
    sr, fl_ms, _, _, _ = FRAME_LENGTHS[fid]
    mfcc, use_power = BUILDS[build]
    cfg = dict(sample_rate=sr, frame_length_ms=fl_ms, use_power=use_power, energy_floor=0.0)
    if mfcc:  # beyond 16 cepstra column 0 is the log energy
        cfg.update(num_mel_bins=40, num_ceps=n_ceps, use_energy=int(n_ceps > 16))
    else:  # a handle for the fbank calls alone, as the Python front makes them
        cfg.update(num_mel_bins=80, num_ceps=0)
    cfg.update(more)
    return Front(ss, sslib, mfcc, **cfg)


def three_rows(front, T, seed):
    """the three-row batch with T frames a row and an ODD row length -> (x [3 x L], the rows in an even-stride device block, ld)"""
    import torch

    L = clip_len(front.cfg, T, extra=3)
    L += 1 - L % 2
    x = batch_of_kinds(seed, L)
    assert ref_num_frames(front.p, L) == T
    wide = torch.zeros((3, L + 1), dtype=torch.float32, device="cuda")
    wide[:, :L] = torch.from_numpy(x).cuda()
    return x, wide, L + 1


@pytest.mark.parametrize("fid,build,n_ceps", MATRIX)
def test_build_matrix(ss, sslib, fid, build, n_ceps):
    """Per frame length and build, T in {1, 5, 9} frames a row: the dense call (even row stride: sample pairs) and the packed call on the
    same clips (odd row length: the middle clip starts at an odd offset and loads single floats) report the names of the table, meet
    f64 at the bars, and the packed rows are the dense rows bit for bit."""
    import torch

    sr, fl_ms, flen, shift, NE = FRAME_LENGTHS[fid]
    front = build_front(ss, sslib, fid, build, n_ceps)
    assert lib_sizes(sslib, front.config.params) == (SS_OK, (flen, shift, 512)) and ref_sizes(front.p) == (flen, shift, 512)
    worst = [0.0, 0.0]
    for T in (1, 5, 9):
        x, wide, ld = three_rows(front, T, 1000 * int(fid) + T)
        L = x.shape[1]
        got, got_e = front.dense(wide.data_ptr(), 3, L, ld)
        name = front.kernel()
        assert name == NAMES[(NE, build)][0], name
        SEEN.add(name)
        sig = torch.from_numpy(x.reshape(-1)).cuda()
        so, fo = np.arange(4, dtype=np.int64) * L, np.arange(4, dtype=np.int64) * T
        assert so[1] % 2 == 1
        pk, pk_e = front.packed(sig.data_ptr(), so, fo)
        name = front.kernel()
        assert name == NAMES[(NE, build)][1], name
        SEEN.add(name)
        assert front.status() == SS_OK
        assert torch.equal(pk, got) and (got_e is None or torch.equal(pk_e, got_e)), T
        for i, fig in enumerate(front.figures(got, got_e, list(x))):
            worst[i] = max(worst[i], fig)
    what = ("column 0", "columns 1..") if front.mfcc else ("block metric", "log energy")
    print(f"kaldi build <{NE},{build}> flen {flen} cepstra {n_ceps if front.mfcc else '-'}: {what[0]} {worst[0]:.3g}, {what[1]} {worst[1]:.3g}")
    assert worst[0] <= BAR and worst[1] <= BAR


# ---- 2. bank shapes --------------------------------------------------------------------------------------------------------

BANKS = {"3_bins": dict(num_mel_bins=3), "16_bins": dict(num_mel_bins=16), "17_bins": dict(num_mel_bins=17), "79_bins": dict(num_mel_bins=79),
         "80_bins_20_1000": dict(num_mel_bins=80, low_freq=20.0, high_freq=1000.0), "40_bins_high_-400": dict(num_mel_bins=40, high_freq=-400.0),
         "80_bins_300_3400": dict(num_mel_bins=80, low_freq=300.0, high_freq=3400.0)}


@pytest.mark.parametrize("build", ["pow2,fbank", "pow2,mfcc"])
@pytest.mark.parametrize("bank", list(BANKS))
def test_bank_shapes(ss, sslib, bank, build):
    """flen 400, T = 5, banks from 3 filters (one spans 198 bins) to a band so narrow that filters stay empty: the handle is created
    (no header-valid bank may be SS_ERR_UNSUPPORTED), the rows meet f64 at the bars, an empty filter's column is ln eps."""
    M = BANKS[bank]["num_mel_bins"]
    front = build_front(ss, sslib, "400", build, **BANKS[bank], **(dict(num_ceps=min(13, M)) if BUILDS[build][0] else {}))
    x, wide, ld = three_rows(front, 5, 4000 + M)
    got, got_e = front.dense(wide.data_ptr(), 3, x.shape[1], ld)
    a, b = front.figures(got, got_e, list(x))
    empty = np.flatnonzero((ref_bank(front.p).astype(np.float32) == 0).all(axis=1))
    print(f"kaldi bank {bank} <13,{build}>: {a:.3g}, {b:.3g}; {len(empty)} empty filters")
    if bank == "80_bins_20_1000":
        assert len(empty) == 19
        if not front.mfcc:
            np.testing.assert_allclose(got.cpu().numpy()[:, empty], LN_EPS, rtol=0, atol=2e-6)
    else:
        assert len(empty) == 0
    assert a <= BAR and b <= BAR


# ---- 5. poisoned LDS, a captured graph, a side stream -----------------------------------------------------------------------

def test_uninitialised_lds_never_reaches_kaldi_results(ss, sslib, sslab):
    """The idiom of test_gpu_sweep.py::test_uninitialised_lds_never_reaches_results on the twelve dense builds and four packed ones:
    the call, ss_debug_poison_lds (every CU's LDS full of 0xFFFFFFFF), the call again -- finite and bit-identical."""
    import torch

    def twice(fn):
        first = fn()
        assert sslab.ss_debug_poison_lds(None) == 0
        second = fn()
        for u, v in zip(first, second):
            if u is not None:
                assert bool(torch.isfinite(v).all()) and torch.equal(u, v)

    packed_too = {("320", "pow2,fbank"), ("400", "mfcc"), ("512", "pow2,mfcc"), ("512", "fbank")}
    names = set()
    for fid in ("320", "400", "512"):
        for build in BUILDS:
            front = build_front(ss, sslib, fid, build, 32 if fid == "400" else 13)
            x, wide, ld = three_rows(front, 5, 77)
            L = x.shape[1]
            twice(lambda: front.dense(wide.data_ptr(), 3, L, ld))
            names.add(front.kernel())
            if (fid, build) in packed_too:
                sig = torch.from_numpy(x.reshape(-1)).cuda()
                twice(lambda: front.packed(sig.data_ptr(), np.arange(4, dtype=np.int64) * L, np.arange(4, dtype=np.int64) * 5))
                names.add(front.kernel())
    assert len(names) == 16


def test_graph_capture_and_side_stream(ss, sslib):
    """The handles first (creation uploads the tables), then ss_kaldi_fbank_device followed by ss_kaldi_mfcc_packed_device captured in
    one straight-line graph: two replays on fresh inputs copied into the captured buffers, and the same two calls on a side stream,
    equal the calls on the default stream bit for bit."""
    import torch

    fb = build_front(ss, sslib, "400", "pow2,fbank")
    mf = build_front(ss, sslib, "320", "pow2,mfcc")
    T = 6
    L = clip_len(fb.cfg, T, extra=2)
    Ts = [1, 3, 2, 5]
    lens = [clip_len(mf.cfg, t, extra=1 + b) for b, t in enumerate(Ts)]
    so, fo = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64), np.concatenate([[0], np.cumsum(Ts)]).astype(np.int64)
    assert any(int(o) % 2 for o in so[1:-1])
    dso, dfo = torch.from_numpy(so).cuda(), torch.from_numpy(fo).cuda()
    x = torch.zeros((3, L), dtype=torch.float32, device="cuda")
    sig = torch.zeros(int(so[-1]), dtype=torch.float32, device="cuda")

    def fresh(seed):
        x.copy_(torch.from_numpy(batch_of_kinds(seed, L)))
        sig.copy_(torch.from_numpy(batch_of_kinds(seed + 50, int(so[-1]))[seed % 3]))

    def pair(stream):
        o1, e1 = fb.buffers(3 * T)
        o2, _ = mf.buffers(int(fo[-1]))
        assert fb.launch_dense(x.data_ptr(), 3, L, L, o1, e1, stream) == SS_OK
        assert mf.launch_packed(sig.data_ptr(), len(Ts), dso, dfo, int(fo[-1]), o2, None, stream) == SS_OK
        return o1, e1, o2

    def same(a, b):
        for u, v in zip(a, b):
            u.check()
            v.check()
            assert torch.equal(u.full, v.full)

    fresh(1)
    eager = pair(None)  # (also the first launch of both builds: nothing of a launch's set-up is left for the capture)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        on_side = pair(side.cuda_stream)
    side.synchronize()
    same(on_side, eager)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        captured = pair(torch.cuda.current_stream().cuda_stream)
    for seed in (2, 3):
        fresh(seed)
        for buf in captured:
            buf.full.fill_(SENTINEL)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        eager = pair(None)
        torch.cuda.synchronize()
        same(captured, eager)
    assert fb.status() == SS_OK and mf.status() == SS_OK


def test_all_24_builds_ran():
    """test_build_matrix, which runs before this in the file, has met every name of the table."""
    assert SEEN == {name for pair in NAMES.values() for name in pair} and len(SEEN) == 24
