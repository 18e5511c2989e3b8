"""The persistent loop of the Kaldi-compatible kernel (ss_kaldi_c256, ss_kaldi512.hip): calls so large that every wave of every
workgroup goes round `while (quad < q_hi)` at least twice more -- the LDS claim, the prefetch into the input registers, the ok_cur /
ok_next hand-over, the packed build's carried clip cursor (offset_seek's steps and its binary search), q_lo / q_hi at a full grid, the
multiply-high frame division -- held to COVERED calls (at most one quad per wave: the regime tests/test_kaldi.py and
tests/test_kaldi_builds.py hold to f64) on the same samples bit for bit, to f64 on sampled clips, and to guard rows around every
output.  tests/test_kaldi_cpu.py::test_loop_test_shapes_reach_the_loop checks the shape arithmetic without a device.

Shapes follow the device's CU count (the library reads the same property): 3 * 12 * CUs + 5 quads and a bit, in clips of 5 frames
(about 7 400 clips of about 1 000 samples on 256 CUs), generated on the device.  The last tests are the small containment cases:
total_frames beyond the tables and entries without rows."""
import numpy as np
import pytest

from test_kaldi import BAR, clip_len
from test_kaldi_builds import SENTINEL, Front
from test_kaldi_cpu import (LOOP_T, SS_ERR_DEVICE, SS_OK, covered_clips, gpu_case_signal, kaldi_grid, loop_dense_clips, loop_packed_frames,
                            packed_chunks, ref_num_frames, ref_sizes, workgroup_quads)

pytestmark = pytest.mark.gpu

# name -> (mfcc, parameters): the first four are the packed cases too
CASES = {
    "ne13_fbank_pow2": (False, dict(num_mel_bins=80)),                                          # with the log energy
    "ne10_mfcc_pow2": (True, dict(frame_length_ms=20.0, num_mel_bins=40, num_ceps=13)),
    "ne16_fbank_magnitude": (False, dict(frame_length_ms=32.0, num_mel_bins=80, use_power=0)),  # flen 512
    "ne13_mfcc_32_cepstra": (True, dict(num_mel_bins=40, num_ceps=32, use_energy=1)),
    "shift_161": (False, dict(num_mel_bins=80, frame_shift_ms=10.0625)),                        # every quad loads single floats
    "odd_ld": (False, dict(num_mel_bins=80)),                                                   # pair and single-float quads alternate
}
PACKED_CASES = list(CASES)[:4]


def cu_count():
    import torch

    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def device_noise(numel, seed):
    import torch

    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    return torch.randn(numel, generator=g, device="cuda", dtype=torch.float32).mul_(0.1)


def boundary_rows(rows, cus):
    """the first and the last row of a few workgroups' [q_lo, q_hi), and of the call"""
    spans = workgroup_quads(-(-rows // 4), cus)
    picked = {0, rows - 1}
    for b in sorted({0, 1, len(spans) // 2, len(spans) - 2, len(spans) - 1}):
        lo, hi = spans[b]
        picked |= {4 * lo, min(4 * hi, rows) - 1}
    return sorted(picked)


def cat_parts(parts):
    import torch

    return [None if parts[0][k] is None else torch.cat([p[k] for p in parts]) for k in (0, 1)]


def same_bits(a, b):
    import torch

    return all(u is None or torch.equal(u, v) for u, v in zip(a, b))


def assert_big_is_the_covered_calls(big, parts):
    """one assertion for both: the big call (made with written=False) equals the covered calls bit for bit, no sentinel is left in it"""
    bits = len(parts) >= 2 and same_bits(cat_parts(parts), big)
    holes = any(t is not None and bool((t == SENTINEL).any()) for t in big)
    assert bits and not holes, f"equal to the covered calls bit for bit: {bits}; rows the big call never wrote: {holes}"


def report(what, front, fig):
    names = ("column 0", "columns 1..") if front.mfcc else ("block metric", "log energy")
    print(f"kaldi loop {what}: {names[0]} {fig[0]:.3g}, {names[1]} {fig[1]:.3g}")
    assert fig[0] <= BAR and fig[1] <= BAR


@pytest.mark.parametrize("case", list(CASES))
def test_dense_loop(ss, sslib, case):
    """(a) the big call is the concatenation of covered calls on consecutive blocks of clips, bit for bit; (b) the first clip, the last
    and those at the ends of a few workgroups' quad ranges meet f64; (c) every output lies between untouched guard rows (Front.dense)
    and holds no sentinel; and, where the rows are contiguous, the same clips as a packed call give the same bytes."""
    cus = cu_count()
    mfcc, cfg = CASES[case]
    front = Front(ss, sslib, mfcc, energy_floor=0.0, **cfg)
    T, B, Bc = LOOP_T, loop_dense_clips(cus), covered_clips(cus)
    L = clip_len(front.cfg, T, extra=6)
    L += L % 2
    ld = L + 1 if case == "odd_ld" else L
    assert ref_num_frames(front.p, L) == ref_num_frames(front.p, ld) == T and ld % 2 == (case == "odd_ld")
    x = device_noise(B * ld, 11).view(B, ld)
    big = front.dense(x.data_ptr(), B, L, ld, written=False)
    assert kaldi_grid(-(-B * T // 4), cus) == cus
    parts = [front.dense(x.data_ptr() + 4 * i * ld, min(Bc, B - i), L, ld) for i in range(0, B, Bc)]
    assert_big_is_the_covered_calls(big, parts)
    worst = [0.0, 0.0]
    for c in sorted({row // T for row in boundary_rows(B * T, cus)}):
        rows = slice(c * T, (c + 1) * T)
        fig = front.figures(big[0][rows], None if big[1] is None else big[1][rows], [x[c, :L].cpu().numpy()])
        worst = [max(w, f) for w, f in zip(worst, fig)]
    report(f"dense {case} ({B} clips of {T} frames, {cus} CUs)", front, worst)
    if ld == L:
        so, fo = np.arange(B + 1, dtype=np.int64) * L, np.arange(B + 1, dtype=np.int64) * T
        assert same_bits(front.packed(x.data_ptr(), so, fo), big) and front.status() == SS_OK


def packed_clips(front, cus, seed):
    """the big packed call's tables: T_b of loop_packed_frames, a few spare samples per clip so that offsets take either parity"""
    flen, shift, _ = ref_sizes(front.p)
    Ts = loop_packed_frames(cus)
    rng = np.random.default_rng(seed)
    lens = np.array([flen + (t - 1) * shift for t in Ts], np.int64) + rng.integers(0, 8, len(Ts))
    assert [ref_num_frames(front.p, int(n)) for n in lens[:200]] == Ts[:200]
    so, fo = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64), np.concatenate([[0], np.cumsum(Ts)]).astype(np.int64)
    assert (so % 2 == 1).sum() > len(Ts) // 4 and (so % 2 == 0).sum() > len(Ts) // 4
    return Ts, so, fo


@pytest.mark.parametrize("case", PACKED_CASES)
def test_packed_loop(ss, sslib, case):
    """Runs of one-frame clips, clips of 1 .. 7 frames and some of about 98: (a) the big packed call is the concatenation of covered
    packed calls on consecutive runs of clips, bit for bit; (c) sampled clips (the ends of workgroups' ranges, a one-frame clip, a
    long one) equal the single-clip dense call bit for bit and meet f64; (d) guards (Front.packed)."""
    cus = cu_count()
    mfcc, cfg = CASES[case]
    front = Front(ss, sslib, mfcc, energy_floor=0.0, **cfg)
    Ts, so, fo = packed_clips(front, cus, 5)
    rows = int(fo[-1])
    sig = device_noise(int(so[-1]), 12)
    big = front.packed(sig.data_ptr(), so, fo, written=False)
    assert front.status() == SS_OK and kaldi_grid(-(-rows // 4), cus) == cus
    runs = packed_chunks(Ts, cus)
    parts = [front.packed(sig.data_ptr() + 4 * int(so[i0]), so[i0:i1 + 1] - so[i0], fo[i0:i1 + 1] - fo[i0]) for i0, i1 in runs]
    assert_big_is_the_covered_calls(big, parts)
    assert front.status() == SS_OK
    sampled = {int(np.searchsorted(fo, row, side="right")) - 1 for row in boundary_rows(rows, cus)}
    sampled |= {Ts.index(1) + 4, int(np.argmax(Ts)), len(Ts) - 1 - int(np.argmax(Ts[::-1]))}
    worst = [0.0, 0.0]
    for c in sorted(sampled):
        lo, hi, n = int(fo[c]), int(fo[c + 1]), int(so[c + 1] - so[c])
        mine = (big[0][lo:hi], None if big[1] is None else big[1][lo:hi])
        assert same_bits(front.dense(sig.data_ptr() + 4 * int(so[c]), 1, n, n), mine), c
        fig = front.figures(mine[0], mine[1], [sig[int(so[c]):int(so[c + 1])].cpu().numpy()])
        worst = [max(w, f) for w, f in zip(worst, fig)]
    report(f"packed {case} ({len(Ts)} clips, {rows} rows, {cus} CUs)", front, worst)


def test_containment_inside_the_loop(ss, sslib):
    """One big packed launch whose frame_offsets entry between two clips in the middle is wrong by one: those two clips keep the
    sentinel, every other row equals the clean launch, the handle reports SS_ERR_DEVICE once.  The kernel skips an inconsistent clip
    before any load: nothing here reads or writes out of range."""
    import torch

    cus = cu_count()
    front = Front(ss, sslib, False, energy_floor=0.0, num_mel_bins=80)
    Ts, so, fo = packed_clips(front, cus, 6)
    sig = device_noise(int(so[-1]), 13)
    clean = front.packed(sig.data_ptr(), so, fo)
    assert front.status() == SS_OK
    m = next(i for i in range(len(Ts) // 2, len(Ts)) if 2 <= Ts[i - 1] <= 7 and 2 <= Ts[i] <= 7)
    bad = fo.copy()
    bad[m] += 1
    got = front.packed(sig.data_ptr(), so, bad, written=False)
    assert front.status() == SS_ERR_DEVICE and front.status() == SS_OK
    lo, hi = int(fo[m - 1]), int(fo[m + 1])
    for g, c in zip(got, clean):
        assert bool((g[lo:hi] == SENTINEL).all())
        assert torch.equal(g[:lo], c[:lo]) and torch.equal(g[hi:], c[hi:])
    assert same_bits(front.packed(sig.data_ptr(), so, fo), clean) and front.status() == SS_OK  # the handle serves the next clean call


# ---- the small containment cases: the few-clip shape of test_kaldi.py::test_packed_containment ------------------------------

def few_clips(front, Ts, lens=None):
    import torch

    lens = lens or [clip_len(front.cfg, T, extra=b) for b, T in enumerate(Ts)]
    clips = [gpu_case_signal(60 + b, n, "unit") for b, n in enumerate(lens)]
    so = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    fo = np.concatenate([[0], np.cumsum(Ts)]).astype(np.int64)
    return torch.from_numpy(np.concatenate(clips)).cuda(), so, fo


def test_total_frames_beyond_the_tables(ss, sslib):
    """total_frames greater than fo[n]: every clip is consistent, so the status stays SS_OK and the clips' rows are the clean call's; the
    trailing rows belong to no clip and keep the sentinel."""
    import torch

    front = Front(ss, sslib, False, energy_floor=0.0, num_mel_bins=80)
    sig, so, fo = few_clips(front, [2, 3, 1, 4, 2])
    rows = int(fo[-1])
    clean = front.packed(sig.data_ptr(), so, fo)
    got = front.packed(sig.data_ptr(), so, fo, rows=rows + 6, written=False)
    assert front.status() == SS_OK
    for g, c in zip(got, clean):
        assert g.shape[0] == rows + 6 and torch.equal(g[:rows], c) and bool((g[rows:] == SENTINEL).all())


@pytest.mark.parametrize("mfcc", [False, True], ids=["fbank", "mfcc"])
@pytest.mark.parametrize("empty", [1, 3])
def test_entries_without_rows(ss, sslib, empty, mfcc):
    """Entries shorter than a frame (fo[b] == fo[b + 1]) between two valid one-frame clips, one and then three in a row -- three inside
    one quad are more than a lane's three steps along the offsets from the quad's first clip.  Each is inconsistent (T == 0): the error
    word is raised; only the inconsistent entry is skipped, so every valid clip's rows are those of the dense call on that clip."""
    front = Front(ss, sslib, mfcc, energy_floor=0.0, num_mel_bins=40)
    flen = ref_sizes(front.p)[0]
    Ts = [1] + [0] * empty + [1, 3]
    lens = [flen + 2] + [7, 120, flen - 1][:empty] + [flen + 1, clip_len(front.cfg, 3, extra=4)]
    sig, so, fo = few_clips(front, Ts, lens)
    assert [ref_num_frames(front.p, n) for n in lens] == Ts
    got = front.packed(sig.data_ptr(), so, fo)  # written: no row of a valid clip may keep the sentinel
    assert front.status() == SS_ERR_DEVICE and front.status() == SS_OK
    for b, T in enumerate(Ts):
        if T:
            lo, hi = int(fo[b]), int(fo[b + 1])
            mine = (got[0][lo:hi], None if got[1] is None else got[1][lo:hi])
            assert same_bits(front.dense(sig.data_ptr() + 4 * int(so[b]), 1, lens[b], lens[b]), mine), b
