"""The NeMo / Parakeet log-mel front end on the device (ss_nemo_c256 and ss_nemo_norm_kernel, ss_nemo512.hip) against the numpy f64
restatement of the header's specification in tests/nemo_model.py.

Bars: block metric max|got - want| / max|want| <= 1e-4 (the project's) for a clip's rows, raw and normalised; the normalisation stage
on its own within 2^-22 * max(1, |out|) per element of the f64 restatement of step 8 on the device's own log-mel rows (one f32
rounding plus slack for an f32 divide).  Every parity test prints the largest figure it met; tests/test_nemo_cpu.py prints the f32
restatement's figures on the same inputs.  Inputs: seeded noise at 0.1.  Clip lengths: every edge case of the loader (nemo_model.GPU_LENS)."""
import ctypes as C
from functools import lru_cache

import numpy as np
import pytest

import nemo_model as nm
from test_nemo_cpu import BAR, SS_ERR_ARG, SS_ERR_DEVICE, SS_OK, make_nemo_params

pytestmark = pytest.mark.gpu
SENTINEL = -7777.0


@lru_cache(maxsize=None)
def want(L, n_mels, normalize, W=400, c=nm.PREEMPH):
    """the f64 restatement on gpu_clip(L): computed once, shared, never written"""
    out = nm.features(nm.gpu_clip(L), n_mels, normalize, W, c)
    out.setflags(write=False)
    return out


def dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def packed(clips):
    return np.concatenate(clips), [len(c) for c in clips]


@pytest.mark.parametrize("n_mels", nm.GPU_BANDS)
def test_log_mel_parity(ss, n_mels):
    worst = {}
    for L in nm.GPU_LENS:
        got = ss.nemo_log_mel(dev(nm.gpu_clip(L)), n_mels=n_mels, normalize=None).cpu().numpy()
        assert got.shape == (L // 160, n_mels)
        worst[L] = nm.block_metric(got, want(L, n_mels, False))
    print(f"nemo log-mel, {n_mels} bands: " + ", ".join(f"{L}: {m:.3g}" for L, m in worst.items()))
    assert max(worst.values()) <= BAR


@pytest.mark.parametrize("n_mels", nm.GPU_BANDS)
def test_normalised_parity(ss, n_mels):
    worst = {}
    for L in nm.GPU_LENS:
        if L // 160 >= 2:
            got = ss.nemo_log_mel(dev(nm.gpu_clip(L)), n_mels=n_mels).cpu().numpy()
            worst[L] = nm.block_metric(got, want(L, n_mels, True))
    print(f"nemo normalised, {n_mels} bands: " + ", ".join(f"{L}: {m:.3g}" for L, m in worst.items()))
    assert max(worst.values()) <= BAR


@pytest.mark.parametrize("n_mels,W,tag", [(3, 400, "13"), (80, 320, "10"), (128, 512, "16"), (128, 258, "10"), (80, 416, "13"), (80, 418, "16")])
def test_other_builds(ss, sslib, n_mels, W, tag):
    """three bands (slots without a filter), and the window lengths of the other two NE builds with their boundaries"""
    worst = 0.0
    for L in (401, 560, 3000):
        x = nm.gpu_clip(L)
        got = ss.nemo_log_mel(dev(x), n_mels=n_mels, normalize=None, win_length=W).cpu().numpy()
        assert sslib.ss_last_kernel_name().decode() == f"ss_nemo_c256<{tag}>"
        worst = max(worst, nm.block_metric(got, want(L, n_mels, False, W)))
        norm = ss.nemo_log_mel(dev(x), n_mels=n_mels, win_length=W).cpu().numpy()
        worst = max(worst, nm.block_metric(norm, want(L, n_mels, True, W)))
    print(f"nemo {n_mels} bands, win_length {W}: {worst:.3g}")
    assert worst <= BAR


def test_kernel_names(ss, sslib):
    x = dev(nm.gpu_clip(3000))
    ss.nemo_log_mel(x)
    assert sslib.ss_last_kernel_name().decode() == "ss_nemo_c256<13>"
    ss.nemo_log_mel_packed(x, [3000])
    assert sslib.ss_last_kernel_name().decode() == "ss_nemo_c256<13,v>"
    ss.nemo_log_mel_packed(x, [3000], win_length=320)
    assert sslib.ss_last_kernel_name().decode() == "ss_nemo_c256<10,v>"
    ss.nemo_log_mel_packed(x, [3000], win_length=512)
    assert sslib.ss_last_kernel_name().decode() == "ss_nemo_c256<16,v>"


@pytest.mark.parametrize("n_mels", nm.GPU_BANDS)
def test_normalisation_stage_on_its_own(ss, n_mels):
    """the stage's input is the device's own log-mel rows (the normalising call forms the same rows with the same kernel, then works in
    place); its reference is step 8 in f64 on them"""
    worst = 0.0
    for L in nm.GPU_LENS:
        x = dev(nm.gpu_clip(L))
        rows = ss.nemo_log_mel(x, n_mels=n_mels, normalize=None).cpu().numpy()
        got = ss.nemo_log_mel(x, n_mels=n_mels).cpu().numpy()
        ref = nm.normalized(rows)
        err = np.abs(got.astype(np.float64) - ref) / np.maximum(1.0, np.abs(ref))
        worst = max(worst, float(err.max()))
        if L // 160 == 1:
            assert (got == 0.0).all()  # T = 1: the deviation is 0, (l - mean) is 0
    print(f"nemo normalisation stage, {n_mels} bands: worst element error {worst:.3g} (bar {2.0 ** -22:.3g})")
    assert worst <= 2.0 ** -22
    zero = ss.nemo_log_mel(dev(np.zeros(800, np.float32)), n_mels=n_mels)
    assert zero.shape == (5, n_mels) and bool((zero == 0.0).all())  # every row is ln(guard): the mean is exact, the rows are exact zeros
    raw = ss.nemo_log_mel(dev(np.zeros(800, np.float32)), n_mels=n_mels, normalize=None).cpu().numpy()
    assert np.abs(raw - np.log(nm.GUARD)).max() <= 2e-6


@pytest.mark.parametrize("normalize", [None, "per_feature"])
def test_bit_for_bit_invariants(ss, normalize):
    import torch

    kw = dict(n_mels=128, normalize=normalize)
    clips = [nm.gpu_clip(L) for L in nm.GPU_LENS]
    singles = [ss.nemo_log_mel(dev(c), **kw) for c in clips]

    def check(block, expect):
        sig, lens = packed(block)
        out, fo = ss.nemo_log_mel_packed(dev(sig), lens, **kw)
        assert fo.tolist() == np.concatenate([[0], np.cumsum([n // 160 for n in lens])]).tolist()
        for b, e in enumerate(expect):
            if e is not None:
                assert torch.equal(out[fo[b]:fo[b + 1]], e), b
            else:
                assert fo[b] == fo[b + 1]
        return out

    # even and odd sample offsets (161, 399, 401 are odd lengths): a packed clip is the dense call on that clip alone
    assert sum(np.cumsum([len(c) for c in clips])[:-1] % 2) >= 2
    whole = check(clips, singles)
    # the rows do not change with the number of clips sharing the call, nor with their order
    check(clips[:3], singles[:3])
    check(clips[::-1], singles[::-1])
    check([clips[7]], [singles[7]])
    # a zero-length clip and a 100-sample clip inside the block own no rows; the others are unchanged
    holes = clips[:2] + [np.zeros(0, np.float32)] + clips[2:5] + [nm.make_input(100, 5)] + clips[5:]
    out = check(holes, singles[:2] + [None] + singles[2:5] + [None] + singles[5:])
    assert torch.equal(out, whole)
    # between two loud neighbours: nothing leaks across a clip's edges (the frames that overhang read zeros, not the neighbour)
    loud = (nm.make_input(777, 9) * np.float32(100.0)).astype(np.float32)
    loud_rows = [ss.nemo_log_mel(dev(loud), **kw), ss.nemo_log_mel(dev(loud[:333]), **kw)]
    for b in (0, 3, 6, 7):
        check([loud, clips[b], loud[:333]], [loud_rows[0], singles[b], loud_rows[1]])
    # row b of a batch equals the single-clip call; the host forms agree with the device forms
    x = np.stack([nm.make_input(1777, 20 + r) for r in range(3)])
    batch = ss.nemo_log_mel(dev(x), **kw)
    for r in range(3):
        assert torch.equal(batch[r], ss.nemo_log_mel(dev(x[r]), **kw))
    np.testing.assert_array_equal(ss.nemo_log_mel(x, **kw), batch.cpu().numpy())
    sig, lens = packed(clips)
    host, fo_h = ss.nemo_log_mel_packed(sig, lens, **kw)
    np.testing.assert_array_equal(host, whole.cpu().numpy())
    as_list = ss.nemo_log_mel_list([dev(c) for c in clips], **kw)
    assert all(torch.equal(a, b) for a, b in zip(as_list, singles))


def test_odd_row_stride(ss):
    """a batch whose rows start at either parity: pair and single-float quads alternate"""
    import torch

    L = 3000
    wide = torch.zeros((4, L + 1), dtype=torch.float32, device="cuda")
    x = np.stack([nm.make_input(L, 40 + r) for r in range(4)])
    wide[:, :L] = dev(x)
    got = ss.nemo_log_mel(wide[:, :L], n_mels=80)
    assert wide[:, :L].stride(0) % 2 == 1
    for r in range(4):
        assert torch.equal(got[r], ss.nemo_log_mel(dev(x[r]), n_mels=80))


@pytest.mark.parametrize("c", [nm.PREEMPH, 0.0])
def test_preemphasis_of_a_constant_clip(ss, c):
    """a constant-1.0 clip of 560 samples: the first sample keeps 1.0, the rest become 1 - c, the tail is zero (the restatement, which
    tests/test_nemo_cpu.py holds to exactly that)"""
    x = np.ones(560, np.float32)
    got = ss.nemo_log_mel(dev(x), n_mels=80, normalize=None, preemph=c).cpu().numpy()
    m = nm.block_metric(got, nm.features(x, 80, False, 400, c))
    print(f"nemo constant clip, preemph {c:.2f}: {m:.3g}")
    assert m <= BAR
    packed_rows, _ = ss.nemo_log_mel_packed(dev(np.concatenate([x * 50, x, x * 50])), [560, 560, 560], n_mels=80, normalize=None, preemph=c)
    np.testing.assert_array_equal(packed_rows[3:6].cpu().numpy(), got)  # the predecessor of the clip's first sample is 0, not the neighbour's


def test_dense_loop(ss, sslib):
    """one dense call with more than 12 quads per CU: every wave goes round the persistent loop again (the LDS claim, the prefetch into
    the input registers, the carried limit / predecessor / edge flag); three of its clips against f64, all of them against the same
    clips in calls of at most one quad per wave, bit for bit"""
    import torch

    cus = int(torch.cuda.get_device_properties(0).multi_processor_count)
    assert nm.loop_quads() > nm.WAVES * cus, "the shape rule of the loop test does not hold on this device"
    B, T = nm.LOOP_CLIPS, nm.LOOP_FRAMES
    L = T * 160 + 37
    g = torch.Generator(device="cuda")
    g.manual_seed(3)
    x = torch.randn((B, L), generator=g, device="cuda", dtype=torch.float32).mul_(0.1)
    raw = ss.nemo_log_mel(x, n_mels=128, normalize=None)
    assert raw.shape == (B, T, 128) and sslib.ss_last_kernel_name().decode() == "ss_nemo_c256<13>"
    worst = 0.0
    for b in (0, B // 2 - 1, B - 1):
        worst = max(worst, nm.block_metric(raw[b].cpu().numpy(), nm.features(x[b].cpu().numpy(), 128, False)))
    print(f"nemo dense loop ({B} clips of {T} frames, {cus} CUs): {worst:.3g}")
    assert worst <= BAR
    per = max(1, nm.WAVES * cus * 4 // T)  # clips of a covered call: at most one quad per wave
    parts = torch.cat([ss.nemo_log_mel(x[i:i + per], n_mels=128, normalize=None) for i in range(0, B, per)])
    assert torch.equal(parts, raw)
    so, fo = np.arange(B + 1, dtype=np.int64) * L, np.arange(B + 1, dtype=np.int64) * T
    rows, fo2 = ss.nemo_log_mel_packed(x.reshape(-1), [L] * B, n_mels=128, normalize=None)
    assert fo2.tolist() == fo.tolist() and torch.equal(rows.view(B, T, 128), raw) and so[-1] == x.numel()


def test_packed_containment(ss, sslib):
    """One decreasing sample_offsets pair and one wrong frame_offsets pair: those clips' rows keep the sentinel, every other clip is bit
    for bit the clean call, the handle reports SS_ERR_DEVICE once; the host form refuses the sample table before any launch.  Nothing
    here may fault: the kernels skip, they do not chase."""
    import torch

    handle = ss.NemoConfig(make_nemo_params(sslib, 80))
    lens = [480, 1000, 700, 900, 350, 1300, 640]
    Ts = [n // 160 for n in lens]
    sig, _ = packed([nm.make_input(n, 60 + b) for b, n in enumerate(lens)])
    so = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    fo = np.concatenate([[0], np.cumsum(Ts)]).astype(np.int64)
    rows = int(fo[-1])
    x = dev(sig)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def run(so_t, fo_t):
        out = torch.full((rows, 80), SENTINEL, dtype=torch.float32, device="cuda")
        dso, dfo = dev(so_t), dev(fo_t)
        assert sslib.ss_nemo_log_mel_packed_device(handle.handle, x.data_ptr(), len(lens), dso.data_ptr(), dfo.data_ptr(), rows, out.data_ptr(),
                                                   stream) == SS_OK
        torch.cuda.synchronize()
        return out.cpu().numpy()

    clean = run(so, fo)
    assert sslib.ss_nemo_config_device_status(handle.handle) == SS_OK and (clean != SENTINEL).all()
    bad_so, bad_fo = so.copy(), fo.copy()
    bad_so[3] = so[2] - 8   # clip 2 has a negative length; clip 3 starts early: 708 + 900 samples are not the 5 rows it owns
    bad_fo[-1] += 1         # the last clip claims a row more than its samples give (and ends past total_frames)
    skipped = {2, 3, 6}
    assert (bad_so[4] - bad_so[3]) // 160 != Ts[3]
    got = run(bad_so, bad_fo)
    assert sslib.ss_nemo_config_device_status(handle.handle) == SS_ERR_DEVICE
    assert sslib.ss_nemo_config_device_status(handle.handle) == SS_OK
    for b in range(len(lens)):
        lo, hi = int(fo[b]), int(fo[b + 1])
        if b in skipped:
            assert (got[lo:hi] == SENTINEL).all(), b
        else:
            np.testing.assert_array_equal(got[lo:hi], clean[lo:hi])
    np.testing.assert_array_equal(run(so, fo), clean)  # the handle serves the next clean call
    assert sslib.ss_nemo_config_device_status(handle.handle) == SS_OK
    out = np.full((rows, 80), SENTINEL, np.float32)
    assert sslib.ss_nemo_log_mel_packed(handle.handle, sig.ctypes.data, len(lens), bad_so.ctypes.data, out.ctypes.data) == SS_ERR_ARG
    assert (out == SENTINEL).all()
    assert sslib.ss_nemo_log_mel_packed_device(handle.handle, x.data_ptr(), 0, None, None, 0, None, stream) == SS_OK


def test_graph_capture_over_changing_tables(ss):
    """nemo_log_mel_packed captured once over device tables, replayed on a second input with other offsets in the same-sized tables"""
    import torch

    sets = [[1000, 480, 2000, 161, 900], [700, 1600, 333, 1200, 1100]]
    n_samples, total = 5200, 40
    kw = dict(n_mels=128)

    def tables(lens):
        so = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        return so, np.concatenate([[0], np.cumsum([n // 160 for n in lens])]).astype(np.int64)

    sig = torch.zeros(n_samples, dtype=torch.float32, device="cuda")
    dso, dfo = dev(tables(sets[0])[0]), dev(tables(sets[0])[1])
    ss.nemo_log_mel_packed(sig, None, device_tables=(dso, dfo, total), **kw)  # warm-up off the capture: the handle, the kernels' set-up
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out, _ = ss.nemo_log_mel_packed(sig, None, device_tables=(dso, dfo, total), **kw)
    for k, lens in enumerate(sets):
        so, fo = tables(lens)
        assert so[-1] <= n_samples and fo[-1] <= total
        x = nm.make_input(n_samples, 300 + k)
        sig.copy_(dev(x))
        dso.copy_(dev(so))
        dfo.copy_(dev(fo))
        out.fill_(SENTINEL)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        eager, fo_e = ss.nemo_log_mel_packed(dev(x[:so[-1]]), lens, **kw)
        assert fo_e.tolist() == fo.tolist()
        assert torch.equal(out[:fo[-1]], eager) and bool((out[fo[-1]:] == SENTINEL).all())
        m = nm.block_metric(out[:fo[1]].cpu().numpy(), nm.features(x[:lens[0]], 128, True))
        assert m <= BAR


def test_chain_from_the_resampler_to_the_padded_batch(ss):
    """resample_packed 44.1 -> 16 kHz, its (out, out_lengths) handed on as they stand; the rows go on to pad_packed in both layouts"""
    import torch

    lens = [2000, 3001, 1500]
    sig = dev(np.concatenate([nm.make_input(n, 90 + b) for b, n in enumerate(lens)]))
    res, res_lens = ss.resample_packed(sig, lens, 44100, 16000)
    oo = np.concatenate([[0], np.cumsum(res_lens)])
    assert any(int(o) % 2 for o in oo[1:-1])
    rows, fo = ss.nemo_log_mel_packed(res, res_lens, n_mels=80)
    singles = [ss.nemo_log_mel(res[int(oo[b]):int(oo[b + 1])].clone(), n_mels=80) for b in range(len(lens))]
    for b, one in enumerate(singles):
        assert torch.equal(rows[fo[b]:fo[b + 1]], one)
    for layout in ("btc", "bct"):
        out, lengths = ss.nemo_log_mel_list([res[int(oo[b]):int(oo[b + 1])] for b in range(len(lens))], n_mels=80, padded=True, layout=layout,
                                            dtype="bfloat16")
        want_out, want_len = ss.pad_packed(rows, fo, None, layout, "bfloat16")
        assert torch.equal(out, want_out) and torch.equal(lengths, want_len) and out.dtype == torch.bfloat16
