"""The Whisper log-mel front end (ss_whisper_*) on the GPU: parity against the numpy f64 restatement (tests/whisper_model.py) at the
project's bar of 1e-4 absolute on an output of order 1, the bit-exact invariants (batch row, packed clip, permutation, host form,
16-bit types, graph replay), the containment of a bad table entry between sentinel guard rows, and the kernel's name."""
import ctypes as C

import numpy as np
import pytest

import whisper_model as wm

pytestmark = pytest.mark.gpu

BAR = 1e-4
KINDS = ("normal", "pcm", "tone")
F32, F16, BF16 = 0, 1, 2


@pytest.fixture(scope="module")
def torch():
    import torch

    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def ss(sslib):
    import speechsauce_amd

    return speechsauce_amd


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda() if a.size else torch.zeros(0, dtype=torch.float32, device="cuda")


def _bits(t):
    """a device tensor of any of the three types as a numpy array of bit patterns"""
    import torch

    if t.dtype == torch.float32:
        return t.cpu().numpy().view(np.uint32)
    return t.view(torch.int16).cpu().numpy().view(np.uint16)


# (n_frames, n_samples): every n_frames of the issue, samples on both sides of trimming, and N - len over the end-reflection and
# silent-frame boundary {0, 1, 39, 40, 41, 199, 200, 201}
def _dense_cases():
    cases = []
    for nf in (2, 3, 8, 9, 17, 100):
        N = nf * 160
        lens = {0, 1, 159, 160, 161, 199, 200, 201, 1600, 16000, N + 1, N + 777}
        lens |= {N - d for d in (0, 1, 39, 40, 41, 199, 200, 201) if N - d >= 0}
        cases += [(nf, n) for n in sorted(lens)]
    return cases


@pytest.mark.parametrize("n_mels", (80, 128))
def test_dense_parity(ss, torch, n_mels):
    worst = {}
    for i, (nf, n) in enumerate(_dense_cases()):
        kind = KINDS[i % 3]
        x = wm.make_input(kind, n, 100 + i)
        got = ss.whisper_log_mel(_dev(torch, x), n_mels=n_mels, n_frames=nf).cpu().numpy()
        assert got.shape == (n_mels, nf) and got.dtype == np.float32
        ref = wm.log_mel(x, n_mels, nf)
        err = np.abs(got - ref).max()
        worst[kind] = max(worst.get(kind, 0.0), err)
        assert err <= BAR, (kind, nf, n, err)
    print(f"n_mels {n_mels}: worst abs err per input {worst}")


@pytest.mark.parametrize("kind", KINDS)
def test_batch_parity_and_default_frames(ss, torch, kind):
    x = np.stack([wm.make_input(kind, 16000, s) for s in range(3)])
    got = ss.whisper_log_mel(_dev(torch, x), n_mels=80).cpu().numpy()  # n_frames=None: 16000 // 160
    assert got.shape == (3, 80, 100)
    errs = [np.abs(got[b] - wm.log_mel(x[b], 80, 100)).max() for b in range(3)]
    f32 = [np.abs(wm.log_mel_f32(x[b], 80, 100) - wm.log_mel(x[b], 80, 100)).max() for b in range(3)]
    print(f"{kind}: kernel {max(errs):.3g}, f32 restatement {max(f32):.3g}")
    assert max(errs) <= BAR


def test_window_of_thirty_seconds(ss, torch):
    """a 3 s clip in the 3000-frame window: 90 % silent frames, none of them loaded or transformed"""
    x = wm.make_input("normal", 48000, 9)
    got = ss.whisper_log_mel(_dev(torch, x), n_mels=128, n_frames=3000).cpu().numpy()
    assert np.abs(got - wm.log_mel(x, 128, 3000)).max() <= BAR
    assert ss._lib.lib().ss_last_kernel_name() == b"ss_whisper_c200"


def test_zero_clips_and_small_banks(ss, torch):
    for nf, n in ((2, 0), (9, 0), (9, 1440), (100, 777)):
        got = ss.whisper_log_mel(_dev(torch, np.zeros(n, np.float32)), n_frames=nf).cpu().numpy()
        assert np.all(got == np.float32(-1.5)), (nf, n)
    for m in (1, 3):
        x = wm.make_input("normal", 3000, m)
        got = ss.whisper_log_mel(_dev(torch, x), n_mels=m, n_frames=17).cpu().numpy()
        assert got.shape == (m, 17) and np.abs(got - wm.log_mel(x, m, 17)).max() <= BAR


LENS = [16000, 1601, 0, 333, 4800, 7, 4801, 2560, 2561, 160]  # odd and even offsets; short clips share a work unit's neighbourhood


def _packed_inputs(seed=40):
    clips = [wm.make_input(KINDS[i % 3], n, seed + i) for i, n in enumerate(LENS)]
    return clips, np.concatenate(clips)


@pytest.mark.parametrize("dtype", ("float32", "float16", "bfloat16"))
def test_packed_clip_equals_dense_call(ss, torch, dtype):
    clips, packed = _packed_inputs()
    for base in (0, 1, 3):  # the packed block on an even, an odd and an unaligned sample of its allocation
        buf = torch.zeros(packed.size + 8, dtype=torch.float32, device="cuda")
        buf[base:base + packed.size] = torch.from_numpy(packed).cuda()
        out, lens = ss.whisper_log_mel_packed(buf[base:base + packed.size], LENS, n_frames=20, dtype=dtype)
        assert out.shape == (len(LENS), 80, 20)
        assert lens.cpu().tolist() == [min(n // 160, 20) for n in LENS]
        for b, c in enumerate(clips):
            want = ss.whisper_log_mel(_dev(torch, c), n_frames=20, dtype=dtype)
            assert np.array_equal(_bits(out[b]), _bits(want)), (base, b)


def test_batch_row_equals_single_clip_and_host_equals_device(ss, torch):
    x = np.stack([wm.make_input(KINDS[s % 3], 5000, 70 + s) for s in range(5)])
    dev = ss.whisper_log_mel(_dev(torch, x), n_mels=128, n_frames=33).cpu().numpy()
    for b in range(5):
        assert np.array_equal(ss.whisper_log_mel(_dev(torch, x[b]), n_mels=128, n_frames=33).cpu().numpy(), dev[b])
    # a strided batch: rows of a wider block
    wide = _dev(torch, np.concatenate([x, np.ones((5, 3), np.float32)], axis=1))
    assert np.array_equal(ss.whisper_log_mel(wide[:, :5000], n_mels=128, n_frames=33).cpu().numpy(), dev)
    assert np.array_equal(ss.whisper_log_mel(x, n_mels=128, n_frames=33), dev)
    clips, packed = _packed_inputs()
    h_out, h_len = ss.whisper_log_mel_packed(packed, LENS, n_frames=20)
    d_out, d_len = ss.whisper_log_mel_packed(_dev(torch, packed), LENS, n_frames=20)
    assert np.array_equal(h_out, d_out.cpu().numpy()) and np.array_equal(h_len, d_len.cpu().numpy())
    l_out, l_len = ss.whisper_log_mel_list(clips, n_frames=20)
    assert np.array_equal(l_out, h_out) and np.array_equal(l_len, h_len)


def test_permutation_of_the_clips_permutes_the_blocks(ss, torch):
    clips, packed = _packed_inputs()
    out, lens = ss.whisper_log_mel_packed(_dev(torch, packed), LENS, n_mels=128, n_frames=20)
    perm = [3, 9, 0, 5, 7, 1, 2, 8, 4, 6]
    out2, lens2 = ss.whisper_log_mel_list([_dev(torch, clips[i]) for i in perm], n_mels=128, n_frames=20)
    assert np.array_equal(out2.cpu().numpy(), out.cpu().numpy()[perm]) and lens2.cpu().tolist() == [lens.cpu().tolist()[i] for i in perm]


def test_sixteen_bit_types_are_the_converted_f32_result(ss, torch):
    x = np.stack([wm.make_input(KINDS[s % 3], 4000, 90 + s) for s in range(3)])
    for nf in (25, 24, 17):  # blocks that are and are not a whole number of 16-byte groups
        f32 = ss.whisper_log_mel(_dev(torch, x), n_frames=nf).cpu().numpy()
        f16 = ss.whisper_log_mel(_dev(torch, x), n_frames=nf, dtype="float16")
        bf16 = ss.whisper_log_mel(_dev(torch, x), n_frames=nf, dtype=torch.bfloat16)
        assert f16.dtype == torch.float16 and bf16.dtype == torch.bfloat16
        assert np.array_equal(f16.cpu().numpy(), f32.astype(np.float16))
        assert np.array_equal(_bits(bf16), wm.to_bf16_bits(f32))
        # the host forms: float16, and bfloat16 as bit patterns
        assert np.array_equal(ss.whisper_log_mel(x, n_frames=nf, dtype="float16"), f32.astype(np.float16))
        assert np.array_equal(ss.whisper_log_mel(x, n_frames=nf, dtype="bfloat16"), wm.to_bf16_bits(f32))


def _raw_packed(sslib, torch, cfg, x, so, n_frames, code, work, out, lens):
    from speechsauce_amd import _lib

    _lib.check(sslib.ss_whisper_log_mel_packed_device(cfg.handle, x.data_ptr(), so.numel() - 1, so.data_ptr(), n_frames, code,
                                                      work.data_ptr() if work is not None else None, out.data_ptr(), lens.data_ptr(),
                                                      C.c_void_p(torch.cuda.current_stream().cuda_stream)))


def test_replayed_graph_over_changed_tables_equals_eager(ss, sslib, torch):
    cfg = ss.WhisperConfig(80)
    nf, n = 20, 6
    rng = np.random.default_rng(5)
    x = _dev(torch, wm.make_input("normal", 40000, 1))
    so = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    out = torch.empty((n, 80, nf), dtype=torch.bfloat16, device="cuda")
    work = torch.empty((n * 80 * nf,), dtype=torch.float32, device="cuda")
    lens = torch.empty((n,), dtype=torch.int32, device="cuda")
    tables = [np.concatenate([[0], np.cumsum(rng.integers(0, 6000, n))]).astype(np.int64) for _ in range(3)]
    so.copy_(torch.from_numpy(tables[0]).cuda())
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _raw_packed(sslib, torch, cfg, x, so, nf, BF16, work, out, lens)  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        _raw_packed(sslib, torch, cfg, x, so, nf, BF16, work, out, lens)
    for tab in tables[1:] + tables[:1]:
        so.copy_(torch.from_numpy(tab).cuda())
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        got, got_len = _bits(out).copy(), lens.cpu().numpy().copy()
        want, want_len = ss.whisper_log_mel_packed(x, np.diff(tab).tolist(), n_frames=nf, dtype="bfloat16")
        assert np.array_equal(got, _bits(want)) and np.array_equal(got_len, want_len.cpu().numpy())
    cfg.device_status()


@pytest.mark.parametrize("code", (F32, BF16))
def test_a_bad_table_entry_is_contained(ss, sslib, torch, code):
    from speechsauce_amd import SpeechSauceError

    cfg = ss.WhisperConfig(80)
    nf, n, M = 20, 4, 80
    clips = [wm.make_input("normal", k, 300 + i) for i, k in enumerate((3000, 1700, 900, 2500))]
    x = _dev(torch, np.concatenate(clips))
    good = np.concatenate([[0], np.cumsum([c.size for c in clips])]).astype(np.int64)
    es = 4 if code == F32 else 2
    tdt = torch.float32 if code == F32 else torch.bfloat16
    guard = 64  # elements: a multiple of 16 bytes for both types

    def run(table):
        so = torch.from_numpy(table).cuda()
        blk = torch.full((n * M * nf + 2 * guard,), 7.0, dtype=tdt, device="cuda")
        wblk = torch.full((n * M * nf + 2 * guard,), 9.0, dtype=torch.float32, device="cuda")
        lblk = torch.full((n + 2,), -77, dtype=torch.int32, device="cuda")
        out, work, lens = blk[guard:guard + n * M * nf], wblk[guard:guard + n * M * nf], lblk[1:1 + n]
        assert out.data_ptr() % 16 == 0 and work.data_ptr() % 16 == 0 and es * guard % 16 == 0
        _raw_packed(sslib, torch, cfg, x, so, nf, code, work if code != F32 else None, out, lens)
        torch.cuda.synchronize()
        for g in (blk[:guard], blk[-guard:]):
            assert bool((g == 7.0).all())
        for g in (wblk[:guard], wblk[-guard:]):
            assert bool((g == 9.0).all())
        assert lblk[0].item() == -77 and lblk[-1].item() == -77
        return _bits(out.view(n, M, nf)), lens.cpu().numpy()

    want, want_len = run(good)
    cfg.device_status()  # nothing to report
    for bad_clip, table in ((1, good.copy()), (2, good.copy())):
        if bad_clip == 1:
            table[2] = table[1] - 5  # clip 1 reversed; clip 2 then starts early but is a consistent segment of its own
        else:
            table[2], table[3] = -4, -2  # entries below zero: clips 1, 2 and 3 are all inconsistent, clip 0 stands
        got, got_len = run(table)
        bad = [b for b in range(n) if table[b] < 0 or table[b + 1] < table[b]]
        assert bad_clip in bad
        minus = _bits(torch.full((1,), -1.5, dtype=tdt))[0]
        for b in range(n):
            if b in bad:
                assert (got[b] == minus).all() and got_len[b] == -1
            elif table[b] == good[b] and table[b + 1] == good[b + 1]:
                assert np.array_equal(got[b], want[b]) and got_len[b] == want_len[b]  # neighbours untouched
        with pytest.raises(SpeechSauceError) as e:
            cfg.device_status()
        assert e.value.status == 6
        cfg.device_status()  # reported once


def test_device_argument_errors(ss, sslib, torch):
    cfg = ss.WhisperConfig(80)
    x = torch.zeros(4000, dtype=torch.float32, device="cuda")
    out = torch.zeros(2 * 80 * 8 + 8, dtype=torch.float32, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    call = lambda xp, ld, nf, dt, work, op: sslib.ss_whisper_log_mel_device(cfg.handle, xp, 2, 1280, ld, nf, dt, work, op, st)
    assert call(x.data_ptr(), 1280, 8, F32, None, out.data_ptr()) == 0
    assert call(x.data_ptr(), 1279, 8, F32, None, out.data_ptr()) == 3   # ld < n_samples
    assert call(x.data_ptr(), 1280, 1, F32, None, out.data_ptr()) == 3   # n_frames < 2
    assert call(None, 1280, 8, F32, None, out.data_ptr()) == 3           # null buffers
    assert call(x.data_ptr(), 1280, 8, F32, None, None) == 3
    assert call(x.data_ptr(), 1280, 8, BF16, None, out.data_ptr()) == 3  # the 16-bit types need the scratch
    assert call(x.data_ptr() + 2, 1280, 8, F32, None, out.data_ptr()) == 3   # alignment
    assert call(x.data_ptr(), 1280, 8, F32, None, out.data_ptr() + 4) == 3
    assert call(x.data_ptr(), 1280, 8, BF16, out.data_ptr() + 4, out.data_ptr()) == 3
    assert sslib.ss_whisper_log_mel_packed_device(cfg.handle, x.data_ptr(), 2, None, 8, F32, None, out.data_ptr(), None, st) == 3
    torch.cuda.synchronize()
    p = ss.SsWhisperParams()
    assert sslib.ss_whisper_config_params(cfg.handle, C.byref(p)) == 0 and (p.n_mels, p.n_fft, p.hop_length, p.sample_rate) == (80, 400, 160, 16000)
