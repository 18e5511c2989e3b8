"""The Kaldi-compatible fbank / MFCC front end on the device (ss_kaldi_c256, ss_kaldi512.hip) against the numpy f64 restatement of
the header's specification in tests/test_kaldi_cpu.py.

Bars (the project's own): block metric max|got - want| / max|want| <= 1e-4 for an fbank block; for MFCC column 0 and columns 1.. each
against their own maximum; log energy within 1e-4 of max|want|.  Every parity test prints the largest figure it met.  Inputs: a
batch row each of standard_normal * 0.1, the same * 32768, and uniform integers in [-32768, 32767] as floats (the overflow probe).
Shapes are small: T in {1, 4, 5, 17} frames covers a lone frame, one full quad, a quad plus one, and several quads."""
import ctypes as C

import numpy as np
import pytest

from test_kaldi_cpu import (EPS, SS_ERR_DEVICE, SS_ERR_UNSUPPORTED, SS_OK, WINDOWS, block_metric, gpu_case_signal, kp, make_kaldi_params,
                            ref_fbank, ref_mfcc, ref_num_frames, ref_sizes)

pytestmark = pytest.mark.gpu
BAR = 1e-4
KINDS = ("unit", "scaled", "int16")
LN_EPS = float(np.log(np.float32(EPS).astype(np.float64)))

# ss_kaldi_params names -> the Python front's (torchaudio's) keyword names
FRONT = dict(sample_rate="sample_frequency", frame_length_ms="frame_length", frame_shift_ms="frame_shift", preemph_coef="preemphasis_coefficient")


def front_kw(cfg, mfcc=False):
    kw = {FRONT.get(k, k): v for k, v in cfg.items()}
    for k in ("remove_dc_offset", "use_power", "use_energy", "raw_energy"):
        if k in kw:
            kw[k] = bool(kw[k])
    if mfcc:
        kw.pop("use_power", None)
    else:
        kw.pop("num_ceps", None)
        kw.pop("cepstral_lifter", None)
    return kw


def clip_len(cfg, T, extra=0):
    flen, shift, _ = ref_sizes(kp(**cfg))
    return flen + (T - 1) * shift + extra


def batch_of_kinds(seed, L):
    """[3 x L]: one row per input family"""
    return np.stack([gpu_case_signal(seed + i, L, kind) for i, kind in enumerate(KINDS)])


def fbank_and_energy(ss, x, cfg):
    """the front's fbank with the log energy in column 0 -> (fbank, log_energy)"""
    out = ss.kaldi_fbank(x, **front_kw({**cfg, "use_energy": 1}))
    out = out.cpu().numpy() if hasattr(out, "cpu") else out
    return out[..., 1:], out[..., 0]


def energy_metric(got, want):
    return float(np.abs(got.astype(np.float64) - want).max() / np.abs(want).max())


FBANK_CONFIGS = {
    "16k_25ms_80": dict(num_mel_bins=80),                                         # NE 13
    "16k_20ms_23": dict(frame_length_ms=20.0, num_mel_bins=23),                   # NE 10
    "16k_32ms_80": dict(frame_length_ms=32.0, num_mel_bins=80),                   # NE 16
    "11k_25ms_40": dict(sample_rate=11025, num_mel_bins=40),                      # odd frame length 275, even shift 110
    "shift_161": dict(num_mel_bins=80, frame_shift_ms=10.0625),                   # odd frame starts
}


@pytest.mark.parametrize("name", list(FBANK_CONFIGS) + ["odd_ld"])
def test_fbank_parity(ss, name):
    import torch

    cfg = {**FBANK_CONFIGS.get(name, dict(num_mel_bins=80)), "energy_floor": 0.0}
    p = kp(**cfg)
    worst, worst_e = 0.0, 0.0
    for T in (1, 4, 5, 17):
        L = clip_len(cfg, T, extra=7 if T > 1 else 0)
        x = batch_of_kinds(100 * T, L)
        assert ref_num_frames(p, L) == T
        if name == "odd_ld":
            wide = torch.zeros((3, L + (2 if L % 2 else 1)), dtype=torch.float32, device="cuda")  # an odd row stride
            wide[:, :L] = torch.from_numpy(x).cuda()
            xd = wide[:, :L]
            assert xd.stride(0) % 2 == 1
        else:
            xd = torch.from_numpy(x).cuda()
        fb, le = fbank_and_energy(ss, xd, cfg)
        assert fb.shape == (3, T, p["num_mel_bins"]) and le.shape == (3, T)
        for r in range(3):
            want, want_e = ref_fbank(x[r], p)
            worst = max(worst, block_metric(fb[r], want))
            worst_e = max(worst_e, energy_metric(le[r], want_e))
    print(f"kaldi fbank {name}: block metric {worst:.3g}, log energy {worst_e:.3g}")
    assert worst <= BAR and worst_e <= BAR


@pytest.mark.parametrize("M,Cc", [(23, 13), (80, 20)])
@pytest.mark.parametrize("lifter", [22.0, 0.0])
@pytest.mark.parametrize("use_energy,raw_energy", [(0, 1), (1, 1), (1, 0)])
def test_mfcc_parity(ss, M, Cc, lifter, use_energy, raw_energy):
    import torch

    cfg = dict(num_mel_bins=M, num_ceps=Cc, cepstral_lifter=lifter, use_energy=use_energy, raw_energy=raw_energy)
    p = kp(**cfg)
    L = clip_len(cfg, 6, extra=11)
    x = batch_of_kinds(7, L)
    got = ss.kaldi_mfcc(torch.from_numpy(x).cuda(), **front_kw(cfg, mfcc=True)).cpu().numpy()
    assert got.shape == (3, 6, Cc)
    c0 = ck = 0.0
    for r in range(3):
        want = ref_mfcc(x[r], p)
        c0 = max(c0, block_metric(got[r][:, 0], want[:, 0]))
        ck = max(ck, block_metric(got[r][:, 1:], want[:, 1:]))
    print(f"kaldi mfcc {M}/{Cc} lifter {lifter} use_energy {use_energy} raw_energy {raw_energy}: column 0 {c0:.3g}, columns 1.. {ck:.3g}")
    assert c0 <= BAR and ck <= BAR


def test_mfcc_beyond_sixteen_cepstra(ss):
    """17 .. 32 cepstra: the lanes' second coefficient"""
    import torch

    cfg = dict(num_mel_bins=40, num_ceps=32)
    x = batch_of_kinds(9, clip_len(cfg, 5))
    got = ss.kaldi_mfcc(torch.from_numpy(x).cuda(), **front_kw(cfg, mfcc=True)).cpu().numpy()
    for r in range(3):
        want = ref_mfcc(x[r], kp(**cfg))
        assert block_metric(got[r][:, 0], want[:, 0]) <= BAR and block_metric(got[r][:, 1:], want[:, 1:]) <= BAR


SWITCHES = {**{f"window_{w}": dict(window_type=w, blackman_coeff=0.40) for w in WINDOWS},
            "magnitude": dict(use_power=0), "no_preemphasis": dict(preemph_coef=0.0), "windowed_energy": dict(raw_energy=0),
            "shift_beyond_the_frame": dict(frame_shift_ms=30.0)}


@pytest.mark.parametrize("name", list(SWITCHES))
def test_switches_one_at_a_time(ss, name):
    import torch

    cfg = {"num_mel_bins": 40, "energy_floor": 0.0, **SWITCHES[name]}
    x = batch_of_kinds(31, clip_len(cfg, 5, extra=3))
    fb, le = fbank_and_energy(ss, torch.from_numpy(x).cuda(), cfg)
    worst = max(block_metric(fb[r], ref_fbank(x[r], kp(**cfg))[0]) for r in range(3))
    worst_e = max(energy_metric(le[r], ref_fbank(x[r], kp(**cfg))[1]) for r in range(3))
    print(f"kaldi fbank switch {name}: block metric {worst:.3g}, log energy {worst_e:.3g}")
    assert worst <= BAR and worst_e <= BAR


def test_dc_removal_switch_on_a_clip_with_an_offset(ss):
    cfg_off = dict(num_mel_bins=40, energy_floor=0.0, remove_dc_offset=0)
    cfg_on = dict(num_mel_bins=40, energy_floor=0.0)
    x = gpu_case_signal(5, clip_len(cfg_off, 5), "unit") + np.float32(0.3)
    for cfg in (cfg_off, cfg_on):
        fb, le = fbank_and_energy(ss, x, cfg)
        want, want_e = ref_fbank(x, kp(**cfg))
        assert block_metric(fb, want) <= BAR and energy_metric(le, want_e) <= BAR
    assert np.abs(fbank_and_energy(ss, x, cfg_off)[1] - fbank_and_energy(ss, x, cfg_on)[1]).min() > 1.0  # the offset dominates the raw energy


def test_energy_floor(ss):
    x = gpu_case_signal(6, clip_len({}, 5), "unit") * np.float32(1e-3)  # a 1e-4-scale clip: frame energies far below 1
    _, le = fbank_and_energy(ss, x, dict(energy_floor=1.0))
    assert (le == 0.0).all()  # ln(energy_floor) = ln 1, exactly
    _, le0 = fbank_and_energy(ss, x, dict(energy_floor=0.0))
    want = ref_fbank(x, kp(energy_floor=0.0))[1]
    assert (want < -5.0).all() and energy_metric(le0, want) <= BAR


def test_known_answers(ss):
    cfg = dict(num_mel_bins=80, energy_floor=0.0)
    L = clip_len(cfg, 5)
    for clip in (np.zeros(L, np.float32), np.full(L, 0.5, np.float32)):
        fb, le = fbank_and_energy(ss, clip, cfg)  # the constant clip: the mean is an exact division, every frame is exactly zero
        np.testing.assert_allclose(fb, LN_EPS, rtol=0, atol=2e-6)
        np.testing.assert_allclose(le, LN_EPS, rtol=0, atol=2e-6)
    cfg = {**cfg, "remove_dc_offset": 0}
    clip = np.full(L, 0.5, np.float32)
    fb, le = fbank_and_energy(ss, clip, cfg)
    want, want_e = ref_fbank(clip, kp(**cfg))
    assert np.abs(want - LN_EPS).max() > 5.0
    m, me = block_metric(fb, want), energy_metric(le, want_e)
    print(f"kaldi fbank constant clip without DC removal: block metric {m:.3g}, log energy {me:.3g}")
    assert m <= BAR and me <= BAR


def test_input_scale_is_the_scaled_input_bit_for_bit(ss):
    import torch

    cfg = dict(num_mel_bins=80, energy_floor=0.0)
    x = gpu_case_signal(8, clip_len(cfg, 9, extra=5), "unit")
    scaled = (x * np.float32(32768.0)).astype(np.float32)
    a = ss.kaldi_fbank(torch.from_numpy(x).cuda(), **front_kw({**cfg, "use_energy": 1, "input_scale": 32768.0}))
    b = ss.kaldi_fbank(torch.from_numpy(scaled).cuda(), **front_kw({**cfg, "use_energy": 1}))
    assert torch.equal(a, b)
    c = ss.kaldi_mfcc(torch.from_numpy(x).cuda(), input_scale=32768.0)
    d = ss.kaldi_mfcc(torch.from_numpy(scaled).cuda())
    assert torch.equal(c, d)


def _packed(clips):
    return np.concatenate(clips), [len(c) for c in clips]


@pytest.mark.parametrize("cfg", [dict(num_mel_bins=80), dict(num_mel_bins=23, frame_length_ms=20.0), dict(sample_rate=11025, num_mel_bins=40),
                                 dict(num_mel_bins=80, frame_shift_ms=10.0625)], ids=["ne13", "ne10", "odd_flen", "odd_shift"])
def test_bit_for_bit_invariants(ss, cfg):
    import torch

    Ts = [1, 1, 1, 1, 2, 3, 5]  # a quad spans up to four clips
    rng = np.random.default_rng(3)
    fkw, mkw = front_kw({**cfg, "use_energy": 1}), front_kw({**cfg, "num_ceps": 13, "use_energy": 1}, mfcc=True)

    def check_block(clips):
        sig, lens = _packed(clips)
        out, fo = ss.kaldi_fbank_packed(torch.from_numpy(sig).cuda(), lens, **fkw)
        cep, fo2 = ss.kaldi_mfcc_packed(torch.from_numpy(sig).cuda(), lens, **mkw)
        assert fo.tolist() == fo2.tolist() == np.concatenate([[0], np.cumsum([ref_num_frames(kp(**cfg), n) for n in lens])]).tolist()
        singles = []
        for b, clip in enumerate(clips):
            one = ss.kaldi_fbank(torch.from_numpy(clip).cuda(), **fkw)  # fbank and the log energy (column 0)
            assert torch.equal(out[fo[b]:fo[b + 1]], one), b
            assert torch.equal(cep[fo[b]:fo[b + 1]], ss.kaldi_mfcc(torch.from_numpy(clip).cuda(), **mkw)), b
            singles.append(one)
        return out, fo, singles

    clips = [gpu_case_signal(40 + b, clip_len(cfg, T, extra=int(rng.integers(0, 5)) * 2), KINDS[b % 3]) for b, T in enumerate(Ts)]
    clips = [c if len(c) % 2 == 0 else np.concatenate([c, c[-1:]]) for c in clips]  # every offset of this first block is even
    assert all(len(c) % 2 == 0 for c in clips) and [ref_num_frames(kp(**cfg), len(c)) for c in clips] == Ts
    out, fo, singles = check_block(clips)
    # permuting the clips permutes the rows
    perm = [3, 6, 0, 5, 1, 4, 2]
    out_p, fo_p, _ = check_block([clips[i] for i in perm])
    for k, i in enumerate(perm):
        assert torch.equal(out_p[fo_p[k]:fo_p[k + 1]], out[fo[i]:fo[i + 1]])
    # a one-sample spacer in front of some clips (the clip before them grows by one sample): odd offsets, the same rows
    spaced = [np.concatenate([c, c[-1:]]) if b in (0, 2, 3, 5) else c for b, c in enumerate(clips)]
    assert [ref_num_frames(kp(**cfg), len(c)) for c in spaced] == Ts
    out_s, fo_s, _ = check_block(spaced)
    assert torch.equal(out_s, out)
    # row b of a batch equals the single-clip call
    L = clip_len(cfg, 6, extra=1)
    x = batch_of_kinds(77, L)
    whole = ss.kaldi_fbank(torch.from_numpy(x).cuda(), **fkw)
    for r in range(3):
        assert torch.equal(whole[r], ss.kaldi_fbank(torch.from_numpy(x[r]).cuda(), **fkw))
    # the host forms agree with the device forms
    np.testing.assert_array_equal(ss.kaldi_fbank(x, **fkw), whole.cpu().numpy())
    np.testing.assert_array_equal(ss.kaldi_mfcc(x, **mkw), ss.kaldi_mfcc(torch.from_numpy(x).cuda(), **mkw).cpu().numpy())
    sig, lens = _packed(clips)
    host, fo_h = ss.kaldi_fbank_packed(sig, lens, **fkw)
    np.testing.assert_array_equal(host, out.cpu().numpy())
    assert fo_h.tolist() == fo.tolist()
    as_list = ss.kaldi_fbank_list([torch.from_numpy(c).cuda() for c in clips], **fkw)
    assert all(torch.equal(a, b) for a, b in zip(as_list, singles))


@pytest.mark.parametrize("wrong", ["last", "interior"])
def test_packed_containment(ss, sslib, wrong):
    """One frame_offsets entry is wrong: the clips that entry bounds are skipped -- their rows keep the sentinel -- every other clip
    equals the clean call, and the handle reports SS_ERR_DEVICE once.  Nothing here may fault: the kernel skips, it does not chase."""
    import torch

    cfg = dict(num_mel_bins=80)
    handle = ss.KaldiConfig(make_kaldi_params(sslib, **cfg))
    Ts = [2, 3, 1, 4, 2]
    clips = [gpu_case_signal(60 + b, clip_len(cfg, T, extra=b), "unit") for b, T in enumerate(Ts)]
    sig, lens = _packed(clips)
    so = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    fo = np.concatenate([[0], np.cumsum(Ts)]).astype(np.int64)
    rows = int(fo[-1])
    x, dso = torch.from_numpy(sig).cuda(), torch.from_numpy(so).cuda()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def run(table):
        out = torch.full((rows, 80), -7777.0, dtype=torch.float32, device="cuda")
        en = torch.full((rows,), -7777.0, dtype=torch.float32, device="cuda")
        dfo = torch.from_numpy(table).cuda()
        assert sslib.ss_kaldi_fbank_packed_device(handle.handle, x.data_ptr(), len(Ts), dso.data_ptr(), dfo.data_ptr(), rows, out.data_ptr(),
                                                  en.data_ptr(), stream) == SS_OK
        torch.cuda.synchronize()
        return out.cpu().numpy(), en.cpu().numpy()

    clean, clean_e = run(fo)
    assert sslib.ss_kaldi_config_device_status(handle.handle) == SS_OK
    assert (clean != -7777.0).all() and (clean_e != -7777.0).all()
    bad = fo.copy()
    if wrong == "last":
        bad[-1] += 1       # the last clip claims a row more than its samples give (and ends past total_frames)
        skipped = [4]
    else:
        bad[3] += 1        # the entry between clips 2 and 3: neither has the rows its samples give
        skipped = [2, 3]
    got, got_e = run(bad)
    assert sslib.ss_kaldi_config_device_status(handle.handle) == SS_ERR_DEVICE
    assert sslib.ss_kaldi_config_device_status(handle.handle) == SS_OK
    for b in range(len(Ts)):
        lo, hi = int(fo[b]), int(fo[b + 1])
        if b in skipped:
            assert (got[lo:hi] == -7777.0).all() and (got_e[lo:hi] == -7777.0).all(), b
        else:
            np.testing.assert_array_equal(got[lo:hi], clean[lo:hi])
            np.testing.assert_array_equal(got_e[lo:hi], clean_e[lo:hi])
    again, _ = run(fo)  # the handle serves the next clean call
    np.testing.assert_array_equal(again, clean)
    assert sslib.ss_kaldi_fbank_packed_device(handle.handle, x.data_ptr(), 0, dso.data_ptr(), dso.data_ptr(), 0, x.data_ptr(), None, stream) == SS_OK


@pytest.mark.parametrize("cfg,mfcc,tag", [
    (dict(num_mel_bins=80), False, "13,pow2,fbank"),
    (dict(num_mel_bins=23, frame_length_ms=20.0), False, "10,pow2,fbank"),
    (dict(num_mel_bins=80, frame_length_ms=32.0, use_power=0), False, "16,fbank"),
    (dict(sample_rate=11025, num_mel_bins=40), False, "10,pow2,fbank"),
    (dict(num_mel_bins=23, num_ceps=13), True, "13,pow2,mfcc"),
])
def test_dispatch(ss, sslib, cfg, mfcc, tag):
    import torch

    x = torch.from_numpy(gpu_case_signal(1, clip_len(cfg, 5), "unit")).cuda()
    kw = front_kw(cfg, mfcc)
    (ss.kaldi_mfcc if mfcc else ss.kaldi_fbank)(x, **kw)
    name = sslib.ss_last_kernel_name().decode()
    assert name.startswith("ss_kaldi_c256<") and name == f"ss_kaldi_c256<{tag}>", name
    (ss.kaldi_mfcc_packed if mfcc else ss.kaldi_fbank_packed)(x, [int(x.shape[0])], **kw)
    assert sslib.ss_last_kernel_name().decode() == f"ss_kaldi_c256<{tag},v>"


def test_other_sizes_fail_create(ss, sslib):
    h = C.c_void_p()
    assert sslib.ss_kaldi_config_create(C.byref(make_kaldi_params(sslib, sample_rate=8000)), C.byref(h)) == SS_ERR_UNSUPPORTED and not h.value
    with pytest.raises(ss.SpeechSauceError) as e:
        ss.kaldi_fbank(np.zeros(4000, np.float32), sample_frequency=8000)
    assert e.value.status == SS_ERR_UNSUPPORTED


def test_chain_from_the_resampler(ss):
    """resample_packed 44.1 -> 16 kHz, its (out, out_lengths) handed to kaldi_fbank_packed as they stand: per clip the rows are those of
    kaldi_fbank on that clip's resampled samples, bit for bit (the resampled clips start at offsets of either parity)."""
    import torch

    lens = [2000, 3001, 1500]
    sig = torch.from_numpy(np.concatenate([gpu_case_signal(90 + b, n, "unit") for b, n in enumerate(lens)])).cuda()
    out, out_lens = ss.resample_packed(sig, lens, 44100, 16000)
    oo = np.concatenate([[0], np.cumsum(out_lens)])
    assert any(int(o) % 2 for o in oo[1:-1])
    kw = dict(num_mel_bins=80, use_energy=True)
    rows, fo = ss.kaldi_fbank_packed(out, out_lens, **kw)
    for b in range(len(lens)):
        clip = out[int(oo[b]):int(oo[b + 1])]
        assert torch.equal(rows[fo[b]:fo[b + 1]], ss.kaldi_fbank(clip.clone(), **kw))
        assert torch.equal(rows[fo[b]:fo[b + 1]], ss.kaldi_fbank(clip, **kw))  # (a view: the clip's own base alignment)
