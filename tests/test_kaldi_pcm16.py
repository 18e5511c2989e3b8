"""The one-shot Kaldi calls fed signed 16-bit PCM: ss_kpcm_{fbank,mfcc}[_packed][_device] and ``pcm_scale=`` of kaldi_fbank,
kaldi_mfcc, their packed and list forms -- the PCM builds ss_kaldi_c256<..,i> (equal-length clips) and <..,vi> (packed clips).

Contract: sample = (float)pcm * scale, scale a power of two, so every output bit -- rows, log energy, the handle's error status -- is
what the float entry point gives on ``pcm.astype(float32) * scale`` with the same handle.  Every comparison below is on raw bits
against that float call (``torch.equal`` / ``np.array_equal`` on whole buffers, guard rows and sentinels included); no tolerance
appears.  Parity with f64 is the float call's (tests/test_kaldi*.py) and is not measured again.

PCM is drawn over the whole int16 range with -32768 and 32767 placed in every clip; scales are 2^-15 and 1.0."""
import ctypes as C

import numpy as np
import pytest

from test_kaldi import clip_len, front_kw
from test_kaldi_builds import SENTINEL, Front
from test_kaldi_cpu import (LOOP_T, SS_ERR_ARG, SS_ERR_DEVICE, SS_OK, kaldi_grid, kp, loop_dense_clips, loop_packed_frames,
                            make_kaldi_params, ref_num_frames, ref_sizes)
from test_kaldi_loop import cu_count, same_bits

pytestmark = pytest.mark.gpu
SCALES = [2.0 ** -15, 1.0]

# name -> (mfcc, parameters, the NE class): the six configurations of the dense comparison; the first four are the packed ones too
CONFIGS = {
    "25ms_fbank80_energy": (False, dict(num_mel_bins=80), 13),
    "20ms_mfcc13_on_40": (True, dict(frame_length_ms=20.0, num_mel_bins=40, num_ceps=13), 10),
    "32ms_magnitude_fbank80": (False, dict(frame_length_ms=32.0, num_mel_bins=80, use_power=0), 16),  # flen 512
    "11025hz_25ms": (False, dict(sample_rate=11025, num_mel_bins=40), 10),                             # flen 275: the half pair
    "flen_257": (False, dict(frame_length_ms=16.0625, num_mel_bins=80), 10),
    "shift_161": (False, dict(num_mel_bins=80, frame_shift_ms=10.0625), 13),
}
PACKED_CONFIGS = list(CONFIGS)[:4]


class PcmFront(Front):
    """tests/test_kaldi_builds.py's Front -- one handle, outputs between guard rows -- with the sample pointer read as int16 PCM times
    ``scale`` (the ss_kpcm_* entries); ``scale=None`` is the float front itself."""

    def __init__(self, ss, sslib, mfcc, scale, **cfg):
        super().__init__(ss, sslib, mfcc, **cfg)
        self.scale = scale

    def float_twin(self):
        """the float calls on the SAME handle"""
        twin = Front.__new__(Front)
        twin.__dict__.update(self.__dict__)
        return twin

    def launch_dense(self, x_ptr, batch, L, ld, out, en, stream=None):
        h, s = self.config.handle, C.c_void_p(stream) if stream else None
        if self.mfcc:
            return self.lib.ss_kpcm_mfcc_device(h, x_ptr, batch, L, ld, self.scale, out.inner.data_ptr(), s)
        return self.lib.ss_kpcm_fbank_device(h, x_ptr, batch, L, ld, self.scale, out.inner.data_ptr(), en.inner.data_ptr(), s)

    def launch_packed(self, x_ptr, n, dso, dfo, rows, out, en, stream=None):
        h, s = self.config.handle, C.c_void_p(stream) if stream else None
        if self.mfcc:
            return self.lib.ss_kpcm_mfcc_packed_device(h, x_ptr, n, dso.data_ptr(), self.scale, dfo.data_ptr(), rows, out.inner.data_ptr(), s)
        return self.lib.ss_kpcm_fbank_packed_device(h, x_ptr, n, dso.data_ptr(), self.scale, dfo.data_ptr(), rows, out.inner.data_ptr(),
                                                    en.inner.data_ptr(), s)


def random_pcm(n, seed):
    """int16 over the whole range, on the device"""
    import torch

    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    return torch.randint(-32768, 32768, (n,), generator=g, device="cuda", dtype=torch.int32).to(torch.int16)


def with_extremes(pcm, starts, ends):
    """-32768 as the first and 32767 as the last sample of every clip [start, end)"""
    for a, b in zip(starts, ends):
        pcm[int(a)] = -32768
        pcm[int(b) - 1] = 32767
    return pcm


def converted(pcm, scale):
    """what the float call is given: pcm.astype(float32) * scale"""
    import torch

    return pcm.to(torch.float32) * scale


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("name", list(CONFIGS))
def test_dense_bits(ss, sslib, name, scale):
    """3 clips of LOOP_T = 5 frames (quads straddle clips) in three layouts: ld = L, ld = L + 1, and the base advanced by one sample
    (2-byte alignment only for the PCM call; the float call takes the same layout of the converted floats)."""
    mfcc, cfg, NE = CONFIGS[name]
    front = PcmFront(ss, sslib, mfcc, scale, **cfg)
    twin = front.float_twin()
    B = 3
    L = clip_len(front.cfg, LOOP_T, extra=3)
    assert ref_num_frames(front.p, L) == LOOP_T
    for label, base, ld in (("ld=L", 0, L), ("ld=L+1", 0, L + 1), ("base+1", 1, L)):
        buf = random_pcm(base + B * ld + 8, 7 + base + ld)  # (the gaps and the tail hold samples that no frame may read)
        with_extremes(buf, [base + b * ld for b in range(B)], [base + b * ld + L for b in range(B)])
        xf = converted(buf, scale)
        want = twin.dense(xf.data_ptr() + 4 * base, B, L, ld)
        fname = twin.kernel()
        got = front.dense(buf.data_ptr() + 2 * base, B, L, ld)
        iname = front.kernel()
        assert same_bits(got, want), (label, int((got[0] != want[0]).sum()))
        assert fname.startswith(f"ss_kaldi_c256<{NE},") and iname == fname[:-1] + ",i>", (fname, iname)
    assert front.status() == SS_OK


def test_input_scale_applies_behind_the_pcm_scale(ss, sslib):
    """scale = 2^-15 with input_scale = 32768: the float call's bits on the converted samples, and -- both factors being powers of
    two -- the bits of scale = 1.0 with input_scale = 1."""
    mfcc, cfg, _ = CONFIGS["25ms_fbank80_energy"]
    front = PcmFront(ss, sslib, mfcc, 2.0 ** -15, input_scale=32768.0, **cfg)
    plain = PcmFront(ss, sslib, mfcc, 1.0, **cfg)
    L = clip_len(front.cfg, LOOP_T, extra=1)
    buf = with_extremes(random_pcm(3 * L, 19), [0, L, 2 * L], [L, 2 * L, 3 * L])
    got = front.dense(buf.data_ptr(), 3, L, L)
    xf = converted(buf, 2.0 ** -15)  # (a name of its own: the block must outlive the launch that reads it)
    assert same_bits(got, front.float_twin().dense(xf.data_ptr(), 3, L, L))
    assert same_bits(got, plain.dense(buf.data_ptr(), 3, L, L))


def packed_case(front, seed):
    """clip lengths flen, flen + 1, flen + shift - 1, flen + shift, flen + 8 shift + 1, flen + 10 shift + 80: offsets of both
    parities, three one-frame clips -> (lens, so, fo, pcm)"""
    flen, shift, _ = ref_sizes(front.p)
    lens = [flen, flen + 1, flen + shift - 1, flen + shift, flen + 8 * shift + 1, flen + 10 * shift + 80]
    Ts = [ref_num_frames(front.p, n) for n in lens]
    assert Ts == [1, 1, 1, 2, 9, 11]
    so, fo = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64), np.concatenate([[0], np.cumsum(Ts)]).astype(np.int64)
    assert {int(o) % 2 for o in so[:-1]} == {0, 1}
    pcm = with_extremes(random_pcm(int(so[-1]), seed), so[:-1], so[1:])
    return lens, so, fo, pcm


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("name", PACKED_CONFIGS)
def test_packed_bits(ss, sslib, name, scale):
    mfcc, cfg, NE = CONFIGS[name]
    front = PcmFront(ss, sslib, mfcc, scale, **cfg)
    twin = front.float_twin()
    lens, so, fo, pcm = packed_case(front, 23)
    xf = converted(pcm, scale)
    rows = int(fo[-1])
    want = twin.packed(xf.data_ptr(), so, fo, rows=rows + 2, written=False)  # two spare rows: left alone
    fname = twin.kernel()
    got = front.packed(pcm.data_ptr(), so, fo, rows=rows + 2, written=False)
    iname = front.kernel()
    assert same_bits(got, want)
    assert bool((got[0][rows:] == SENTINEL).all()) and not bool((got[0][:rows] == SENTINEL).any())
    assert fname.startswith(f"ss_kaldi_c256<{NE},") and fname.endswith(",v>") and iname == fname[:-3] + ",vi>", (fname, iname)
    # every clip equals the dense PCM call on that clip alone
    for b, n in enumerate(lens):
        one = front.dense(pcm.data_ptr() + 2 * int(so[b]), 1, n, n)
        lo, hi = int(fo[b]), int(fo[b + 1])
        assert same_bits(one, [got[0][lo:hi], None if got[1] is None else got[1][lo:hi]]), b
    assert front.status() == SS_OK


@pytest.mark.parametrize("scale", SCALES)
def test_host_forms_and_python_front(ss, sslib, scale):
    import torch

    for name in ("25ms_fbank80_energy", "20ms_mfcc13_on_40", "11025hz_25ms"):
        mfcc, cfg, _ = CONFIGS[name]
        front = PcmFront(ss, sslib, mfcc, scale, **cfg)
        h = front.config.handle
        cols = front.cols
        # dense: 3 rows at ld = L + 1 on the host
        L = clip_len(front.cfg, LOOP_T, extra=2)
        wide = with_extremes(random_pcm(3 * (L + 1), 31), [b * (L + 1) for b in range(3)], [b * (L + 1) + L for b in range(3)])
        dev = front.dense(wide.data_ptr(), 3, L, L + 1)
        hw = wide.cpu().numpy()
        out, en = np.full((3 * LOOP_T, cols), SENTINEL, np.float32), np.full((3 * LOOP_T,), SENTINEL, np.float32)
        if mfcc:
            assert sslib.ss_kpcm_mfcc(h, hw.ctypes.data, 3, L, L + 1, scale, out.ctypes.data) == SS_OK, sslib.ss_last_error_string()
        else:
            assert sslib.ss_kpcm_fbank(h, hw.ctypes.data, 3, L, L + 1, scale, out.ctypes.data, en.ctypes.data) == SS_OK, sslib.ss_last_error_string()
            assert np.array_equal(en.view(np.int32), dev[1].cpu().numpy().view(np.int32))
        assert np.array_equal(out.view(np.int32), dev[0].cpu().numpy().view(np.int32))
        # packed: the host form takes the sample offsets alone
        lens, so, fo, pcm = packed_case(front, 37)
        devp = front.packed(pcm.data_ptr(), so, fo)
        hp = pcm.cpu().numpy()
        rows = int(fo[-1])
        out, en = np.full((rows, cols), SENTINEL, np.float32), np.full((rows,), SENTINEL, np.float32)
        if mfcc:
            assert sslib.ss_kpcm_mfcc_packed(h, hp.ctypes.data, len(lens), so.ctypes.data, scale, out.ctypes.data) == SS_OK
        else:
            assert sslib.ss_kpcm_fbank_packed(h, hp.ctypes.data, len(lens), so.ctypes.data, scale, out.ctypes.data, en.ctypes.data) == SS_OK
            assert np.array_equal(en.view(np.int32), devp[1].cpu().numpy().view(np.int32))
        assert np.array_equal(out.view(np.int32), devp[0].cpu().numpy().view(np.int32))
        assert front.status() == SS_OK

    # the Python front: the same functions on the converted floats, numpy and torch inputs
    def host(t):
        return t.cpu().numpy() if hasattr(t, "cpu") else t

    fkw = front_kw(dict(num_mel_bins=80, use_energy=1))
    mkw = front_kw(dict(frame_length_ms=20.0, num_mel_bins=40, num_ceps=13), mfcc=True)
    L = clip_len({}, 6, extra=1)
    x = with_extremes(random_pcm(3 * L, 41), [0, L, 2 * L], [L, 2 * L, 3 * L]).view(3, L)
    want = ss.kaldi_fbank(converted(x, scale), **fkw)
    for sig in (x, x.cpu().numpy(), x[1], x[1].cpu().numpy()):
        got = ss.kaldi_fbank(sig, pcm_scale=scale, **fkw)
        assert isinstance(got, np.ndarray) != hasattr(sig, "is_cuda")
        w = want if len(sig.shape) == 2 else want[1]
        assert got.shape == w.shape and np.array_equal(host(got).view(np.int32), host(w).view(np.int32))
    assert sslib.ss_last_kernel_name().endswith(b",i>")
    mf = PcmFront(ss, sslib, True, scale, frame_length_ms=20.0, num_mel_bins=40, num_ceps=13)
    lens, so, fo, pcm = packed_case(mf, 43)
    want, fo_w = ss.kaldi_mfcc_packed(converted(pcm, scale), lens, **mkw)
    for sig in (pcm, pcm.cpu().numpy()):
        got, fo_g = ss.kaldi_mfcc_packed(sig, lens, pcm_scale=scale, **mkw)
        assert fo_g.tolist() == fo_w.tolist() == fo.tolist() and np.array_equal(host(got).view(np.int32), host(want).view(np.int32))
    lens, so, fo, pcm = packed_case(PcmFront(ss, sslib, False, scale, num_mel_bins=80), 47)  # (25 ms frames: the list call's shape)
    clips = [pcm[int(so[b]):int(so[b + 1])] for b in range(len(lens))]
    wants = ss.kaldi_fbank_list([converted(c, scale) for c in clips], **fkw)
    for lst in (clips, [c.cpu().numpy() for c in clips]):
        gots = ss.kaldi_fbank_list(lst, pcm_scale=scale, **fkw)
        assert len(gots) == len(wants) and all(np.array_equal(host(g).view(np.int32), host(w).view(np.int32)) for g, w in zip(gots, wants))
    assert bool(torch.isfinite(want).all())


@pytest.mark.parametrize("wrong", ["last", "interior", "short"])
def test_packed_containment(ss, sslib, wrong):
    """tests/test_kaldi.py::test_packed_containment on ss_kpcm_fbank_packed_device beside the float call on the converted samples: the
    same rows keep the sentinel, every other row has the float call's bits, the return codes and the handle's status agree."""
    import torch

    cfg = dict(num_mel_bins=80)
    scale = 2.0 ** -15
    handles = [ss.KaldiConfig(make_kaldi_params(sslib, **cfg)) for _ in range(2)]  # (each call family its own error word)
    Ts = [2, 3, 1, 4, 2]
    lens = [clip_len(cfg, T, extra=b) for b, T in enumerate(Ts)]
    if wrong == "short":
        lens[2] = ref_sizes(kp(**cfg))[0] - 1  # a clip shorter than a frame, with the row its table claims
    so = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    fo = np.concatenate([[0], np.cumsum(Ts)]).astype(np.int64)
    rows = int(fo[-1])
    pcm = with_extremes(random_pcm(int(so[-1]), 61), so[:-1], so[1:])
    xf = converted(pcm, scale)
    dso = torch.from_numpy(so).cuda()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def run(table, as_pcm):
        out = torch.full((rows, 80), SENTINEL, dtype=torch.float32, device="cuda")
        en = torch.full((rows,), SENTINEL, dtype=torch.float32, device="cuda")
        dfo = torch.from_numpy(table).cuda()
        if as_pcm:
            rc = sslib.ss_kpcm_fbank_packed_device(handles[0].handle, pcm.data_ptr(), len(Ts), dso.data_ptr(), scale, dfo.data_ptr(), rows,
                                                   out.data_ptr(), en.data_ptr(), stream)
        else:
            rc = sslib.ss_kaldi_fbank_packed_device(handles[1].handle, xf.data_ptr(), len(Ts), dso.data_ptr(), dfo.data_ptr(), rows,
                                                    out.data_ptr(), en.data_ptr(), stream)
        torch.cuda.synchronize()
        status = sslib.ss_kaldi_config_device_status(handles[0 if as_pcm else 1].handle)
        again = sslib.ss_kaldi_config_device_status(handles[0 if as_pcm else 1].handle)
        return rc, status, again, out.cpu().numpy(), en.cpu().numpy()

    bad = fo.copy()
    if wrong == "last":
        bad[-1] += 1
        skipped = [4]
    elif wrong == "interior":
        bad[3] += 1
        skipped = [2, 3]
    else:
        skipped = [2]
    got, want = run(bad, True), run(bad, False)
    assert got[:3] == want[:3] == (SS_OK, SS_ERR_DEVICE, SS_OK)
    assert np.array_equal(got[3].view(np.int32), want[3].view(np.int32)) and np.array_equal(got[4].view(np.int32), want[4].view(np.int32))
    for b in range(len(Ts)):
        lo, hi = int(fo[b]), int(fo[b + 1])
        kept = (got[3][lo:hi] == SENTINEL).all() and (got[4][lo:hi] == SENTINEL).all()
        written = not (got[3][lo:hi] == SENTINEL).any() and not (got[4][lo:hi] == SENTINEL).any()
        assert kept if b in skipped else written, b
    if wrong != "short":  # the handle serves the next clean call
        clean_i, clean_f = run(fo, True), run(fo, False)
        assert clean_i[:3] == clean_f[:3] == (SS_OK, SS_OK, SS_OK) and np.array_equal(clean_i[3].view(np.int32), clean_f[3].view(np.int32))
        assert not (clean_i[3] == SENTINEL).any()


def test_a_bad_scale_is_an_argument_error_and_nothing_runs(ss, sslib):
    import torch

    front = PcmFront(ss, sslib, False, 1.0, num_mel_bins=80)
    h = front.config.handle
    L = clip_len(front.cfg, LOOP_T)
    pcm = random_pcm(2 * L, 71)
    so = torch.tensor([0, L, 2 * L], dtype=torch.int64, device="cuda")
    fo = torch.tensor([0, LOOP_T, 2 * LOOP_T], dtype=torch.int64, device="cuda")
    out = torch.full((2 * LOOP_T, 80), SENTINEL, device="cuda")
    en = torch.full((2 * LOOP_T,), SENTINEL, device="cuda")
    xf = converted(pcm, 1.0)
    front.float_twin().dense(xf.data_ptr(), 2, L, L)  # a float call first: the name a rejected call leaves in place
    fname = front.kernel()
    hp, hout = pcm.cpu().numpy(), np.full((2 * LOOP_T, 80), SENTINEL, np.float32)
    hso = np.array([0, L, 2 * L], np.int64)
    for bad in (3.0, 0.0, float("nan"), 2.0 ** 70):
        assert sslib.ss_kpcm_fbank_device(h, pcm.data_ptr(), 2, L, L, bad, out.data_ptr(), en.data_ptr(), None) == SS_ERR_ARG
        assert b"scale must be a power of two" in sslib.ss_last_error_string()
        assert sslib.ss_kpcm_mfcc_device(h, pcm.data_ptr(), 2, L, L, bad, out.data_ptr(), None) == SS_ERR_ARG
        assert sslib.ss_kpcm_fbank_packed_device(h, pcm.data_ptr(), 2, so.data_ptr(), bad, fo.data_ptr(), 2 * LOOP_T, out.data_ptr(), en.data_ptr(),
                                                 None) == SS_ERR_ARG
        assert sslib.ss_kpcm_mfcc_packed_device(h, pcm.data_ptr(), 2, so.data_ptr(), bad, fo.data_ptr(), 2 * LOOP_T, out.data_ptr(), None) == SS_ERR_ARG
        assert sslib.ss_kpcm_fbank(h, hp.ctypes.data, 2, L, L, bad, hout.ctypes.data, None) == SS_ERR_ARG
        assert sslib.ss_kpcm_fbank_packed(h, hp.ctypes.data, 2, hso.ctypes.data, bad, hout.ctypes.data, None) == SS_ERR_ARG
        assert b"scale must be a power of two" in sslib.ss_last_error_string()
    # the float call's other rules, in the PCM form: ld < n_samples, null buffers, a signal shorter than a frame, an odd address
    assert sslib.ss_kpcm_fbank_device(h, pcm.data_ptr(), 2, L, L - 1, 1.0, out.data_ptr(), en.data_ptr(), None) == SS_ERR_ARG
    assert sslib.ss_kpcm_fbank_device(h, None, 2, L, L, 1.0, out.data_ptr(), en.data_ptr(), None) == SS_ERR_ARG
    assert sslib.ss_kpcm_fbank_device(h, pcm.data_ptr(), 2, 100, 100, 1.0, out.data_ptr(), en.data_ptr(), None) == 1  # SS_ERR_SHORT_SIGNAL
    assert sslib.ss_kpcm_fbank_device(h, pcm.data_ptr() + 1, 2, L - 1, L - 1, 1.0, out.data_ptr(), en.data_ptr(), None) == SS_ERR_ARG
    assert sslib.ss_kpcm_fbank_device(h, None, 0, L, L, 1.0, None, None, None) == SS_OK  # an empty batch, as the float form
    assert sslib.ss_kpcm_fbank_packed_device(h, None, 0, None, 1.0, None, 0, None, None, None) == SS_OK
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()) and bool((en == SENTINEL).all()) and (hout == SENTINEL).all()
    assert front.kernel() == fname and front.status() == SS_OK
    for s in (2.0 ** 64, 2.0 ** -64):  # the ends of the range are in it
        assert sslib.ss_kpcm_fbank_device(h, pcm.data_ptr(), 2, L, L, s, out.data_ptr(), en.data_ptr(), None) == SS_OK
    torch.cuda.synchronize()


def test_dense_loop(ss, sslib):
    """The persistent loop (tests/test_kaldi_loop.py's shape: 3 * 12 * CUs + 5 quads): the PCM build carries raw dwords across the
    loop's prefetch hand-over.  NE 13, fbank with the log energy, odd ld; the big PCM call equals the big float call bit for bit."""
    cus = cu_count()
    front = PcmFront(ss, sslib, False, 2.0 ** -15, num_mel_bins=80, energy_floor=0.0)
    B = loop_dense_clips(cus)
    L = clip_len(front.cfg, LOOP_T, extra=6)
    ld = L + 1
    assert ref_num_frames(front.p, L) == LOOP_T and kaldi_grid(-(-B * LOOP_T // 4), cus) == cus
    pcm = random_pcm(B * ld, 81)
    xf = converted(pcm, front.scale)
    want = front.float_twin().dense(xf.data_ptr(), B, L, ld)
    got = front.dense(pcm.data_ptr(), B, L, ld)
    assert front.kernel() == "ss_kaldi_c256<13,pow2,fbank,i>"
    assert same_bits(got, want)


def test_packed_loop(ss, sslib):
    """NE 10, MFCC, the big packed call of tests/test_kaldi_loop.py (one-frame runs, 1 .. 7 frames, a long clip now and then; offsets of
    both parities): bit for bit the big float call."""
    cus = cu_count()
    front = PcmFront(ss, sslib, True, 1.0, frame_length_ms=20.0, num_mel_bins=40, num_ceps=13, energy_floor=0.0)
    flen, shift, _ = ref_sizes(front.p)
    Ts = loop_packed_frames(cus)
    rng = np.random.default_rng(5)
    lens = np.array([flen + (t - 1) * shift for t in Ts], np.int64) + rng.integers(0, 8, len(Ts))
    so, fo = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64), np.concatenate([[0], np.cumsum(Ts)]).astype(np.int64)
    assert (so % 2 == 1).sum() > len(Ts) // 4 and (so % 2 == 0).sum() > len(Ts) // 4
    assert kaldi_grid(-(-int(fo[-1]) // 4), cus) == cus
    pcm = random_pcm(int(so[-1]), 82)
    xf = converted(pcm, front.scale)
    want = front.float_twin().packed(xf.data_ptr(), so, fo)
    got = front.packed(pcm.data_ptr(), so, fo)
    assert front.kernel() == "ss_kaldi_c256<10,pow2,mfcc,vi>" and front.status() == SS_OK
    assert same_bits(got, want)


@pytest.mark.parametrize("cfg,mfcc,tag", [
    (dict(num_mel_bins=80), False, "13,pow2,fbank"),
    (dict(num_mel_bins=23, frame_length_ms=20.0), False, "10,pow2,fbank"),
    (dict(num_mel_bins=80, frame_length_ms=32.0, use_power=0), False, "16,fbank"),
    (dict(sample_rate=11025, num_mel_bins=40), False, "10,pow2,fbank"),
    (dict(num_mel_bins=23, num_ceps=13), True, "13,pow2,mfcc"),
])
def test_dispatch(ss, sslib, cfg, mfcc, tag):
    """tests/test_kaldi.py::test_dispatch through ``pcm_scale=``: the float call's NE and switch tags with ,i> / ,vi>"""
    x = random_pcm(clip_len(cfg, 5), 91)
    kw = front_kw(cfg, mfcc)
    (ss.kaldi_mfcc if mfcc else ss.kaldi_fbank)(x, pcm_scale=1.0, **kw)
    assert sslib.ss_last_kernel_name().decode() == f"ss_kaldi_c256<{tag},i>"
    (ss.kaldi_mfcc_packed if mfcc else ss.kaldi_fbank_packed)(x, [int(x.shape[0])], pcm_scale=1.0, **kw)
    assert sslib.ss_last_kernel_name().decode() == f"ss_kaldi_c256<{tag},vi>"


def test_graph_capture_replays_over_new_samples_and_new_tables(ss, sslib):
    """One packed PCM fbank call, captured (a single kernel node: a chain without branches) and replayed after the samples and both
    device tables were overwritten in place: the replay equals the eager PCM call and the float call on the new tables."""
    import torch

    front = PcmFront(ss, sslib, False, 2.0 ** -15, num_mel_bins=80)
    twin = front.float_twin()
    flen, shift, _ = ref_sizes(front.p)
    frame_sets = [[1, 3, 2, 5, 4], [5, 1, 1, 2, 3], [2, 2, 6, 1, 1], [4, 1, 2, 2, 7]]
    extras = [[0, 1, 3, 2, 5], [1, 1, 0, 4, 2], [3, 0, 0, 1, 1], [2, 5, 1, 0, 3]]
    tables = []
    for Ts, ex in zip(frame_sets, extras):
        lens = [flen + (t - 1) * shift + e for t, e in zip(Ts, ex)]
        tables.append((np.concatenate([[0], np.cumsum(lens)]).astype(np.int64), np.concatenate([[0], np.cumsum(Ts)]).astype(np.int64)))
    n = max(int(so[-1]) for so, _ in tables)
    total = max(int(fo[-1]) for _, fo in tables)
    dso, dfo = torch.from_numpy(tables[0][0]).cuda(), torch.from_numpy(tables[0][1]).cuda()
    pcm = random_pcm(n, 100)
    out, en = front.buffers(total)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up off the capture
        assert front.launch_packed(pcm.data_ptr(), 5, dso, dfo, total, out, en, side.cuda_stream) == SS_OK
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        assert front.launch_packed(pcm.data_ptr(), 5, dso, dfo, total, out, en, torch.cuda.current_stream().cuda_stream) == SS_OK
    assert front.kernel() == "ss_kaldi_c256<13,pow2,fbank,vi>"
    for k in (1, 2, 3):
        pcm.copy_(random_pcm(n, 100 + k))
        dso.copy_(torch.from_numpy(tables[k][0]))
        dfo.copy_(torch.from_numpy(tables[k][1]))
        out.full.fill_(SENTINEL)
        en.full.fill_(SENTINEL)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        out.check(written=False)
        en.check(written=False)
        eager = front.packed(pcm.data_ptr(), tables[k][0], tables[k][1], rows=total, written=False)
        xf = converted(pcm, front.scale)
        want = twin.packed(xf.data_ptr(), tables[k][0], tables[k][1], rows=total, written=False)
        assert same_bits([out.inner, en.inner], eager) and same_bits(eager, want), k
        rows = int(tables[k][1][-1])
        assert not bool((out.inner[:rows] == SENTINEL).any()) and bool((out.inner[rows:] == SENTINEL).all()), k
    assert front.status() == SS_OK
