"""Noise mixing and gain perturbation of packed clips on the device: ss_noise_plan_packed[_i16]_device, ss_noise_apply_packed*,
ss_noise_mix_packed* and the Python front's noise_plan_packed, noise_apply_packed, noise_mix_packed and NoiseMix.

Against the numpy restatement of the header (tests/noise_mix_model.py): the draw fields, the two f64 energies and every output sample
are compared as bit patterns; the two gain words alone may be the restatement's f32 or its neighbour (the device's pow is not
correctly rounded), which is why the mix is held to the restatement on the device's own plan.  out, the plan and the scratch sit
between guard words.
"""
import ctypes as C

import numpy as np
import pytest

import noise_mix_model as m

pytestmark = pytest.mark.gpu

LENS = [0, 1, 3, 255, 256, 257, 2047, 2048, 2049, 4097, 40000]  # packed end to end: the offsets 1, 259, 515, 2819, 4867, 11013 are odd
NOISE_LENS = [1, 7, 1000, 50001]  # a clip sees no wrap, one wrap and thousands
# seed 120: the clip of 2048 draws the noise clip of 1000 at start 997 and the one of 40000 wraps the 50001 once; seed 131: the clip of
# 40000 draws the noise clip of 7 at start 4 (5714 wraps) -- test_the_seeds_reach_the_ends holds them to that
SEEDS = (120, 131)
SCALARS = (1.0, 10.0, 30.0, -6.0, 6.0)  # prob, SNR and gain ranges
GUARD = 64
PCM = 2.0 ** -15


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _i16(v, scale):
    return np.clip(np.round(np.asarray(v) / scale), -32768, 32767).astype(np.int16)


class Case:
    """speech and bank, float and PCM, on the host and on the device"""

    def __init__(self, torch, lens=LENS, noise_lens=NOISE_LENS, seed=0, pcm=False):
        self.so, self.no = m.table(lens), m.table(noise_lens)
        self.total, self.total_noise, self.n, self.n_noise = int(self.so[-1]), int(self.no[-1]), len(lens), len(noise_lens)
        x, nz = m.speech(lens, seed), m.speech(noise_lens, 1000 + seed, 0.03)
        self.scales = (PCM, PCM / 4) if pcm else None
        if pcm:
            self.raw_x, self.raw_nz = _i16(x, PCM), _i16(nz, PCM / 4)
            x, nz = self.raw_x.astype(np.float32) * np.float32(PCM), self.raw_nz.astype(np.float32) * np.float32(PCM / 4)
        else:
            self.raw_x, self.raw_nz = x, nz
        self.x, self.nz = x, nz  # the float samples the restatement works on
        self.d_x, self.d_nz = torch.from_numpy(self.raw_x).cuda(), torch.from_numpy(self.raw_nz).cuda()
        self.d_so, self.d_no = torch.from_numpy(self.so).cuda(), torch.from_numpy(self.no).cuda()

    def head(self, d_x=None):
        """the shared head of the argument lists"""
        sx, sn = ([self.scales[0]], [self.scales[1]]) if self.scales else ([], [])
        return [(self.d_x if d_x is None else d_x).data_ptr(), *sx, self.n, self.d_so.data_ptr(), self.total, self.d_nz.data_ptr(), *sn, self.n_noise,
                self.d_no.data_ptr(), self.total_noise]

    def fn(self, sslib, kind):
        return getattr(sslib, f"ss_noise_{kind}_packed{'_i16' if self.scales else ''}_device")

    def plan_ref(self, rng, scalars=SCALARS, base=0):
        return m.plan_ref(self.x, rng, base, self.so, self.total, self.nz, self.no, self.total_noise, scalars[0], scalars[1:3], scalars[3:5])

    def mix_ref(self, plan, out):
        return m.mix_ref(self.x, self.so, self.total, self.nz, self.no, self.total_noise, plan, out)


class Guarded:
    """a device block of `count` words of `dtype` between guards, pre-filled with a sentinel; `phase` words into its allocation"""

    def __init__(self, torch, count, dtype, sentinel, phase=0):
        self.count, self.sentinel = count, sentinel
        self.raw = torch.full((phase + GUARD + count + GUARD,), sentinel, dtype=dtype, device="cuda")
        self.at = phase + GUARD
        self.view = self.raw[self.at:self.at + count]

    def host(self, what):
        raw = self.raw.cpu().numpy()
        assert (raw[:self.at] == self.sentinel).all() and (raw[self.at + self.count:] == self.sentinel).all(), f"guard of {what}"
        return raw[self.at:self.at + self.count]


def _rng(torch, seed, epoch):
    return torch.from_numpy(np.array([seed, epoch], np.uint64).view(np.int64)).cuda()


def _words(block):
    return [int(v) for v in block.cpu().numpy().view(np.uint64)]


def _work_words(sslib, case):
    n = C.c_size_t()
    assert sslib.ss_noise_mix_work_bytes(case.n, case.total, C.byref(n)) == 0
    return n.value // 8


def _device_plan(torch, sslib, case, rng, scalars=SCALARS, base=0):
    """ss_noise_plan_packed[_i16]_device -> the plan on the host, guards of the plan and the scratch checked, the block untouched"""
    plan = Guarded(torch, case.n * 5, torch.int64, -99)
    work = Guarded(torch, _work_words(sslib, case), torch.float64, -7.0)
    block = _rng(torch, *rng)
    rc = case.fn(sslib, "plan")(*case.head(), block.data_ptr(), base, *scalars, plan.view.data_ptr(), work.view.data_ptr(), work.count * 8, None)
    assert rc == 0, sslib.ss_last_error_string()
    torch.cuda.synchronize()
    work.host("work")
    assert _words(block) == list(rng)  # the plan alone does not touch the epoch
    return plan.host("plan").view(m.ROW), plan


def _same_plan(got, want, gains_exact=False):
    for f in m.DRAW_FIELDS + ("speech_energy", "noise_energy"):
        assert np.array_equal(_bits(got[f]), _bits(want[f])), f
    for f in ("speech_gain", "noise_gain"):
        ok = _bits(got[f]) == _bits(want[f]) if gains_exact else m.adjacent_f32(got[f], want[f])
        assert ok.all(), (f, got[f], want[f])


@pytest.fixture(scope="module")
def cases():
    import torch

    return {pcm: Case(torch, pcm=pcm) for pcm in (False, True)}


def test_the_seeds_reach_the_ends(ss):
    d = ss.noise_draws((120, 0), LENS, NOISE_LENS, *SCALARS[:1], SCALARS[1:3], SCALARS[3:5])
    assert (d["noise_clip"][7], d["start"][7]) == (2, 997) and LENS[7] == 2048         # 3 samples before the end of the clip of 1000
    assert d["noise_clip"][10] == 3 and d["start"][10] + LENS[10] > NOISE_LENS[3]        # one wrap
    assert sorted(set(d["noise_clip"].tolist())) == [0, 1, 2, 3]
    d = ss.noise_draws((131, 0), LENS, NOISE_LENS, *SCALARS[:1], SCALARS[1:3], SCALARS[3:5])
    assert (d["noise_clip"][10], d["start"][10]) == (1, 4) and LENS[10] // NOISE_LENS[1] > 5000  # thousands of wraps, from 3 before the end


@pytest.mark.parametrize("pcm", (False, True), ids=("f32", "i16"))
def test_plan_against_the_model(sslib, cases, pcm):
    import torch

    case = cases[pcm]
    for rng, scalars, base in (((120, 0), SCALARS, 0), ((131, 0), SCALARS, 0), ((120, 2 ** 32 - 1), (0.5, 5.0, 5.0, 0.0, 0.0), 7)):
        got, _ = _device_plan(torch, sslib, case, rng, scalars, base)
        want = case.plan_ref(rng, scalars, base)
        _same_plan(got, want)
        mixed = got["noise_clip"] >= 0
        assert (got["noise_energy"][~mixed] == 0).all() and (got["noise_gain"][~mixed] == 0).all()
        assert got["speech_energy"][0] == 0 and got["noise_gain"][0] == 0  # the clip without samples
        assert (got["noise_gain"][1:][mixed[1:]] > 0).all()
        if scalars[3:5] == (0.0, 0.0):
            assert (_bits(got["speech_gain"]) == 0x3F800000).all()  # exactly 1.0f


@pytest.mark.parametrize("pcm", (False, True), ids=("f32", "i16"))
def test_apply_against_the_model_on_the_devices_plan(sslib, cases, pcm):
    import torch

    case = cases[pcm]
    for rng in ((120, 0), (131, 0)):
        rows, plan = _device_plan(torch, sslib, case, rng)
        held = np.full(case.total, -7.0, np.float32)
        want = case.mix_ref(rows, held)
        for phase in (0, 1, 3):  # out starts 0, 4 and 12 bytes past a 16-byte boundary
            out = Guarded(torch, case.total, torch.float32, -7.0, phase)
            rc = case.fn(sslib, "apply")(*case.head(), plan.view.data_ptr(), out.view.data_ptr(), None)
            assert rc == 0, sslib.ss_last_error_string()
            torch.cuda.synchronize()
            assert np.array_equal(_bits(out.host("out")), _bits(want)), phase
        if not pcm:  # in place: the samples themselves sit between the guards
            for phase in (0, 2):
                out = Guarded(torch, case.total, torch.float32, -7.0, phase)
                out.view.copy_(case.d_x)
                rc = case.fn(sslib, "apply")(*case.head(out.view), plan.view.data_ptr(), out.view.data_ptr(), None)
                assert rc == 0, sslib.ss_last_error_string()
                torch.cuda.synchronize()
                assert np.array_equal(_bits(out.host("out")), _bits(want)), phase
        plan.host("plan")


@pytest.mark.parametrize("pcm", (False, True), ids=("f32", "i16"))
def test_silent_speech_and_silent_noise_have_gain_zero(sslib, pcm):
    import torch

    case = Case(torch, [300, 300, 300, 5], [50, 100], seed=3, pcm=pcm)
    for a, lo, hi in ((case.raw_x, 0, 300), (case.x, 0, 300), (case.raw_nz, 0, 50), (case.nz, 0, 50)):
        a[lo:hi] = 0
    case.d_x, case.d_nz = torch.from_numpy(case.raw_x).cuda(), torch.from_numpy(case.raw_nz).cuda()
    seen = set()
    for epoch in range(6):
        rows, plan = _device_plan(torch, sslib, case, (9, epoch))
        _same_plan(rows, case.plan_ref((9, epoch)))
        assert rows["speech_energy"][0] == 0 and rows["noise_gain"][0] == 0
        silent = rows["noise_clip"] == 0
        assert (rows["noise_energy"][silent] == 0).all() and (rows["noise_gain"][silent] == 0).all()
        seen.update(rows["noise_clip"][1:].tolist())
        out = Guarded(torch, case.total, torch.float32, -7.0, 1)
        assert case.fn(sslib, "apply")(*case.head(), plan.view.data_ptr(), out.view.data_ptr(), None) == 0
        torch.cuda.synchronize()
        got = out.host("out")
        assert np.isfinite(got).all() and (got[:300] == 0).all()
        assert np.array_equal(_bits(got), _bits(case.mix_ref(rows, np.full(case.total, -7.0, np.float32))))
    assert seen == {0, 1}


def test_the_pcm_call_equals_the_float_call_on_the_converted_samples(sslib, cases):
    import torch

    pcm = cases[True]
    flt = Case(torch, pcm=False)
    flt.x, flt.nz, flt.raw_x, flt.raw_nz = pcm.x, pcm.nz, pcm.x, pcm.nz
    flt.d_x, flt.d_nz = torch.from_numpy(pcm.x).cuda(), torch.from_numpy(pcm.nz).cuda()
    for rng in ((120, 5), (131, 5)):
        outs, plans = [], []
        for case in (pcm, flt):
            plan = Guarded(torch, case.n * 5, torch.int64, -99)
            work = Guarded(torch, _work_words(sslib, case), torch.float64, -7.0)
            out = Guarded(torch, case.total, torch.float32, -7.0, 1)
            block = _rng(torch, *rng)
            rc = case.fn(sslib, "mix")(*case.head(), block.data_ptr(), 0, *SCALARS, out.view.data_ptr(), plan.view.data_ptr(), work.view.data_ptr(),
                                       work.count * 8, None)
            assert rc == 0, sslib.ss_last_error_string()
            torch.cuda.synchronize()
            work.host("work")
            assert _words(block) == [rng[0], rng[1] + 1]  # the mix call leaves epoch + 1
            outs.append(out.host("out"))
            plans.append(plan.host("plan"))
        assert np.array_equal(plans[0], plans[1]) and np.array_equal(_bits(outs[0]), _bits(outs[1]))  # every plan word, every output bit
        rows = plans[0].view(m.ROW)
        _same_plan(rows, pcm.plan_ref(rng))
        assert np.array_equal(_bits(outs[0]), _bits(pcm.mix_ref(rows, np.full(pcm.total, -7.0, np.float32))))


def test_a_clip_alone_equals_the_clip_in_the_batch(ss, cases):
    """... at the same clip_base + b, whatever its offset; and a plan applied twice gives equal outputs"""
    import torch

    case = cases[False]
    rng = np.array([120, 3], np.uint64)
    d_x = case.d_x
    block = _rng(torch, 120, 3)
    out, plan = ss.noise_mix_packed(d_x, LENS, case.d_nz, NOISE_LENS, block, *SCALARS[:1], SCALARS[1:3], SCALARS[3:5])
    rows = ss.noise_plan_rows(plan)
    assert _words(block) == [120, 4]
    whole = out.cpu().numpy()
    for b in (3, 7, 9, 10):
        lo, hi = int(case.so[b]), int(case.so[b + 1])
        for lead in (0, 1):  # the clip alone, and behind a one-sample clip (another offset, another alignment)
            sig = torch.cat([torch.zeros(lead, device="cuda"), d_x[lo:hi]])
            o, p = ss.noise_mix_packed(sig, [1] * lead + [hi - lo], case.d_nz, NOISE_LENS, _rng(torch, 120, 3), *SCALARS[:1], SCALARS[1:3], SCALARS[3:5],
                                       clip_base=b - lead)
            assert ss.noise_plan_rows(p)[lead:].tobytes() == rows[b:b + 1].tobytes(), (b, lead)
            assert np.array_equal(_bits(o.cpu().numpy()[lead:]), _bits(whole[lo:hi])), (b, lead)
    again = ss.noise_apply_packed(d_x, LENS, case.d_nz, NOISE_LENS, plan)
    inplace = d_x.clone()
    assert ss.noise_apply_packed(inplace, LENS, case.d_nz, NOISE_LENS, rows, out=inplace) is inplace  # the plan as a host record array
    assert np.array_equal(_bits(again.cpu().numpy()), _bits(whole)) and np.array_equal(_bits(inplace.cpu().numpy()), _bits(whole))
    # the host-pointer form: the same plan, the same samples, the epoch advanced in the caller's words
    o, p = ss.noise_mix_packed(case.x, LENS, case.nz, NOISE_LENS, rng, *SCALARS[:1], SCALARS[1:3], SCALARS[3:5])
    assert p.tobytes() == rows.tobytes() and np.array_equal(_bits(o), _bits(whole)) and rng.tolist() == [120, 4]
    assert np.array_equal(_bits(ss.noise_apply_packed(case.x, LENS, case.nz, NOISE_LENS, p)), _bits(whole))


def test_the_banks_layout_changes_nothing(ss, cases):
    """The other noise clips permuted (the drawn one keeps its index and moves in memory) and the bank re-based in its allocation:
    the same row but for nothing, the same samples."""
    import torch

    case = cases[False]
    b = 10
    lo, hi = int(case.so[b]), int(case.so[b + 1])
    sig = case.d_x[lo:hi]
    for seed in SEEDS:
        o, p = ss.noise_mix_packed(sig, [hi - lo], case.d_nz, NOISE_LENS, _rng(torch, seed, 0), *SCALARS[:1], SCALARS[1:3], SCALARS[3:5], clip_base=b)
        row = ss.noise_plan_rows(p)[0]
        c = int(row["noise_clip"])
        others = [i for i in range(4) if i != c][::-1]
        order = [others.pop(0) if i != c else c for i in range(4)]
        assert order != list(range(4)) and order[c] == c
        clips = [case.nz[int(case.no[i]):int(case.no[i + 1])] for i in order]
        room = torch.zeros(case.total_noise + 5, device="cuda")
        room[5:] = torch.from_numpy(np.concatenate(clips)).cuda()
        o2, p2 = ss.noise_mix_packed(sig, [hi - lo], room[5:], [len(v) for v in clips], _rng(torch, seed, 0), *SCALARS[:1], SCALARS[1:3], SCALARS[3:5], clip_base=b)
        assert ss.noise_plan_rows(p2).tobytes() == ss.noise_plan_rows(p).tobytes() and np.array_equal(_bits(o2.cpu().numpy()), _bits(o.cpu().numpy())), seed


def test_bad_segments_and_bad_rows_are_contained(sslib):
    import torch

    case = Case(torch, [100, 0, 110, 50], [7, 300], seed=5)
    #         good [0, 100) | reversed [100, 90) | good [90, 200): its first ten samples lie in clip 0 as well | ends past the 260 samples
    case.so = np.array([0, 100, 90, 200, 300], np.int64)
    case.d_so = torch.from_numpy(case.so).cuda()
    rng = (77, 0)
    rows, plan = _device_plan(torch, sslib, case, rng)
    want = case.plan_ref(rng)
    assert rows["noise_clip"].tolist()[1] == -2 and rows["noise_clip"][3] == -2 and (rows["noise_clip"][[0, 2]] >= 0).all()
    for b in (1, 3):
        assert rows[b]["speech_gain"] == 0 and rows[b]["noise_gain"] == 0 and rows[b]["speech_energy"] == 0 and rows[b]["start"] == 0
    _same_plan(rows, want)
    # the neighbours: clip 0 as the clip alone, clip 2 on the samples that are its own alone
    alone = Case(torch, [100], [7, 300], seed=5)
    alone.x, alone.d_x = case.x[:100], case.d_x[:100].clone()
    solo, _ = _device_plan(torch, sslib, alone, rng)
    assert solo.tobytes() == rows[:1].tobytes()
    out = Guarded(torch, case.total, torch.float32, -7.0, 1)
    assert case.fn(sslib, "apply")(*case.head(), plan.view.data_ptr(), out.view.data_ptr(), None) == 0
    torch.cuda.synchronize()
    got = out.host("out")
    held = np.full(case.total, -7.0, np.float32)
    first = m.mix_ref(case.x, [0, 100], case.total, case.nz, case.no, case.total_noise, rows[:1], held)
    third = m.mix_ref(case.x, [90, 200], case.total, case.nz, case.no, case.total_noise, rows[2:3], held)
    assert np.array_equal(_bits(got[:90]), _bits(first[:90])) and np.array_equal(_bits(got[100:200]), _bits(third[100:200]))
    shared = slice(90, 100)  # a sample in two segments is mixed as part of one of them
    assert ((_bits(got[shared]) == _bits(first[shared])) | (_bits(got[shared]) == _bits(third[shared]))).all()
    assert (got[200:] == -7.0).all()  # in no good clip: left unwritten
    # a caller's plan: noise_clip past the bank, below -2, a start at and past the clip's length, a negative start -- not mixed
    good = Case(torch, [100, 0, 110, 50], [7, 300], seed=5)
    own = np.zeros(4, m.ROW)
    own["speech_gain"], own["noise_gain"] = [2.0, 1.0, 0.5, -1.0], 3.0
    for clips, starts in (([2, 0, 7, -3], [0, 0, 0, 0]), ([0, 0, 1, 1], [7, 0, 300, -1]), ([0, 1, 1, 0], [2 ** 31 - 1, 0, -2 ** 31, 8])):
        own["noise_clip"], own["start"] = clips, starts
        d_plan = torch.from_numpy(own.view(np.int64).copy()).cuda()
        out = Guarded(torch, good.total, torch.float32, -7.0, 2)
        assert good.fn(sslib, "apply")(*good.head(), d_plan.data_ptr(), out.view.data_ptr(), None) == 0
        torch.cuda.synchronize()
        gains = np.repeat(own["speech_gain"], [100, 0, 110, 50])
        assert np.array_equal(_bits(out.host("out")), _bits(gains * good.x)), clips
    own["noise_clip"], own["start"] = [0, 0, 1, -2], [6, 0, 299, 0]  # the last valid starts mix, and -2 leaves its clip alone
    d_plan = torch.from_numpy(own.view(np.int64).copy()).cuda()
    out = Guarded(torch, good.total, torch.float32, -7.0)
    assert good.fn(sslib, "apply")(*good.head(), d_plan.data_ptr(), out.view.data_ptr(), None) == 0
    torch.cuda.synchronize()
    got = out.host("out")
    assert np.array_equal(_bits(got), _bits(good.mix_ref(own, np.full(good.total, -7.0, np.float32))))
    assert (got[210:] == -7.0).all() and not np.array_equal(got[:100], 2 * good.x[:100])


def test_a_captured_graph_draws_fresh_noise_on_every_replay(ss, cases):
    """NoiseMix with device_tables, captured after a warm-up outside the capture and replayed twice with no host involvement: two
    different plans, each the restatement's at its epoch (the second carries into the high dword)."""
    import torch

    case = cases[False]
    e = 2 ** 32 - 1
    mix = ss.NoiseMix(120, case.nz, NOISE_LENS, epoch=e - 1)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up outside the capture: it takes one epoch
        mix(case.d_x, None, *SCALARS[:1], SCALARS[1:3], SCALARS[3:5], device_tables=case.d_so)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert (mix.seed, mix.epoch) == (120, e)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out, plan = mix(case.d_x, None, *SCALARS[:1], SCALARS[1:3], SCALARS[3:5], device_tables=case.d_so)
    assert mix.epoch == e  # capturing runs nothing
    seen = []
    for k in range(2):
        g.replay()
        torch.cuda.synchronize()
        rows = ss.noise_plan_rows(plan)
        _same_plan(rows, case.plan_ref((120, e + k)))
        assert np.array_equal(_bits(out.cpu().numpy()), _bits(case.mix_ref(rows, np.zeros(case.total, np.float32))))
        assert mix.epoch == e + k + 1
        seen.append(rows.tobytes())
    assert seen[0] != seen[1]


def test_the_mixed_samples_go_on_to_the_front_end(ss):
    """noise_mix_packed -> kaldi_fbank_packed on the same (signal, lengths) equals the front end on the restatement's mixed samples"""
    import torch

    lens = [4097, 40000, 2049, 401]
    case = Case(torch, lens, NOISE_LENS, seed=11)
    mix = ss.NoiseMix(131, case.d_nz, NOISE_LENS)
    out, plan = mix(case.d_x, lens, 0.7, (10, 30), (-6, 6))
    want = case.mix_ref(ss.noise_plan_rows(plan), np.zeros(case.total, np.float32))
    assert np.array_equal(_bits(out.cpu().numpy()), _bits(want)) and mix.epoch == 1
    rows, fo = ss.kaldi_fbank_packed(out, lens, input_scale=32768.0)
    ref, fo_ref = ss.kaldi_fbank_packed(torch.from_numpy(want).cuda(), lens, input_scale=32768.0)
    assert np.array_equal(fo, fo_ref) and rows.shape[0] == int(fo[-1]) > 0
    assert np.array_equal(_bits(rows.cpu().numpy()), _bits(ref.cpu().numpy()))
