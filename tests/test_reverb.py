"""Reverberation of packed clips on the device: ss_reverb_plan_packed_device, ss_reverb_apply_packed*, ss_reverb_packed* and the
Python front's ReverbBank, reverb_plan_packed, reverb_apply_packed, reverb_packed and Reverb.

The output is held to the f64 direct sum over the taps the handle returns (tests/reverb_model.py) by the project's block metric,
max |got - want| / max |want| <= 1e-4 per clip; everything the header calls exact -- a clip against itself at another place, the
copies, the PCM forms, the host forms, the plans -- is compared as bit patterns.  Blocks are laid out with a lead, a tail and gap
segments (clips whose rows are -2 in the caller's plan) so that clips start at even and odd offsets and anything written outside a
clip shows.
"""
import numpy as np
import pytest

import reverb_model as m

pytestmark = pytest.mark.gpu

SENTINEL = np.float32(-7.0)
LONG_GROUPS = 2 * 8 * m.N + 1  # more than two passes of a workgroup (eight block pairs each)
CLIPS = m.CLIP_LENS + [LONG_GROUPS]
PCM = 2.0 ** -15


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _layout(lens, lead, gaps):
    """offsets of a block: `lead` samples in no clip, then clip, gap segment, clip, .. (gap k has gaps[k % len] samples), then a tail of
    5 samples in no clip -> (so, clip index of every real clip, total)"""
    so, real = [lead], []
    for k, n in enumerate(lens):
        real.append(len(so) - 1)
        so.append(so[-1] + n)
        so.append(so[-1] + gaps[k % len(gaps)])
    return np.array(so, np.int64), real, so[-1] + 5


def _block(clips, so, real, total, fill):
    x = np.full(total, fill, np.float32)
    for c, b in zip(clips, real):
        x[so[b]:so[b + 1]] = c
    return x


def _split(x, lens):
    at = np.concatenate([[0], np.cumsum(lens)])
    return [x[at[i]:at[i + 1]] for i in range(len(lens))]


def _plan(n, real, rirs, shifts):
    plan = np.zeros(n, m.ROW)
    plan["rir"] = -2
    for b, r, s in zip(real, rirs, shifts):
        plan[b] = (r, s)
    return plan


@pytest.fixture(scope="module")
def banks(ss):
    """the responses of the model's list and the longest one the stage serves, aligned to their peaks and not"""
    hs = [m.response(k, p, i) for i, (k, p) in enumerate(zip(m.RIR_LENS, m.RIR_PEAKS))] + [m.response(m.LONG_RIR, 8000, 99)]
    packed, lens = np.concatenate(hs), [h.size for h in hs]
    return {align: ss.ReverbBank(packed, lens, normalize="energy", align_peak=align) for align in (True, False)}


@pytest.fixture(scope="module")
def signals():
    return {kind: _split(m.speech(CLIPS, kind, seed=3), CLIPS) for kind in ("noise", "tone")}


def _apply(ss, torch, bank, x, so, total, plan, out_fill=SENTINEL, pcm_scale=None):
    d_x = torch.from_numpy(x).cuda()
    d_out = torch.full((total,), float(out_fill), dtype=torch.float32, device="cuda")
    got = ss.reverb_apply_packed(d_x, None, bank, plan, pcm_scale=pcm_scale, out=d_out, device_tables=torch.from_numpy(so).cuda())
    assert got is d_out
    return d_out.cpu().numpy()


def _outside_untouched(out, so, real, fill=SENTINEL):
    keep = np.ones(out.size, bool)
    for b in real:
        keep[so[b]:so[b + 1]] = False
    assert (out[keep] == fill).all()


@pytest.mark.parametrize("align", [True, False])
@pytest.mark.parametrize("kind", ["noise", "tone"])
def test_parity_with_the_f64_direct_sum(ss, banks, signals, kind, align):
    """every clip length against every response of up to 3000 taps, the lead and the gaps making odd and even offsets"""
    import torch

    bank, clips = banks[align], signals[kind]
    so, real, total = _layout(CLIPS, 3, [1, 2, 5])
    x = _block(clips, so, real, total, np.nan)
    worst = 0.0
    for r in range(len(m.RIR_LENS)):
        taps, peak = bank.rir(r)
        shift = peak if align else 0
        out = _apply(ss, torch, bank, x, so, total, _plan(len(so) - 1, real, [r] * len(CLIPS), [shift] * len(CLIPS)))
        _outside_untouched(out, so, real)
        for c, b in zip(clips, real):
            err = m.block_error(out[so[b]:so[b + 1]], m.conv_ref(c, taps, shift))
            worst = max(worst, err)
            assert err <= m.BAR, (kind, align, r, c.size, err)
    print(f"reverb parity {kind} align={align}: worst block error {worst:.3e}")


@pytest.mark.parametrize("kind", ["noise", "tone"])
def test_parity_of_the_longest_response(ss, banks, kind):
    """16384 taps (32 partitions) on a 3000-sample clip, peak aligned and not, and a delta response"""
    import torch

    x = m.speech([m.LONG_CLIP], kind, seed=5)
    so = np.array([1, 1 + x.size], np.int64)
    blk = _block([x], so, [0], x.size + 6, np.nan)
    r = len(m.RIR_LENS)
    for align in (True, False):
        taps, peak = banks[align].rir(r)
        assert taps.size == m.MAX_TAPS
        shift = peak if align else 0
        out = _apply(ss, torch, banks[align], blk, so, blk.size, np.array([(r, shift)], m.ROW))
        err = m.block_error(out[1:1 + x.size], m.conv_ref(x, taps, shift))
        print(f"reverb parity {kind} K=16384 align={align}: block error {err:.3e}")
        assert err <= m.BAR, err
    delta = np.zeros(700, np.float32)
    delta[600] = 1.0
    for h, align in ((np.ones(1, np.float32), False), (delta, True)):
        bank = ss.ReverbBank(h, [h.size], normalize="none", align_peak=align)
        out = _apply(ss, torch, bank, blk, so, blk.size, np.array([(0, bank.shift(0))], m.ROW))
        assert m.block_error(out[1:1 + x.size], x) <= m.BAR


def test_a_clip_does_not_depend_on_its_place(ss, banks, signals):
    """bit for bit: a packed clip equals the call on that clip alone at offset 0 and at an odd offset, its neighbours NaN or 1e30"""
    import torch

    bank, clips = banks[True], signals["noise"]
    rirs = [b % (len(m.RIR_LENS) + 1) for b in range(len(CLIPS))]
    shifts = [bank.shift(r) for r in rirs]
    so, real, total = _layout(CLIPS, 3, [1, 2, 5])
    packed = {}
    for fill in (np.nan, np.float32(1e30)):
        out = _apply(ss, torch, bank, _block(clips, so, real, total, fill), so, total, _plan(len(so) - 1, real, rirs, shifts))
        _outside_untouched(out, so, real)
        packed[str(fill)] = out
    assert np.array_equal(_bits(packed["nan"]), _bits(packed["1e+30"]))
    for c, b, r, s in zip(clips, real, rirs, shifts):
        for lead in (0, 7):
            so1 = np.array([lead, lead + c.size], np.int64)
            alone = _apply(ss, torch, bank, _block([c], so1, [0], lead + c.size + 5, np.float32(1e30)), so1, lead + c.size + 5, np.array([(r, s)], m.ROW))
            _outside_untouched(alone, so1, [0])
            assert np.array_equal(_bits(alone[lead:lead + c.size]), _bits(packed["nan"][so[b]:so[b + 1]])), (c.size, r, lead)


def test_rows_that_are_not_reverberated(ss, banks):
    """-1 rows are bit copies, -2 rows and samples in no clip keep what out held, out-of-range rows of a caller's plan behave as -1, and
    one plan applied twice gives equal bits"""
    import torch

    bank = banks[True]
    lens = [9, 1030, 2049, 600, 600, 600, 8200]
    x = m.speech(lens, "noise", seed=8)
    xb = _bits(x)
    xb[2], xb[3], xb[4] = 0x7FC12345, 0x80000000, 0x00000001  # a NaN payload, -0.0 and a denormal
    xb[500], xb[501] = 0xFFC54321, 0x807FFFFF
    so = np.concatenate([[2], 2 + np.cumsum(lens)]).astype(np.int64)
    total = int(so[-1]) + 3
    blk = np.full(total, np.float32(0.25), np.float32)
    blk[2:2 + x.size] = x
    n_rir = len(bank)
    plan = np.array([(-1, 0), (-1, 0), (-2, 0), (n_rir, 0), (1, 2), (1, -1), (-5, 0)], m.ROW)  # response 1 has two taps
    out = _apply(ss, torch, bank, blk, so, total, plan)
    again = _apply(ss, torch, bank, blk, so, total, plan)
    assert np.array_equal(_bits(out), _bits(again))
    for b in (0, 1, 3, 4, 5, 6):
        assert np.array_equal(_bits(out[so[b]:so[b + 1]]), _bits(blk[so[b]:so[b + 1]])), b
    assert (out[so[2]:so[3]] == SENTINEL).all() and (out[:2] == SENTINEL).all() and (out[so[-1]:] == SENTINEL).all()
    # tables whose first segment is reversed, or starts below 0, and whose last ends past the block: both unwritten, the good clip served
    taps, _ = bank.rir(2)
    for first in (700, -5):
        bad = np.array([first, 600, 1100, total + 1], np.int64)
        out = _apply(ss, torch, bank, blk, bad, total, np.array([(2, 0), (2, 0), (2, 0)], m.ROW))
        assert m.block_error(out[600:1100], m.conv_ref(blk[600:1100], taps, 0)) <= m.BAR
        assert (out[:600] == SENTINEL).all() and (out[1100:] == SENTINEL).all()


def test_many_clips_share_one_column_of_workgroups(ss, banks):
    """past 4096 clips a clip's groups are all served by one workgroup: two of them, and the copy of a long clip, among empty clips"""
    import torch

    bank = banks[True]
    lens = [0] * 4100
    lens[7], lens[2000], lens[4099] = LONG_GROUPS, 2 * 8 * m.N + 77, 1500
    so = m.table(lens)
    x = m.speech(lens, "noise", seed=9)
    plan = np.zeros(len(lens), m.ROW)
    plan["rir"] = -1
    plan[7] = (6, bank.shift(6))
    plan[4099] = (2, bank.shift(2))
    out = _apply(ss, torch, bank, x, so, x.size, plan)
    for b in (7, 4099):
        taps, _ = bank.rir(int(plan[b]["rir"]))
        assert m.block_error(out[so[b]:so[b + 1]], m.conv_ref(x[so[b]:so[b + 1]], taps, int(plan[b]["shift"]))) <= m.BAR
    assert np.array_equal(_bits(out[so[2000]:so[2001]]), _bits(x[so[2000]:so[2001]]))


def test_the_device_plan_and_the_combined_call(ss, banks):
    """the device plan equals ss_reverb_draws bit for bit, the combined call's output equals apply on that plan, the epoch moves by
    exactly one (with a carry), prob 0 copies every clip and prob 1 reverberates every clip"""
    import torch

    bank = banks[True]
    lens = [700, 0, 1025, 3000, 1, 2048]
    x = m.speech(lens, "noise", seed=12)
    d_x = torch.from_numpy(x).cuda()
    shifts = [bank.shift(c) for c in range(len(bank))]
    for epoch, prob, base in ((0, 0.5, 0), (2 ** 32 - 1, 0.5, 5), (2 ** 32, 1.0, 0), (9, 0.0, 0)):
        aug = ss.SpecAugment(77, epoch)
        want = ss.reverb_draws((77, epoch), lens, bank, prob, base)
        assert np.array_equal(want, m.draws_ref((77, epoch), base, m.table(lens), x.size, shifts, prob))
        rows = ss.reverb_plan_rows(ss.reverb_plan_packed(lens, bank, aug, prob, base))
        assert rows.tobytes() == want.tobytes() and aug.epoch == epoch
        out, plan = ss.reverb_packed(d_x, lens, bank, aug, prob, base)
        torch.cuda.synchronize()
        assert ss.reverb_plan_rows(plan).tobytes() == want.tobytes() and (aug.seed, aug.epoch) == (77, epoch + 1)
        ref = ss.reverb_apply_packed(d_x, lens, bank, want)
        assert np.array_equal(_bits(out.cpu().numpy()), _bits(ref.cpu().numpy()))
        if prob == 0.0:
            assert (want["rir"] == -1).all() and np.array_equal(_bits(out.cpu().numpy()), _bits(x))
        if prob == 1.0:
            assert (want["rir"] >= 0).all()


@pytest.mark.parametrize("scale", [1.0, PCM])
def test_pcm_equals_the_float_call_on_the_converted_samples(ss, banks, scale):
    """outputs and plan bit for bit, the clips at odd sample offsets (2-byte alignment is enough), copies included"""
    import torch

    bank = banks[True]
    lens = [1, 1027, 2500, 333, 9000]
    pcm = np.clip(np.round(m.speech(lens, "noise", seed=21) * 32768.0), -32768, 32767).astype(np.int16)
    conv = pcm.astype(np.float32) * np.float32(scale)
    d_pcm, d_f = torch.from_numpy(np.concatenate([[0], pcm]).astype(np.int16)).cuda()[1:], torch.from_numpy(conv).cuda()
    assert d_pcm.data_ptr() % 4 == 2
    a, b = ss.SpecAugment(5, 3), ss.SpecAugment(5, 3)
    out_i, plan_i = ss.reverb_packed(d_pcm, lens, bank, a, 0.6, pcm_scale=scale)
    out_f, plan_f = ss.reverb_packed(d_f, lens, bank, b, 0.6)
    rows = ss.reverb_plan_rows(plan_i)
    assert rows.tobytes() == ss.reverb_plan_rows(plan_f).tobytes() and set(rows["rir"] >= 0) == {True, False}
    assert np.array_equal(_bits(out_i.cpu().numpy()), _bits(out_f.cpu().numpy()))
    again = ss.reverb_apply_packed(d_pcm, lens, bank, rows, pcm_scale=scale)
    assert np.array_equal(_bits(again.cpu().numpy()), _bits(out_f.cpu().numpy()))


def test_the_host_forms_equal_the_device_forms(ss, banks):
    import torch

    bank = banks[False]
    lens = [513, 0, 4100, 77]
    x = m.speech(lens, "tone")
    rng = np.array([31, 2 ** 32 - 1], np.uint64)
    out, plan = ss.reverb_packed(x, lens, bank, rng, 0.7)
    assert int(rng[1]) == 2 ** 32 and plan.tobytes() == ss.reverb_draws((31, 2 ** 32 - 1), lens, bank, 0.7).tobytes()
    d_out = ss.reverb_apply_packed(torch.from_numpy(x).cuda(), lens, bank, plan)
    assert np.array_equal(_bits(out), _bits(d_out.cpu().numpy()))
    keep = np.full(x.size, SENTINEL, np.float32)
    own = np.array([(0, 0), (-1, 0), (-2, 0), (3, 100)], m.ROW)
    got = ss.reverb_apply_packed(x, lens, bank, own, out=keep)
    d_got = ss.reverb_apply_packed(torch.from_numpy(x).cuda(), lens, bank, own, out=torch.full((x.size,), float(SENTINEL), device="cuda"))
    assert got is keep and np.array_equal(_bits(got), _bits(d_got.cpu().numpy())) and (got[513:4613] == SENTINEL).all()
    pcm = np.clip(np.round(x * 32768.0), -32768, 32767).astype(np.int16)
    got = ss.reverb_apply_packed(pcm, lens, bank, plan, pcm_scale=PCM)
    d_got = ss.reverb_apply_packed(torch.from_numpy(pcm).cuda(), lens, bank, plan, pcm_scale=PCM)
    assert np.array_equal(_bits(got), _bits(d_got.cpu().numpy()))


def test_a_captured_graph_draws_afresh_on_every_replay(ss, banks):
    """Reverb -> noise_mix_packed -> the Kaldi fbank front end on device tables, captured after a warm-up of the same sizes and replayed
    twice over changed tables: the plans differ, each the host's at its epoch, and each replay's reverberated samples equal
    reverb_apply_packed on that plan"""
    import torch

    bank = banks[True]
    tables = [[4000, 1500, 2600], [1500, 2600, 4000], [2600, 4000, 1500]]  # one total, one set of frame counts
    total = sum(tables[0])
    x = m.speech([total], "noise", seed=40)
    nz, nz_lens = m.speech([900, 5000], "noise", seed=41), [900, 5000]
    d_x = torch.from_numpy(x).cuda()
    aug = ss.SpecAugment(2026, 2 ** 32 - 2)
    reverb, mix = ss.Reverb(aug, bank), ss.NoiseMix(2026, nz, nz_lens)
    mix.rng = aug  # one {seed, epoch} block for both stages
    cfg = ss._kaldi_cfg("graph", d_x, False, 16000.0, 25.0, 10.0, 23, 0, 20.0, 0.0, 0.97, 0.0, "povey", 0.42, True, True, False, True, 1.0, 32768.0, {})
    lib = ss._lib.lib()
    frames = [np.empty(4, np.int64) for _ in tables]
    for t, fo in zip(tables, frames):
        assert lib.ss_kaldi_packed_frame_offsets(ss.C.byref(cfg.params), 3, m.table(t).ctypes.data, fo.ctypes.data) == 0
    rows = int(frames[0][-1])
    assert all(int(fo[-1]) == rows for fo in frames)
    d_so, d_fo = torch.from_numpy(m.table(tables[0])).cuda(), torch.from_numpy(frames[0]).cuda()
    feats = torch.zeros((rows, 23), dtype=torch.float32, device="cuda")

    def chain():
        wet, plan = reverb(d_x, None, 0.7, device_tables=d_so)
        noisy, _ = mix(wet, None, 0.5, (10, 30), device_tables=d_so)
        ss._launch(d_x.device, lib.ss_kaldi_fbank_packed_device, cfg.handle, noisy, 3, d_so, d_fo, rows, feats.data_ptr(), None)
        return wet, plan, noisy

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up outside the capture: the bank's spectra go up, two epochs pass
        chain()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    e = 2 ** 32
    assert aug.epoch == e
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        wet, plan, noisy = chain()
    assert aug.epoch == e  # capturing runs nothing
    seen = []
    for k in (1, 2):
        d_so.copy_(torch.from_numpy(m.table(tables[k])).cuda())
        d_fo.copy_(torch.from_numpy(frames[k]).cuda())
        g.replay()
        torch.cuda.synchronize()
        got = ss.reverb_plan_rows(plan)
        assert got.tobytes() == ss.reverb_draws((2026, e), tables[k], bank, 0.7).tobytes() and aug.epoch == e + 2
        ref = ss.reverb_apply_packed(d_x, tables[k], bank, got)
        assert np.array_equal(_bits(wet.cpu().numpy()), _bits(ref.cpu().numpy()))
        want, _ = ss.kaldi_fbank_packed(noisy, tables[k], input_scale=32768.0)
        assert np.array_equal(_bits(feats.cpu().numpy()), _bits(want.cpu().numpy()))
        seen.append(got.tobytes())
        e += 2
    assert seen[0] != seen[1]
