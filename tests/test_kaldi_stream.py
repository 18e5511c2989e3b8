"""The Kaldi front end over a pool of stream states on the device (ss_kstream_*; the sp / spi builds of ss_kaldi_c256).

The contract of the ss_kstream_* section of include/speechsauce_amd.h: all of a stream's rows over all calls, however the stream was
cut into calls, are bit for bit the rows of ss_kaldi_fbank_device / ss_kaldi_mfcc_device on zeros(S) ++ stream; rows D.. meet the f64
restatement of tests/test_kaldi_cpu.py at the bar of tests/test_kaldi.py (block metric 1e-4, taken from there).  Shapes are the
small ones of tests/test_kaldi_stream_cpu.py; every parity test prints the largest figure it met."""
import ctypes as C

import numpy as np
import pytest

from test_kaldi import BAR, KINDS, energy_metric
from test_kaldi_cpu import SS_ERR_ARG, SS_ERR_DEVICE, SS_OK, block_metric, gpu_case_signal, kp, make_kaldi_params, ref_fbank, ref_mfcc
from test_kaldi_stream_cpu import HOPS, HOPS_13, POOL, SHAPES, SLOTS, loop_hops, loop_rows

pytestmark = pytest.mark.gpu
FILL = -7777.0
FBANK, MFCC = dict(num_mel_bins=80, energy_floor=0.0), dict(num_mel_bins=23, num_ceps=13, use_energy=1, energy_floor=0.0)


class Rig:
    """One handle and its sizes; the raw device calls on it."""

    def __init__(self, ss, sslib, mfcc, **cfg):
        self.ss, self.lib, self.mfcc = ss, sslib, mfcc
        self.p = kp(**cfg)
        self.cfg = ss.KaldiConfig(make_kaldi_params(sslib, **cfg))
        S, D, fl, sh, pad = (C.c_size_t() for _ in range(5))
        assert sslib.ss_kstream_state_len(C.byref(self.cfg.params), C.byref(S), C.byref(D)) == SS_OK
        assert sslib.ss_kaldi_sizes(C.byref(self.cfg.params), C.byref(fl), C.byref(sh), C.byref(pad)) == SS_OK
        self.S, self.D, self.flen, self.shift = S.value, D.value, fl.value, sh.value
        self.cols = self.p["num_ceps"] if mfcc else self.p["num_mel_bins"]

    def status(self):
        return self.lib.ss_kaldi_config_device_status(self.cfg.handle)

    def new_pool(self, torch, rows=POOL, named=()):
        """a pool of sentinel rows with the named rows zero (fresh streams)"""
        pool = torch.full((rows, self.S), FILL, dtype=torch.float32, device="cuda")
        if len(named):
            pool[list(named)] = 0
        return pool

    def outs(self, torch, rows):
        return (torch.full((rows, self.cols), FILL, dtype=torch.float32, device="cuda"), torch.full((rows,), FILL, dtype=torch.float32, device="cuda"))

    def raw(self, torch, x, so, ro, total_rows, slots, pool_streams, pool, out, en, scale=None, stream=None, ptr=None):
        """the _device entry point of this rig's kind; tables are device tensors or host arrays -> rc"""
        dev = [t if torch.is_tensor(t) else torch.from_numpy(np.ascontiguousarray(np.asarray(t, dt))).cuda()
               for t, dt in ((so, np.int64), (ro, np.int64), (slots, np.int32))]
        self.keep = dev
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream if stream is None else stream)
        args = [self.cfg.handle, x.data_ptr() if ptr is None else ptr, dev[2].numel(), dev[0].data_ptr(), dev[1].data_ptr(), total_rows,
                dev[2].data_ptr(), pool_streams]
        if scale is not None:
            args.append(scale)
        args += [pool.data_ptr() if pool is not None and self.S else None, out.data_ptr()]
        if not self.mfcc:
            args.append(en.data_ptr() if en is not None else None)
        kind = "mfcc" if self.mfcc else "fbank"
        return getattr(self.lib, f"ss_kstream_{kind}_packed{'_i16' if scale is not None else ''}_device")(*args, st)

    def call(self, torch, chunks, slots, pool, slack=2, scale=None):
        """one call over `chunks` (1-D device tensors) -> (rows, log energy, ro); the slack rows are checked here"""
        lens = [int(c.numel()) for c in chunks]
        assert all(n % self.shift == 0 for n in lens)
        so = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        ro = so // self.shift
        R = int(ro[-1])
        x = torch.cat(chunks) if lens else torch.zeros(0, device="cuda")
        if x.numel() == 0:
            x = torch.zeros(1, dtype=x.dtype, device="cuda")
        out, en = self.outs(torch, R + slack)
        rc = self.raw(torch, x, so, ro, R + slack, slots, int(pool.shape[0]), pool, out, en, scale)
        assert rc == SS_OK, self.lib.ss_last_error_string()
        torch.cuda.synchronize()
        assert (out[R:] == FILL).all() and (en[R:] == FILL).all()  # rows past ro[n_active] are left alone
        if not self.mfcc:
            assert (en[:R] != FILL).all()
        return out[:R], en[:R], ro

    def dense(self, torch, stream_samples):
        """ss_kaldi_*_device on zeros(S) ++ stream -> (rows [K x cols], log energy [K])"""
        x = torch.cat([torch.zeros(self.S, dtype=torch.float32, device="cuda"), stream_samples]).contiguous()
        K = int(stream_samples.numel()) // self.shift
        out, en = self.outs(torch, K)
        if K == 0:
            return out, en
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        if self.mfcc:
            rc = self.lib.ss_kaldi_mfcc_device(self.cfg.handle, x.data_ptr(), 1, x.numel(), x.numel(), out.data_ptr(), st)
        else:
            rc = self.lib.ss_kaldi_fbank_device(self.cfg.handle, x.data_ptr(), 1, x.numel(), x.numel(), out.data_ptr(), en.data_ptr(), st)
        assert rc == SS_OK, self.lib.ss_last_error_string()
        torch.cuda.synchronize()
        assert (out != FILL).all()
        return out, en


def serve(torch, rig, streams, slots, cuts, scale=None):
    """Feeds stream i (pool row slots[i]) cuts[c][i] hops in call c from a fresh pool -> (per-stream rows, per-stream log energies,
    the pool).  scale: the streams are int16 PCM."""
    pool = rig.new_pool(torch, named=slots)
    at = [0] * len(streams)
    rows, ens = [[] for _ in streams], [[] for _ in streams]
    for c, hops in enumerate(cuts):
        chunks = []
        for i, h in enumerate(hops):
            chunks.append(streams[i][at[i]:at[i] + h * rig.shift])
            at[i] += h * rig.shift
        out, en, ro = rig.call(torch, chunks, slots, pool, scale=scale)
        for i in range(len(streams)):
            rows[i].append(out[int(ro[i]):int(ro[i + 1])])
            ens[i].append(en[int(ro[i]):int(ro[i + 1])])
    assert all(a == int(s.numel()) for a, s in zip(at, streams))
    return [torch.cat(r) for r in rows], [torch.cat(e) for e in ens], pool


def three_cuts(totals):
    """the same totals per stream cut three ways: the standard call then the 13-row one, one call, and one-hop calls"""
    assert totals == [a + b for a, b in zip(HOPS, HOPS_13)]
    return [[HOPS, HOPS_13], [totals], [[1 if c < k else 0 for k in totals] for c in range(max(totals))]]


@pytest.mark.parametrize("mfcc", [False, True], ids=["fbank", "mfcc"])
@pytest.mark.parametrize("name", list(SHAPES))
def test_equals_the_dense_call_however_the_stream_is_cut(ss, sslib, name, mfcc):
    import torch

    cfg, flen, shift, NE, D, S = SHAPES[name]
    rig = Rig(ss, sslib, mfcc, **cfg, **(MFCC if mfcc else FBANK))
    assert (rig.flen, rig.shift, rig.D, rig.S) == (flen, shift, D, S)
    totals = [a + b for a, b in zip(HOPS, HOPS_13)]
    host = [gpu_case_signal(300 + i, k * shift, KINDS[i % 3]) for i, k in enumerate(totals)]
    streams = [torch.from_numpy(h).cuda() for h in host]
    want = [rig.dense(torch, s) for s in streams]
    pools = []
    for cuts in three_cuts(totals):
        rows, ens, pool = serve(torch, rig, streams, SLOTS, cuts)
        tag = f"ss_kaldi_c256<{NE},pow2,{'mfcc' if mfcc else 'fbank'},sp>"
        assert sslib.ss_last_kernel_name().decode() == tag
        for i in range(len(streams)):
            assert torch.equal(rows[i], want[i][0]), (name, i)
            if not mfcc:
                assert torch.equal(ens[i], want[i][1]), (name, i)
        pools.append(pool)
    assert rig.status() == SS_OK
    unnamed = [r for r in range(POOL) if r not in SLOTS]
    for pool in pools:
        assert torch.equal(pool, pools[0])
        assert (pool[unnamed] == FILL).all() or S == 0
        for i, s in enumerate(SLOTS):  # the last S samples of zeros(S) ++ stream
            assert torch.equal(pool[s], torch.cat([torch.zeros(S, device="cuda"), streams[i]])[streams[i].numel():])
    # rows D.. against the f64 restatement of the stream itself
    worst = worst_e = 0.0
    for i, k in enumerate(totals):
        if k <= D:
            continue
        got = want[i][0][D:].cpu().numpy()
        if mfcc:
            ref = ref_mfcc(host[i], rig.p)
            worst = max(worst, block_metric(got[:, 0], ref[:, 0]), block_metric(got[:, 1:], ref[:, 1:]))
        else:
            ref, ref_e = ref_fbank(host[i], rig.p)
            worst = max(worst, block_metric(got, ref))
            worst_e = max(worst_e, energy_metric(want[i][1][D:].cpu().numpy(), ref_e))
        assert got.shape == ref.shape
    print(f"kaldi stream pool {name} {'mfcc' if mfcc else 'fbank'}: rows D.. block metric {worst:.3g}, log energy {worst_e:.3g}")
    assert worst <= BAR and worst_e <= BAR


@pytest.mark.parametrize("cfg,mfcc,pcm,tag", [
    (dict(num_mel_bins=80), False, False, "13,pow2,fbank,sp"),
    (dict(num_mel_bins=23, frame_length_ms=20.0, use_power=0), False, True, "10,fbank,spi"),
    (dict(num_mel_bins=80, frame_length_ms=32.0, use_power=0), False, False, "16,fbank,sp"),
    (dict(num_mel_bins=23, num_ceps=13), True, True, "13,pow2,mfcc,spi"),
    (dict(num_mel_bins=23, num_ceps=13, frame_length_ms=32.0), True, False, "16,pow2,mfcc,sp"),
])
def test_dispatch(ss, sslib, cfg, mfcc, pcm, tag):
    import torch

    rig = Rig(ss, sslib, mfcc, **cfg)
    x = torch.from_numpy(gpu_case_signal(1, 3 * rig.shift, "int16")).cuda()
    pool = rig.new_pool(torch, named=[3])
    rows, _, _ = rig.call(torch, [x.to(torch.int16) if pcm else x], [3], pool, scale=1.0 if pcm else None)
    assert sslib.ss_last_kernel_name().decode() == f"ss_kaldi_c256<{tag}>"
    assert torch.equal(rows, rig.dense(torch, x)[0])  # (magnitude builds too)


@pytest.mark.parametrize("mfcc", [False, True], ids=["fbank", "mfcc"])
@pytest.mark.parametrize("name", ["16k_25_10", "11k_25_10", "16k_20_10.1", "16k_25_30"])
def test_pcm_equals_the_float_call(ss, sslib, name, mfcc):
    import torch

    cfg = SHAPES[name][0]
    rig = Rig(ss, sslib, mfcc, **cfg, **(MFCC if mfcc else FBANK))
    totals = [a + b for a, b in zip(HOPS, HOPS_13)]
    rng = np.random.default_rng(17)
    pcm = [torch.from_numpy(rng.integers(-32768, 32768, k * rig.shift).astype(np.int16)).cuda() for k in totals]
    cuts = three_cuts(totals)[0]
    for scale in (1.0, 2.0 ** -15):
        floats = [p.float() * scale for p in pcm]
        rows_f, ens_f, pool_f = serve(torch, rig, floats, SLOTS, cuts)
        rows_i, ens_i, pool_i = serve(torch, rig, pcm, SLOTS, cuts, scale=scale)
        assert sslib.ss_last_kernel_name().decode().endswith(",spi>")
        # a stream fed PCM and floats in turn
        mixed = [[p, f] for p, f in zip(pcm, floats)]
        pool_m = rig.new_pool(torch, named=SLOTS)
        at, rows_m = [0] * len(pcm), [[] for _ in pcm]
        for c, hops in enumerate(cuts):
            kind = c % 2  # call 0 PCM, call 1 floats
            chunks = [mixed[i][kind][at[i]:at[i] + h * rig.shift] for i, h in enumerate(hops)]
            at = [a + h * rig.shift for a, h in zip(at, hops)]
            out, _, ro = rig.call(torch, chunks, SLOTS, pool_m, scale=None if kind else scale)
            for i in range(len(pcm)):
                rows_m[i].append(out[int(ro[i]):int(ro[i + 1])])
        for i in range(len(pcm)):
            assert torch.equal(rows_i[i], rows_f[i]) and torch.equal(torch.cat(rows_m[i]), rows_f[i]), (scale, i)
            assert mfcc or torch.equal(ens_i[i], ens_f[i])
        assert torch.equal(pool_i, pool_f) and torch.equal(pool_m, pool_f)
    # d_x at an odd sample offset: 2-byte aligned only
    chunks = [p[:h * rig.shift] for p, h in zip(pcm, HOPS)]
    want, want_e, ro = rig.call(torch, chunks, SLOTS, rig.new_pool(torch, named=SLOTS), scale=1.0)
    buf = torch.zeros(1 + sum(c.numel() for c in chunks), dtype=torch.int16, device="cuda")
    buf[1:] = torch.cat(chunks)
    so = np.concatenate([[0], np.cumsum([c.numel() for c in chunks])])
    R = int(ro[-1])
    out, en = rig.outs(torch, R)
    assert (buf.data_ptr() + 2) % 4 == 2
    rc = rig.raw(torch, buf, so, ro, R, SLOTS, POOL, rig.new_pool(torch, named=SLOTS), out, en, scale=1.0, ptr=buf.data_ptr() + 2)
    torch.cuda.synchronize()
    assert rc == SS_OK and torch.equal(out, want) and (mfcc or torch.equal(en, want_e))
    # a scale that is no power of two: SS_ERR_ARG, nothing touched
    pool = rig.new_pool(torch, named=SLOTS)
    out, en = rig.outs(torch, R)
    for bad in (3.0, 0.0, -1.0, float("inf"), 2.0 ** 65):
        assert rig.raw(torch, buf, so, ro, R, SLOTS, POOL, pool, out, en, scale=bad) == SS_ERR_ARG
    torch.cuda.synchronize()
    assert (out == FILL).all() and (en == FILL).all() and torch.equal(pool, rig.new_pool(torch, named=SLOTS))
    assert rig.status() == SS_OK


@pytest.mark.parametrize("name", ["16k_25_10", "16k_25_10.1", "16k_20_10.1", "11k_25_10"])
def test_place_independence(ss, sslib, name):
    """The same entry -- the same chunk on the same carried state -- at another position, beside other neighbours, at another slot and
    with its chunk at an odd sample offset gives the same bits."""
    import torch

    rig = Rig(ss, sslib, False, **SHAPES[name][0], **FBANK)
    sh = rig.shift
    mine = torch.from_numpy(gpu_case_signal(70, 5 * sh, "scaled")).cuda()
    others = [torch.from_numpy(gpu_case_signal(71 + i, k * sh, KINDS[i % 3])).cuda() for i, k in enumerate([1, 0, 3, 2, 0, 1])]

    def run(slot, before, after, shift_base=0):
        """two calls: 2 hops alone (the state), then 3 hops between `before` and `after`"""
        pool = rig.new_pool(torch, named=range(POOL))
        rig.call(torch, [mine[:2 * sh]], [slot], pool)
        chunks = before + [mine[2 * sh:]] + after
        slots = [s for s in range(POOL) if s != slot][:len(before)] + [slot] + [s for s in range(POOL) if s != slot][len(before):len(chunks) - 1]
        if shift_base:  # the whole block one sample further on: a buffer that is 4-byte but not 8-byte aligned
            lens = [int(c.numel()) for c in chunks]
            so = np.concatenate([[0], np.cumsum(lens)])
            ro = so // sh
            buf = torch.zeros(1 + int(so[-1]), device="cuda")
            buf[1:] = torch.cat(chunks)
            out, en = rig.outs(torch, int(ro[-1]))
            assert rig.raw(torch, buf, so, ro, int(ro[-1]), slots, POOL, pool, out, en, ptr=buf.data_ptr() + 4) == SS_OK
            torch.cuda.synchronize()
        else:
            out, en, ro = rig.call(torch, chunks, slots, pool)
        k = len(before)
        return out[int(ro[k]):int(ro[k + 1])].clone(), en[int(ro[k]):int(ro[k + 1])].clone(), pool[slot].clone()

    base = run(0, [], [])
    assert base[0].shape[0] == 3
    for slot, before, after, off in ((0, others[:3], others[3:], 0), (13, others[:1], [], 0), (7, others[3:], others[:3], 0), (5, others[:4], others[4:], 1),
                                     (2, [], others[:2], 1)):
        got = run(slot, before, after, off)
        assert all(torch.equal(a, b) for a, b in zip(got, base)), (slot, len(before), off)
    if sh % 2:
        assert sum(int(c.numel()) for c in others[:1]) % 2 == 1  # (odd shift: the chunk behind one hop starts at an odd so)


CONTAIN_HOPS = [2, 1, 3, 1, 2]
CONTAIN_SLOTS = [5, 0, 7, 2, 4]


@pytest.mark.parametrize("where", ["interior", "last"])
@pytest.mark.parametrize("kind", ["not_whole_hops", "ro_inconsistent", "past_total_rows", "slot_out_of_range"])
@pytest.mark.parametrize("pcm", [False, True], ids=["float", "pcm"])
def test_containment(ss, sslib, kind, where, pcm):
    """One bad entry per call, every buffer allocated exactly to size and the last entry ending on the buffer's last sample: the bad
    entry's rows and pool row keep what they held, every other entry is bit-exact, the handle reports SS_ERR_DEVICE once.  A
    contract check over valid memory throughout."""
    import torch

    rig = Rig(ss, sslib, False, **FBANK)
    sh, n, P = rig.shift, len(CONTAIN_HOPS), 8
    bad = 2 if where == "interior" else n - 1
    scale = 1.0 if pcm else None
    chunks = [torch.from_numpy(gpu_case_signal(80 + i, h * sh, "int16")).cuda() for i, h in enumerate(CONTAIN_HOPS)]
    state = torch.from_numpy(gpu_case_signal(90, P * rig.S, "int16").reshape(P, rig.S)).cuda()
    typed = [c.to(torch.int16) for c in chunks] if pcm else chunks
    clean_pool = state.clone()
    clean, clean_e, ro0 = rig.call(torch, typed, CONTAIN_SLOTS, clean_pool, slack=0, scale=scale)
    assert rig.status() == SS_OK
    lens = [int(c.numel()) for c in typed]
    claimed = list(CONTAIN_HOPS)
    slots = list(CONTAIN_SLOTS)
    skipped = {bad}
    if kind == "not_whole_hops":
        typed = list(typed)
        typed[bad] = torch.cat([typed[bad], typed[bad][:3]])
        lens[bad] += 3
    elif kind == "ro_inconsistent":
        claimed[bad] += 1
    elif kind == "slot_out_of_range":
        slots[bad] = P if where == "interior" else -1
    so = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    ro = np.concatenate([[0], np.cumsum(claimed)]).astype(np.int64)
    total_rows = int(ro[-1])
    if kind == "past_total_rows":
        total_rows = int(ro[bad + 1]) - 1  # the entry, and every one behind it, ends past the block
        skipped = set(range(bad, n))
    x = torch.cat(typed)
    assert x.numel() == int(so[-1])
    pool = state.clone()
    out, en = rig.outs(torch, total_rows)
    rc = rig.raw(torch, x, so, ro, total_rows, slots, P, pool, out, en, scale=scale)
    assert rc == SS_OK, sslib.ss_last_error_string()  # the tables are device data: the call itself cannot know
    torch.cuda.synchronize()
    for i in range(n):
        lo, hi = int(ro[i]), min(int(ro[i + 1]), total_rows)
        if i in skipped:
            assert (out[lo:hi] == FILL).all() and (en[lo:hi] == FILL).all(), i
            if 0 <= CONTAIN_SLOTS[i] < P:
                assert torch.equal(pool[CONTAIN_SLOTS[i]], state[CONTAIN_SLOTS[i]]), i
        else:
            assert torch.equal(out[lo:hi], clean[int(ro0[i]):int(ro0[i + 1])]), i
            assert torch.equal(en[lo:hi], clean_e[int(ro0[i]):int(ro0[i + 1])]), i
            assert torch.equal(pool[CONTAIN_SLOTS[i]], clean_pool[CONTAIN_SLOTS[i]]), i
    named = {CONTAIN_SLOTS[i] for i in range(n) if i not in skipped}
    for r in range(P):
        if r not in named:
            assert torch.equal(pool[r], state[r]), r
    assert rig.status() == SS_ERR_DEVICE
    assert rig.status() == SS_OK
    again, _, _ = rig.call(torch, [c.to(torch.int16) for c in chunks] if pcm else chunks, CONTAIN_SLOTS, state.clone(), slack=0, scale=scale)
    assert torch.equal(again, clean) and rig.status() == SS_OK  # the handle serves the next clean call


def test_argument_rules(ss, sslib):
    import torch

    rig = Rig(ss, sslib, False, **FBANK)
    fb_only = Rig(ss, sslib, True, num_mel_bins=23, num_ceps=0)
    x = torch.zeros(2 * rig.shift, device="cuda")
    so, ro, slots = [0, 2 * rig.shift], [0, 2], [1]
    pool = rig.new_pool(torch, rows=4)
    out, en = rig.outs(torch, 2)
    assert rig.raw(torch, x, so[:1], ro[:1], 0, [], 4, pool, out, en) == SS_OK  # no entries: no launch
    assert fb_only.raw(torch, x, so, ro, 2, slots, 4, pool, out, None) == SS_ERR_ARG  # num_ceps == 0 on an MFCC call
    assert rig.raw(torch, x, so, ro, 2, slots, 4, None, out, en) == SS_ERR_ARG  # null pool with S > 0
    assert rig.raw(torch, x, so, ro, 1 << 31, slots, 4, pool, out, en) == SS_ERR_ARG
    assert rig.raw(torch, x, so, ro, 2, slots, 1 << 31, pool, out, en) == SS_ERR_ARG
    both = torch.full((4 * rig.S + 2 * 80,), FILL, device="cuda")  # the output inside the pool's range
    assert rig.raw(torch, x, so, ro, 2, slots, 4, both, both[rig.S:], en) == SS_ERR_ARG
    torch.cuda.synchronize()
    assert (pool == FILL).all() and (out == FILL).all() and (en == FILL).all() and (both == FILL).all()
    assert rig.status() == SS_OK


@pytest.mark.parametrize("mfcc,pcm", [(False, False), (True, True)], ids=["fbank_sp", "mfcc_spi"])
def test_persistent_loop(ss, sslib, mfcc, pcm):
    """4 (3 * 12 * CUs + 5) + 1 rows over 64 entries: every wave goes round the loop, claims again and prefetches behind pass 1."""
    import torch

    cus = torch.cuda.get_device_properties(0).multi_processor_count
    rig = Rig(ss, sslib, mfcc, **(MFCC if mfcc else FBANK))
    hops = loop_hops(cus)
    assert sum(hops) == loop_rows(cus)
    rng = np.random.default_rng(3)
    total = sum(hops) * rig.shift
    if pcm:
        x = torch.from_numpy(rng.integers(-32768, 32768, total).astype(np.int16)).cuda()
    else:
        x = torch.from_numpy((rng.standard_normal(total) * 0.1).astype(np.float32)).cuda()
    so = np.concatenate([[0], np.cumsum(np.asarray(hops) * rig.shift)])
    chunks = [x[int(so[i]):int(so[i + 1])] for i in range(64)]
    slots = rng.permutation(64).tolist()
    pool = rig.new_pool(torch, rows=64, named=range(64))
    out, en, ro = rig.call(torch, chunks, slots, pool, slack=3, scale=1.0 if pcm else None)
    assert sslib.ss_last_kernel_name().decode().endswith(",spi>" if pcm else ",sp>")
    for i in range(64):
        want, want_e = rig.dense(torch, chunks[i].float())
        assert torch.equal(out[int(ro[i]):int(ro[i + 1])], want), i
        assert mfcc or torch.equal(en[int(ro[i]):int(ro[i + 1])], want_e), i
        if hops[i]:
            assert torch.equal(pool[slots[i]], torch.cat([torch.zeros(rig.S, device="cuda"), chunks[i].float()])[chunks[i].numel():])
    assert rig.status() == SS_OK


def test_graph_replay_over_changing_tables_equals_eager_calls(ss, sslib):
    import torch

    rig = Rig(ss, sslib, False, **FBANK)
    N, CAP, sh = len(HOPS), 16, 160
    x = torch.zeros(CAP * sh, device="cuda")
    d_so, d_ro = torch.zeros(N + 1, dtype=torch.int64, device="cuda"), torch.zeros(N + 1, dtype=torch.int64, device="cuda")
    d_sl = torch.arange(N, dtype=torch.int32, device="cuda")
    out, en = rig.outs(torch, CAP)
    pool_g = torch.zeros((POOL, rig.S), device="cuda")
    pool_e = pool_g.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up outside the capture, on a side stream (the zero tables are N entries without rows)
        assert rig.raw(torch, x, d_so, d_ro, CAP, d_sl, POOL, pool_g.clone(), out, en, stream=side.cuda_stream) == SS_OK
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        assert rig.raw(torch, x, d_so, d_ro, CAP, d_sl, POOL, pool_g, out, en) == SS_OK
    rng = np.random.default_rng(8)
    for k, hops in enumerate((HOPS, HOPS_13, [3, 0, 0, 2, 1, 4, 0, 0, 5])):
        slots = rng.permutation(POOL)[:N].astype(np.int32) if k else np.asarray(SLOTS, np.int32)
        so = np.concatenate([[0], np.cumsum(np.asarray(hops) * sh)]).astype(np.int64)
        ro = so // sh
        xs = torch.from_numpy(gpu_case_signal(60 + k, int(so[-1]), KINDS[k])).cuda()
        want, want_e, _ = rig.call(torch, [xs[int(so[i]):int(so[i + 1])] for i in range(N)], slots.tolist(), pool_e)
        x[:xs.numel()] = xs
        d_so.copy_(torch.from_numpy(so))
        d_ro.copy_(torch.from_numpy(ro))
        d_sl.copy_(torch.from_numpy(slots))
        out.fill_(FILL)
        en.fill_(FILL)
        g.replay()
        torch.cuda.synchronize()
        R = int(ro[-1])
        assert torch.equal(out[:R], want) and torch.equal(en[:R], want_e), k
        assert (out[R:] == FILL).all() and (en[R:] == FILL).all()
        assert torch.equal(pool_g, pool_e), k
    assert rig.status() == SS_OK


@pytest.mark.parametrize("mfcc", [False, True], ids=["fbank", "mfcc"])
def test_forms(ss, sslib, mfcc):
    """The host forms equal the device forms; the Python classes equal the ctypes path, for torch and numpy; reset() zeroes exactly the
    named rows."""
    import torch

    rig = Rig(ss, sslib, mfcc, **(MFCC if mfcc else FBANK))
    sh = rig.shift
    host = [gpu_case_signal(40 + i, h * sh, KINDS[i % 3]) for i, h in enumerate(HOPS)]
    pcm = [np.round(h).astype(np.int16) if KINDS[i % 3] != "unit" else np.round(h * 32768).astype(np.int16) for i, h in enumerate(host)]
    state = gpu_case_signal(50, POOL * rig.S, "unit").reshape(POOL, rig.S)
    so = np.concatenate([[0], np.cumsum([len(h) for h in host])]).astype(np.int64)
    sl = np.asarray(SLOTS, np.int32)
    R = int(so[-1]) // sh
    kind = "mfcc" if mfcc else "fbank"
    kw = dict(num_mel_bins=rig.p["num_mel_bins"], energy_floor=0.0)
    if mfcc:
        kw.update(num_ceps=13, use_energy=True)
    cls = ss.KaldiMfccStreamPool if mfcc else ss.KaldiFbankStreamPool
    for scale in (None, 2.0 ** -15):
        parts = host if scale is None else pcm
        pool_d = torch.from_numpy(state).cuda()
        dev, dev_e, ro = rig.call(torch, [torch.from_numpy(c).cuda() for c in parts], SLOTS, pool_d, slack=0, scale=scale)
        # the host form
        xh = np.concatenate(parts)
        pool_h = state.copy()
        out_h, en_h = np.full((R, rig.cols), FILL, np.float32), np.full(R, FILL, np.float32)
        args = [rig.cfg.handle, xh.ctypes.data, len(SLOTS), so.ctypes.data, sl.ctypes.data, POOL] + ([scale] if scale else []) + \
               [pool_h.ctypes.data, out_h.ctypes.data] + ([] if mfcc else [en_h.ctypes.data])
        fn = getattr(sslib, f"ss_kstream_{kind}_packed{'_i16' if scale else ''}")
        dup = sl.copy()
        dup[4] = dup[1]
        bad = list(args)
        bad[4] = dup.ctypes.data
        assert fn(*bad) == SS_ERR_ARG and b"entry 4" in sslib.ss_last_error_string()  # a slot named twice
        odd = so.copy()
        odd[3] += 8
        bad = list(args)
        bad[3] = odd.ctypes.data
        assert fn(*bad) == SS_ERR_ARG and b"entry 2" in sslib.ss_last_error_string()  # a partial hop: the first bad entry is named
        assert np.array_equal(pool_h, state) and (out_h == FILL).all()
        assert fn(*args) == SS_OK, sslib.ss_last_error_string()
        np.testing.assert_array_equal(out_h, dev.cpu().numpy())
        np.testing.assert_array_equal(pool_h, pool_d.cpu().numpy())
        if not mfcc:
            np.testing.assert_array_equal(en_h, dev_e.cpu().numpy())
        # the Python classes, torch and numpy
        for to in (lambda a: torch.from_numpy(a).cuda(), lambda a: a):
            pool = cls(POOL, **kw)
            assert (pool.state_len, pool.delay_rows) == (rig.S, rig.D)
            pool(to(xh), so, SLOTS, pcm_scale=scale)  # (places the pool)
            pool.state[...] = to(state)
            got = pool(to(xh), so if scale else [len(c) for c in parts], SLOTS, pcm_scale=scale, **({} if mfcc else {"with_energy": True}))
            if hasattr(got[0], "cpu"):
                torch.cuda.synchronize()
            arr = [a.cpu().numpy() if hasattr(a, "cpu") else a for a in got]
            np.testing.assert_array_equal(arr[0], out_h)
            np.testing.assert_array_equal(arr[-1], ro)
            if not mfcc:
                np.testing.assert_array_equal(arr[1], en_h)
            st = pool.state.cpu().numpy() if hasattr(pool.state, "cpu") else pool.state
            np.testing.assert_array_equal(st, pool_h)
            pool.reset([SLOTS[3], SLOTS[7]])
            st = pool.state.cpu().numpy() if hasattr(pool.state, "cpu") else pool.state
            want = pool_h.copy()
            want[[SLOTS[3], SLOTS[7]]] = 0
            np.testing.assert_array_equal(st, want)
    assert rig.status() == SS_OK


def test_chain_into_cmvn_and_add_deltas(ss):
    """Kaldi pool -> CmvnStreamPool -> AddDeltasStreamPool on one set of row_offsets / slots, new streams primed as documented: the
    result equals those two stages fed the dense call's rows."""
    import torch

    M, sh = 23, 160
    kpool = ss.KaldiFbankStreamPool(POOL, num_mel_bins=M)
    D = kpool.delay_rows
    cm_a, cm_b = ss.CmvnStreamPool(POOL, M, win_size=5), ss.CmvnStreamPool(POOL, M, win_size=5)
    de_a, de_b = ss.AddDeltasStreamPool(POOL, M), ss.AddDeltasStreamPool(POOL, M)
    totals = [a + b for a, b in zip(HOPS, HOPS_13)]
    streams = [torch.from_numpy(gpu_case_signal(20 + i, (D + k) * sh, KINDS[i % 3])).cuda() for i, k in enumerate(totals)]
    # priming: the first D hops of every new stream go through a call of their own whose rows are discarded
    kpool([s[:D * sh] for s in streams], None, SLOTS)
    at = [D * sh] * len(streams)
    got = [[] for _ in streams]
    ref = [[] for _ in streams]
    # K - D offline frames = the rows behind the warm-up rows
    dense = [ss.kaldi_fbank(s, num_mel_bins=M) if k else torch.zeros((0, M), device="cuda") for s, k in zip(streams, totals)]
    done = [0] * len(streams)
    for hops in (HOPS, HOPS_13):
        chunks = [s[a:a + h * sh] for s, a, h in zip(streams, at, hops)]
        at = [a + h * sh for a, h in zip(at, hops)]
        rows, ro = kpool(chunks, None, SLOTS)
        out = de_a(cm_a(rows, ro, SLOTS), ro, SLOTS)
        want_rows = torch.cat([dense[i][done[i]:done[i] + h] for i, h in enumerate(hops)])
        done = [d + h for d, h in zip(done, hops)]
        assert torch.equal(rows, want_rows)
        want = de_b(cm_b(want_rows, ro, SLOTS), ro, SLOTS)
        assert torch.equal(out, want)
    assert done == [int(d.shape[0]) for d in dense]
