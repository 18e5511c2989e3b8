"""The resampler on the GPU (ss_resample* in include/speechsauce_amd.h): parity with the f64 restatement of
tests/test_resample_cpu.py at a derived bar, the bit-exact invariants (packed == dense == host == PCM, place and neighbours do not
matter), containment under bad tables, the pool invariant (any cut of a stream + flush == the packed call on the whole clip), and
graph capture of the resample -> MFCC chain and of the pool call."""
import ctypes as C

import numpy as np
import pytest

from common import rel as _rel
from test_resample_cpu import ref_filter, ref_out_len, ref_resample, ref_sizes

pytestmark = pytest.mark.gpu

RATIOS = {"3/1": (48000, 16000), "1/2": (8000, 16000), "2/1": (16000, 8000), "7/5": (7, 5), "441/160": (44100, 16000),
          "160/147": (16000, 14700)}
CANARY = np.float32(-7.25e9)


def _bits(a):
    a = a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _noise(rng, n, scale=0.1):
    return (rng.standard_normal(n) * scale).astype(np.float32)


def _info(ss, orig, new):
    return ss._get_resampler(orig, new).info


def _bound(x, orig, new):
    """|got - want| <= (c + 3) 2^-24 sum_k |h[i][k]| max|x| per output: gamma_c of the chain of c = count[i] fmas, the table's rounding
    and the final rounding."""
    o, n, width, h, _ = ref_filter(orig, new)
    s = ref_sizes(orig, new)
    per_phase = (s["count"] + 3) * 2.0 ** -24 * np.abs(h).sum(axis=1) * float(np.abs(x).max() if len(x) else 0.0)
    m = ref_out_len(o, n, len(x))
    return per_phase[np.arange(m) % n]


def _lengths(info, o, n, width):
    tile_in = info.tile_outputs * o // n  # input samples under one workgroup tile
    assert tile_in * n == info.tile_outputs * o
    lens = [1, o - 1, o, o + 1, width, 2 * width + o, tile_in - 1, tile_in, tile_in + 1, 3 * tile_in + 17]
    return [L for L in lens if L > 0]


@pytest.fixture(scope="module")
def parity_case(ss):
    """Per ratio, computed once and left unchanged: the clips, the packed device result and the f64 references."""
    import torch

    cache = {}

    def get(name):
        if name not in cache:
            orig, new = RATIOS[name]
            info = _info(ss, orig, new)
            o, n, width = info.o, info.n, info.width
            rng = np.random.default_rng(sum(ord(ch) for ch in name))
            lens = _lengths(info, o, n, width)
            clips = [_noise(rng, L) for L in lens]
            out, out_lens = ss.resample_packed(torch.from_numpy(np.concatenate(clips)).cuda(), lens, orig, new)
            torch.cuda.synchronize()
            want = [ref_resample(c, orig, new) for c in clips]
            cache[name] = dict(orig=orig, new=new, info=info, lens=lens, clips=clips, out=out.cpu().numpy(), out_lens=out_lens, want=want)
        return cache[name]

    return get


@pytest.mark.parametrize("name", sorted(RATIOS))
def test_packed_parity_with_the_f64_restatement(ss, parity_case, name):
    c = parity_case(name)
    orig, new, o, n = c["orig"], c["new"], c["info"].o, c["info"].n
    assert c["out_lens"].tolist() == [ref_out_len(o, n, L) for L in c["lens"]]
    oo = np.concatenate([[0], np.cumsum(c["out_lens"])])
    worst = 0.0
    for b, (x, want) in enumerate(zip(c["clips"], c["want"])):
        got = c["out"][oo[b]:oo[b + 1]].astype(np.float64)
        err, bar = np.abs(got - want), _bound(x, orig, new)
        worst = max(worst, float((err / np.maximum(bar, 1e-300)).max()))
        assert (err <= bar).all(), (name, c["lens"][b], float(err.max()), float(bar.max()))
    print(f"{name}: worst error / bound = {worst:.3f}")
    assert 0.0 < worst <= 1.0


@pytest.mark.parametrize("name", sorted(RATIOS))
def test_dense_batch_with_a_wide_leading_dimension(ss, sslib, parity_case, name):
    """ld > n_samples and ld_out > out_len: rows of a wider buffer, what lies past a row's end is neither read into the result nor
    written.  Every row equals the packed call's clip of the same samples bit for bit."""
    import torch

    c = parity_case(name)
    orig, new, o, n = c["orig"], c["new"], c["info"].o, c["info"].n
    b = len(c["lens"]) - 2  # the clip of tile + 1 samples
    L, m = c["lens"][b], int(c["out_lens"][b])
    wide = torch.full((3, L + 5), float("nan"), device="cuda")
    rng = np.random.default_rng(5)
    rows = [c["clips"][b], _noise(rng, L), _noise(rng, L)]
    for r, x in enumerate(rows):
        wide[r, :L] = torch.from_numpy(x)
    got = ss.resample(wide[:, :L], orig, new)  # a view: stride(0) = L + 5
    assert got.shape == (3, m)
    oo = np.concatenate([[0], np.cumsum(c["out_lens"])])
    assert np.array_equal(_bits(got[0]), _bits(c["out"][oo[b]:oo[b + 1]]))
    for r, x in enumerate(rows):
        assert (np.abs(got[r].cpu().numpy().astype(np.float64) - ref_resample(x, orig, new)) <= _bound(x, orig, new)).all()
    assert sslib.ss_last_kernel_name() == b"ss_resample_kernel<dense,f32>"
    # ld_out > out_len through the C ABI: the tail of every out row keeps its canary
    rs = ss._get_resampler(orig, new)
    out = torch.full((3, m + 7), float(CANARY), device="cuda")
    assert sslib.ss_resample_device(rs.handle, wide.data_ptr(), 3, L, L + 5, out.data_ptr(), m + 7, None) == 0
    torch.cuda.synchronize()
    assert np.array_equal(_bits(out[:, :m]), _bits(got)) and (out[:, m:] == float(CANARY)).all()
    one = ss.resample(torch.from_numpy(rows[1]).cuda(), orig, new)
    assert one.shape == (m,) and np.array_equal(_bits(one), _bits(got[1]))


@pytest.mark.parametrize("name", ["3/1", "441/160", "1/2"])
def test_bit_exact_invariants(ss, sslib, name):
    import torch

    orig, new = RATIOS[name]
    info = _info(ss, orig, new)
    o, n = info.o, info.n
    tile_in = info.tile_outputs * o // n
    rng = np.random.default_rng(17)
    lens = [tile_in + 3, 1, 0, 5 * o + 1, 2 * tile_in + o - 1, o]
    clips = [_noise(rng, L) for L in lens]
    packed = torch.from_numpy(np.concatenate(clips)).cuda()
    out, out_lens = ss.resample_packed(packed, lens, orig, new)
    assert sslib.ss_last_kernel_name() == b"ss_resample_kernel<packed,f32>"
    oo = np.concatenate([[0], np.cumsum(out_lens)])
    assert out_lens.tolist() == [ref_out_len(o, n, L) for L in lens] and out_lens[2] == 0 and out_lens[1] == ref_out_len(o, n, 1) >= 1
    # packed clip b == the dense call on that clip alone
    alone = [ss.resample(torch.from_numpy(c).cuda(), orig, new) for c in clips]
    for b in range(len(lens)):
        assert np.array_equal(_bits(out[oo[b]:oo[b + 1]]), _bits(alone[b])), (name, b)
    # the same clips at other places, every neighbour NaN or Inf: the same bits
    poison = [np.full(7, np.nan, np.float32), np.full(o + 2, np.inf, np.float32), np.full(3, -np.inf, np.float32)]
    order = [4, 0, 3, 1, 5, 2]
    seq, seq_lens = [poison[0]], [7]
    for k, b in enumerate(order):
        seq += [clips[b], poison[k % 3]]
        seq_lens += [lens[b], len(poison[k % 3])]
    out2, lens2 = ss.resample_packed(torch.from_numpy(np.concatenate(seq)).cuda(), seq_lens, orig, new)
    oo2 = np.concatenate([[0], np.cumsum(lens2)])
    for k, b in enumerate(order):
        got = out2[oo2[1 + 2 * k]:oo2[2 + 2 * k]]
        assert np.array_equal(_bits(got), _bits(alone[b])), (name, b)
        assert torch.isfinite(got).all()
    # host forms == device forms
    host, host_lens = ss.resample_packed(np.concatenate(clips), lens, orig, new)
    assert isinstance(host, np.ndarray) and np.array_equal(host_lens, out_lens) and np.array_equal(_bits(host), _bits(out))
    assert np.array_equal(_bits(ss.resample(clips[0], orig, new)), _bits(alone[0]))
    batch = np.stack([clips[0], clips[0][::-1].copy()])
    assert np.array_equal(_bits(ss.resample(batch, orig, new)), _bits(ss.resample(torch.from_numpy(batch).cuda(), orig, new)))
    lst = ss.resample_list([torch.from_numpy(c).cuda() for c in clips], orig, new)
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(lst, alone))


@pytest.mark.parametrize("name", ["3/1", "441/160"])
@pytest.mark.parametrize("scale", [2.0 ** -15, 1.0])
def test_pcm_forms_equal_the_float_forms_bit_for_bit(ss, sslib, name, scale):
    import torch

    orig, new = RATIOS[name]
    info = _info(ss, orig, new)
    o, n = info.o, info.n
    tile_in = info.tile_outputs * o // n
    rng = np.random.default_rng(23)
    lens = [tile_in + 1, 1, 0, 3 * o + 2, tile_in - 1]
    total = sum(lens)
    buf = torch.from_numpy(rng.integers(-32768, 32768, total + 1, dtype=np.int16)).cuda()
    pcm = buf[1:]  # an odd 2-byte-aligned address
    assert pcm.data_ptr() % 4 == 2
    xf = pcm.float() * scale
    want, want_lens = ss.resample_packed(xf, lens, orig, new)
    got, got_lens = ss.resample_packed(pcm, lens, orig, new, pcm_scale=scale)
    assert sslib.ss_last_kernel_name() == b"ss_resample_kernel<packed,i16>"
    assert np.array_equal(got_lens, want_lens) and np.array_equal(_bits(got), _bits(want))
    L = lens[0]
    dense = ss.resample(pcm[:L], orig, new, pcm_scale=scale)
    assert sslib.ss_last_kernel_name() == b"ss_resample_kernel<dense,i16>"
    assert np.array_equal(_bits(dense), _bits(want[:want_lens[0]]))
    two = torch.stack([pcm[:L], pcm[1:L + 1]])
    assert np.array_equal(_bits(ss.resample(two, orig, new, pcm_scale=scale)), _bits(ss.resample(two.float() * scale, orig, new)))
    # host forms
    host, _ = ss.resample_packed(pcm.cpu().numpy(), lens, orig, new, pcm_scale=scale)
    assert np.array_equal(_bits(host), _bits(want))
    assert np.array_equal(_bits(ss.resample(pcm[:L].cpu().numpy(), orig, new, pcm_scale=scale)), _bits(dense))


def test_small_tiles_of_a_steep_decimation(ss):
    """64 / 1 with lowpass_filter_width = 1: 130 taps and a tile of few periods -- the shape in which a tile holds fewer outputs than
    the workgroup has lanes."""
    import torch

    orig, new, lpw = 64000, 1000, 1
    rs = ss._get_resampler(orig, new, lpw, 0.99)
    assert rs.info.o == 64 and rs.info.n == 1 and rs.info.taps > 100 and rs.info.tile_outputs < 256
    rng = np.random.default_rng(31)
    J = rs.info.tile_outputs
    lens = [64 * J + 1, 64 * 3 * J + 5, 63]
    clips = [_noise(rng, L) for L in lens]
    out, out_lens = ss.resample_packed(torch.from_numpy(np.concatenate(clips)).cuda(), lens, orig, new, lowpass_filter_width=lpw)
    oo = np.concatenate([[0], np.cumsum(out_lens)])
    o, n, width, h, _ = ref_filter(orig, new, lpw)
    s = ref_sizes(orig, new, lpw)
    for b, x in enumerate(clips):
        want = ref_resample(x, orig, new, lpw)
        bar = (s["count"][0] + 3) * 2.0 ** -24 * np.abs(h[0]).sum() * np.abs(x).max()
        assert np.abs(out[oo[b]:oo[b + 1]].cpu().numpy() - want).max() <= bar


# ---- containment ----
def test_bad_clip_tables_are_contained(ss, sslib):
    """A reversed clip, a clip whose output span has the wrong length, a clip past total_in and one past total_out, given to the
    device form as data: their spans and every unowned output keep the canary, the valid clips of the same block are unaffected."""
    import torch

    orig, new = RATIOS["441/160"]
    rs = ss._get_resampler(orig, new)
    o, n = rs.info.o, rs.info.n
    rng = np.random.default_rng(41)
    total_in = 30000
    x = torch.from_numpy(_noise(rng, total_in)).cuda()
    A, B, Cc = 7000, 16001, 21000
    ol = lambda L: ref_out_len(o, n, L)  # noqa: E731
    #        clip 0 valid   1 reversed     2 valid            3 wrong span      4 past total_in     5 past total_out
    so = [0, A,             A - 10,        B,                 Cc,               total_in + 7,       total_in + 7 + 441]
    spans = [ol(A),         5,             ol(B - A + 10),    ol(Cc - B) - 1,   ol(total_in + 7 - Cc), 160]
    oo = np.concatenate([[0], np.cumsum(spans)]).astype(np.int64)
    so = np.asarray(so, np.int64)
    total_out = int(oo[5]) + 100  # clip 5's span ends past it
    out = torch.full((int(oo[-1]) + 64,), float(CANARY), device="cuda")
    d_so, d_oo = torch.from_numpy(so).cuda(), torch.from_numpy(oo).cuda()
    assert sslib.ss_resample_packed_device(rs.handle, x.data_ptr(), 6, d_so.data_ptr(), d_oo.data_ptr(), total_in, total_out, out.data_ptr(),
                                           None) == 0
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    for b, (lo, hi) in ((0, (0, A)), (2, (A - 10, B))):
        alone = ss.resample(x[lo:hi], orig, new)
        assert np.array_equal(_bits(got[oo[b]:oo[b + 1]]), _bits(alone)), b
    for b in (1, 3, 4, 5):
        assert (got[oo[b]:oo[b + 1]] == CANARY).all(), b
    assert (got[oo[-1]:] == CANARY).all()
    # tables of rubbish: negative and huge offsets
    junk = torch.tensor([-5, 3, 2 ** 62, -2 ** 62, 10, 10, 12], dtype=torch.int64, device="cuda")
    out.fill_(float(CANARY))
    assert sslib.ss_resample_packed_device(rs.handle, x.data_ptr(), 6, junk.data_ptr(), junk.data_ptr(), total_in, total_out, out.data_ptr(),
                                           None) == 0
    torch.cuda.synchronize()
    assert (out == float(CANARY)).all()


def test_bad_pool_entries_are_contained(ss, sslib):
    """A slot outside the pool, an entry that is not whole periods and a NaN count word, as data: the bad entries write nothing and
    leave every pool row alone; the NaN count word reads as 0 (a fresh stream's warm-up)."""
    import torch

    orig, new = RATIOS["441/160"]
    rs = ss._get_resampler(orig, new)
    o, n, D = rs.info.o, rs.info.n, rs.info.latency_periods
    H = D * o + rs.info.lookback
    rng = np.random.default_rng(43)
    P = 4
    x = torch.from_numpy(_noise(rng, 8 * o + 1)).cuda()
    so = np.array([0, 3 * o, 5 * o, 7 * o, 8 * o + 1], np.int64)      # entry 3 brings o + 1 samples
    slots = np.array([2, 99, -1, 1], np.int32)                        # entries 1 and 2 name no pool row
    pool = torch.from_numpy(_noise(rng, P * (H + 1)).reshape(P, H + 1)).cuda()
    pool[:, H] = 0
    pool[2, H] = float("nan")
    before = pool.clone()
    n_out = 8 * n
    out = torch.full((n_out + 2 * n,), float(CANARY), device="cuda")
    d_so, d_sl = torch.from_numpy(so).cuda(), torch.from_numpy(slots).cuda()
    assert sslib.ss_resample_stream_packed_device(rs.handle, x.data_ptr(), 4, d_so.data_ptr(), 8 * o + 1, d_sl.data_ptr(), P, pool.data_ptr(),
                                                  out.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert sslib.ss_last_kernel_name() == b"ss_resample_stream_kernel<f32>"
    got = out.cpu().numpy()
    assert (got[3 * n:] == CANARY).all()                              # entries 1, 2, 3 and everything behind
    e0 = got[:3 * n]
    assert (_bits(e0[:D * n]) == 0).all() and np.isfinite(e0).all() and e0[D * n:].any()   # count NaN -> 0: D periods of +0.0 warm-up
    after = pool.cpu().numpy()
    assert np.array_equal(_bits(after[[0, 1, 3]]), _bits(before.cpu().numpy()[[0, 1, 3]]))
    assert after[2, H] == D
    assert H <= 3 * o and np.array_equal(_bits(after[2, :H]), _bits(x[3 * o - H:3 * o]))   # the row: the stream's last H samples
    # the flush: a bad slot is skipped, the good one is served and zeroed
    fl = torch.full((2, D * n), float(CANARY), device="cuda")
    d_fs = torch.tensor([7, 2], dtype=torch.int32, device="cuda")
    assert sslib.ss_resample_stream_flush_device(rs.handle, 2, d_fs.data_ptr(), P, pool.data_ptr(), fl.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert sslib.ss_last_kernel_name() == b"ss_resample_stream_kernel<flush>"
    assert (fl[0] == float(CANARY)).all() and torch.isfinite(fl[1]).all() and not pool[2].any()
    assert np.array_equal(_bits(pool[[0, 1, 3]]), _bits(before[[0, 1, 3]]))


# ---- the pool invariant ----
@pytest.mark.parametrize("name", ["3/1", "441/160"])
def test_pool_invariant_any_cut_plus_flush_equals_the_packed_call(ss, sslib, name):
    import torch

    orig, new = RATIOS[name]
    info = _info(ss, orig, new)
    o, n, D = info.o, info.n, info.latency_periods
    rng = np.random.default_rng(51)
    S, POOL, scale = 5, 8, 2.0 ** -15
    periods = rng.integers(12, 26, S)
    pcm = [rng.integers(-32768, 32768, int(p) * o, dtype=np.int16) for p in periods]     # every stream exists as PCM and as floats
    flt = [c.astype(np.float32) * np.float32(scale) for c in pcm]
    slot_of = rng.permutation(POOL)[:S]
    pool = ss.ResampleStreamPool(POOL, orig, new)
    assert (pool.period_in, pool.period_out, pool.lag) == (o, n, D * n)
    fed = np.zeros(S, np.int64)
    got = [[] for _ in range(S)]
    call = 0
    while (fed < periods).any():
        order = rng.permutation(S)                                                         # changing slot order
        take = np.minimum(rng.integers(0, 5, S), (periods - fed)[order])                   # 0 - 4 periods, empty entries included
        if call == 1:
            take[0] = 0
        use_pcm = call % 2 == 1                                                            # float and PCM calls alternate
        src = pcm if use_pcm else flt
        chunks = [src[s][fed[s] * o:(fed[s] + t) * o] for s, t in zip(order, take)]
        so = np.concatenate([[0], np.cumsum([len(c) for c in chunks])]).astype(np.int64)
        block = torch.from_numpy(np.concatenate(chunks)).cuda() if so[-1] else torch.zeros(0, dtype=torch.int16 if use_pcm else torch.float32,
                                                                                            device="cuda")
        state_before = None if pool.state is None else pool.state.clone()
        out = pool.push(block, so, slot_of[order], pcm_scale=scale if use_pcm else None)
        if so[-1]:
            assert sslib.ss_last_kernel_name() == (b"ss_resample_stream_kernel<i16>" if use_pcm else b"ss_resample_stream_kernel<f32>")
        assert out.shape == (int(so[-1]) // o * n,)
        for k, (s, t) in enumerate(zip(order, take)):
            got[s].append(out[so[k] // o * n:so[k + 1] // o * n].cpu().numpy())
            if t == 0 and state_before is not None:                                        # an empty entry leaves its pool row bit for bit
                assert np.array_equal(_bits(pool.state[slot_of[s]]), _bits(state_before[slot_of[s]]))
        fed[order] += take
        call += 1
    assert np.array_equal(pool.periods_seen[slot_of], periods)
    tail = pool.flush(slot_of)
    assert tail.shape == (S, D * n) and not pool.state[slot_of].any() and not pool.periods_seen.any()
    whole, whole_lens = ss.resample_packed(torch.from_numpy(np.concatenate(flt)).cuda(), [len(c) for c in flt], orig, new)
    oo = np.concatenate([[0], np.cumsum(whole_lens)])
    assert whole_lens.tolist() == (periods * n).tolist()
    for s in range(S):
        stream = np.concatenate(got[s] + [tail[s].cpu().numpy()])
        assert (_bits(stream[:D * n]) == 0).all()                                          # the warm-up: exactly +0.0
        assert np.array_equal(_bits(stream[D * n:]), _bits(whole[oo[s]:oo[s + 1]])), (name, s)
    # the numpy (host-pointer) pool gives the same bits
    hpool = ss.ResampleStreamPool(POOL, orig, new)
    a = hpool.push(flt[0][:3 * o], [0, 3 * o], [4])
    b = hpool.push(pcm[0][3 * o:], [0, len(pcm[0]) - 3 * o], [4], pcm_scale=scale)
    c = hpool.flush([4])
    assert isinstance(a, np.ndarray) and not hpool.state.any()
    assert np.array_equal(_bits(np.concatenate([a, b, c[0]])[D * n:]), _bits(whole[oo[0]:oo[1]]))


# ---- graphs ----
def _hip_runtime():
    """The HIP runtime this process has loaded (torch's), for the stream-capture calls the graph-shape check needs."""
    with open("/proc/self/maps") as f:
        paths = {line.split()[-1] for line in f if "libamdhip64" in line}
    assert paths, "no HIP runtime loaded"
    return C.CDLL(sorted(paths)[0])


def test_graph_of_packed_resample_then_mfcc_on_its_out_offsets(ss, sslib, oracle):
    """48 kHz clips -> 16 kHz -> MFCC in one captured graph: out_offsets of the resampler are the sample_offsets of
    ss_mfcc_packed_device.  Replayed on new audio the pair equals the eager pair bit for bit and the oracle's MFCC of the
    f64-resampled clips at the sweep's 1e-4 block bar."""
    import torch

    from speechsauce_amd import _lib

    orig, new = 48000, 16000
    rs = ss._get_resampler(orig, new)
    cfg = ss.SpeechConfig(_lib.make_params())
    lens = np.array([48000, 23331, 4803, 30000], np.int64)
    so = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    oo = np.empty_like(so)
    assert sslib.ss_resample_packed_offsets(orig, new, 4, so.ctypes.data, oo.ctypes.data) == 0
    fo = ss._frame_offsets(cfg, oo)
    total_in, total_out, rows = int(so[-1]), int(oo[-1]), int(fo[-1])
    d_so, d_oo, d_fo = (torch.from_numpy(t).cuda() for t in (so, oo, fo))
    x = torch.zeros(total_in, device="cuda")
    mid = torch.zeros(total_out, device="cuda")
    feat = torch.zeros((rows, 13), device="cuda")

    def pair(stream, mid, feat):
        st = C.c_void_p(stream)
        assert sslib.ss_resample_packed_device(rs.handle, x.data_ptr(), 4, d_so.data_ptr(), d_oo.data_ptr(), total_in, total_out, mid.data_ptr(),
                                               st) == 0, sslib.ss_last_error_string()
        assert sslib.ss_mfcc_packed_device(cfg.handle, mid.data_ptr(), 4, d_oo.data_ptr(), d_fo.data_ptr(), rows, feat.data_ptr(), st) == 0

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # the warm call outside the capture uploads the resampler's table
        pair(side.cuda_stream, mid, feat)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        pair(torch.cuda.current_stream().cuda_stream, mid, feat)
    p = oracle.make_params()
    for seed in (61, 62):
        xs = _noise(np.random.default_rng(seed), total_in)
        x.copy_(torch.from_numpy(xs))
        mid.zero_()
        feat.zero_()
        g.replay()
        torch.cuda.synchronize()
        mid_e, feat_e = torch.empty_like(mid), torch.empty_like(feat)
        pair(torch.cuda.current_stream().cuda_stream, mid_e, feat_e)
        torch.cuda.synchronize()
        assert np.array_equal(_bits(mid), _bits(mid_e)) and np.array_equal(_bits(feat), _bits(feat_e))
        for b in range(4):
            want = oracle.mfcc(p, ref_resample(xs[so[b]:so[b + 1]], orig, new).astype(np.float32))
            assert _rel(feat[fo[b]:fo[b + 1]].cpu().numpy(), want) <= 1e-4, (seed, b)
    cfg.device_status()


def test_graph_of_the_pool_call_is_one_kernel_node_over_changing_tables(ss, sslib):
    import torch

    orig, new = RATIOS["441/160"]
    rs = ss._get_resampler(orig, new)
    o, n, D = rs.info.o, rs.info.n, rs.info.latency_periods
    H = D * o + rs.info.lookback
    N, P, CAP = 5, 8, 16  # entries, pool rows, periods the block can hold
    x = torch.zeros(CAP * o, device="cuda")
    out = torch.zeros(CAP * n, device="cuda")
    d_so = torch.zeros(N + 1, dtype=torch.int64, device="cuda")
    d_sl = torch.arange(N, dtype=torch.int32, device="cuda")
    pool_g, pool_e = torch.zeros((P, H + 1), device="cuda"), torch.zeros((P, H + 1), device="cuda")

    def call(pool, out, stream, n_active=N):
        return sslib.ss_resample_stream_packed_device(rs.handle, x.data_ptr(), n_active, d_so.data_ptr(), CAP * o, d_sl.data_ptr(), P,
                                                      pool.data_ptr(), out.data_ptr(), C.c_void_p(stream))

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up outside the capture (zero tables: N entries without samples)
        assert call(pool_g.clone(), out, side.cuda_stream) == 0
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    hip = _hip_runtime()
    hip.hipGraphGetNodes.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_size_t)]
    hip.hipGraphNodeGetType.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
    for n_active in (N, 3):  # ONE kernel node, for 3 entries as for 5
        raw, graph = torch.cuda.Stream(), C.c_void_p()
        assert hip.hipStreamBeginCapture(C.c_void_p(raw.cuda_stream), 2) == 0  # hipStreamCaptureModeRelaxed
        try:
            rc = call(pool_g, out, raw.cuda_stream, n_active)
        finally:
            assert hip.hipStreamEndCapture(C.c_void_p(raw.cuda_stream), C.byref(graph)) == 0
        assert rc == 0
        n_nodes = C.c_size_t()
        assert hip.hipGraphGetNodes(graph, None, C.byref(n_nodes)) == 0 and n_nodes.value == 1
        nodes, kind = (C.c_void_p * 1)(), C.c_int(-1)
        assert hip.hipGraphGetNodes(graph, nodes, C.byref(n_nodes)) == 0
        assert hip.hipGraphNodeGetType(nodes[0], C.byref(kind)) == 0 and kind.value == 0  # hipGraphNodeTypeKernel
        assert hip.hipGraphDestroy(graph) == 0
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        assert call(pool_g, out, torch.cuda.current_stream().cuda_stream) == 0
    rng = np.random.default_rng(71)
    for k in range(3):  # ticks with changed tables
        take = rng.integers(0, 4, N)
        take[rng.integers(0, N)] = 0
        so = np.concatenate([[0], np.cumsum(take * o)]).astype(np.int64)
        slots = rng.permutation(P)[:N].astype(np.int32)
        x.zero_()
        x[:int(so[-1])] = torch.from_numpy(_noise(rng, int(so[-1])))
        d_so.copy_(torch.from_numpy(so))
        d_sl.copy_(torch.from_numpy(slots))
        out.fill_(float(CANARY))
        g.replay()
        torch.cuda.synchronize()
        out_e = torch.full_like(out, float(CANARY))
        assert call(pool_e, out_e, torch.cuda.current_stream().cuda_stream) == 0
        torch.cuda.synchronize()
        assert np.array_equal(_bits(out), _bits(out_e)) and np.array_equal(_bits(pool_g), _bits(pool_e))
        assert (out[int(so[-1]) // o * n:] == float(CANARY)).all()
    assert pool_g[:, H].sum() > 0
