"""The fused splice + affine transform on the device: ss_affine_splice_packed* and the Python front's Affine, splice_affine_packed,
splice_affine and transform_feats_packed.

The contract is one serial f32 fmaf chain per output element, so the device rows are compared with the numpy chain of
tests/affine_model.py on uint32 views; the operand maps are pinned separately on exact integer data, where no tolerance can hide a
swapped index.  Outputs sit between guard rows of a sentinel bit pattern.

Measured on an MI355X, 2026-10-21: every shape bit for bit the model chain; the largest |device - f64| as a fraction of the bar (K4 +
1) * 2^-24 * (|bias| + sum |M| |s|) was 0.19 (K = 1), 0.15 (K = 13), 0.044 (K = 69), 0.035 (K = 91), 0.028 (K = 200), 0.0076 (K = 440),
0.0053 (K = 560) and 0.0006 (K = 4096); test_within_the_bar_of_the_f64_restatement prints the figures before it asserts.
"""
import ctypes as C

import numpy as np
import pytest

from affine_model import LENS, SENTINEL, SHAPE_4096, SHAPES, affine_f64, affine_ref, block, matrix, rows, u32, want
from splice_model import splice_ref

pytestmark = pytest.mark.gpu

ALL = SHAPES + (SHAPE_4096,)
GUARD = 3
SENT_I32 = int(SENTINEL) - (1 << 32)


def _fill(torch, shape):
    """a device block of the sentinel"""
    return torch.full(shape, SENT_I32, dtype=torch.int32, device="cuda").view(torch.float32)


def _bits(t):
    import torch

    return t.contiguous().view(torch.int32)


def _is_sentinel(t):
    return bool((_bits(t) == SENT_I32).all())


def _stream():
    import torch

    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class Transform:
    """an ss_affine handle for the length of a test"""

    def __init__(self, lib, M, bias=None):
        self.lib, self.h, self.out_dim = lib, C.c_void_p(), M.shape[0]
        M = np.ascontiguousarray(M, np.float32)
        b = None if bias is None else np.ascontiguousarray(bias, np.float32)
        assert lib.ss_affine_create(M.ctypes.data, M.shape[0], M.shape[1], M.shape[1], None if b is None else b.ctypes.data, C.byref(self.h)) == 0

    def __del__(self):
        self.lib.ss_affine_destroy(self.h)


def _offsets(lens, stride):
    ro = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    oo = np.concatenate([[0], np.cumsum([-(-int(n) // stride) for n in lens])]).astype(np.int64)
    return ro, oo


def _device(torch, lib, t, clips, shape, ro=None, oo=None, total_out=None):
    """ss_affine_splice_packed_device on host clips [T_b, cols] (tables: the gap-free ones unless given); the output sits between guard
    rows and starts as the sentinel.  -> (out [total_out, out_dim] on the host, oo)"""
    cols, left, right, stride, out_dim = shape
    lens = [c.shape[0] for c in clips]
    ro0, oo0 = _offsets(lens, stride)
    ro, oo = ro0 if ro is None else np.asarray(ro, np.int64), oo0 if oo is None else np.asarray(oo, np.int64)
    R, RO = int(ro0[-1]), int(oo0[-1]) if total_out is None else total_out
    x = torch.from_numpy(np.concatenate(list(clips)).reshape(R, cols)).cuda()
    out = _fill(torch, (RO + 2 * GUARD, out_dim))
    d_ro, d_oo = torch.from_numpy(ro).cuda(), torch.from_numpy(oo).cuda()
    rc = lib.ss_affine_splice_packed_device(t.h, x.data_ptr(), len(ro) - 1, d_ro.data_ptr(), R, d_oo.data_ptr(), RO, cols, left, right, stride,
                                            out[GUARD:].data_ptr(), _stream())
    assert rc == 0, lib.ss_last_error_string()
    torch.cuda.synchronize()
    assert _is_sentinel(out[:GUARD]) and _is_sentinel(out[GUARD + RO:])
    return out[GUARD:GUARD + RO].cpu().numpy(), oo


def _same_bits(got, ref):
    assert got.shape == ref.shape, (got.shape, ref.shape)
    bad = np.argwhere(u32(got) != u32(ref))
    assert bad.size == 0, (len(bad), bad[:6].tolist(), got[tuple(bad[0])], ref[tuple(bad[0])])


def _int_rows(cols, T, seed):
    """integer-valued rows, none zero, every value of a clip distinct where the clip is small enough: |v| < 2^20"""
    rng = np.random.default_rng(seed)
    v = (np.arange(T * cols).reshape(T, cols) + 1 + 1000 * seed).astype(np.float32)
    return v * np.where(rng.random((T, cols)) < 0.5, -1, 1).astype(np.float32)


@pytest.mark.parametrize("shape", ALL)
def test_operand_maps_on_exact_data(sslib, shape):
    """A selection matrix that is not symmetric -- output i is input (7 i + 3) mod K -- makes every output a bit copy of the spliced
    element it names: a swap of row and column, of the matrix's two indices, or a wrong k order shows without any tolerance.  Then
    a small-integer matrix (|M| <= 3, M[i][k] depends on i and k differently) on small integers, whose chain is exact."""
    import torch

    cols, left, right, stride, out_dim = shape
    K = (left + 1 + right) * cols
    clips = [_int_rows(cols, T, i) for i, T in enumerate(LENS)]
    spliced = np.concatenate([splice_ref(c, left, right, stride) for c in clips])
    sel = (7 * np.arange(out_dim) + 3) % K
    M = np.zeros((out_dim, K), np.float32)
    M[np.arange(out_dim), sel] = 1.0
    got, _ = _device(torch, sslib, Transform(sslib, M), clips, shape)
    _same_bits(got, spliced[:, sel])
    i, k = np.arange(out_dim)[:, None], np.arange(K)[None, :]
    M = ((3 * i + 5 * k + (i * k) % 3) % 7 - 3).astype(np.float32)
    small = [np.sign(c) * (np.abs(c) % 9) for c in clips]  # |s| <= 8, zeros among them
    bias = (np.arange(out_dim) % 5 - 2).astype(np.float32)
    exact = np.concatenate([splice_ref(c, left, right, stride) for c in small]).astype(np.int64) @ M.astype(np.int64).T + bias.astype(np.int64)
    assert np.abs(exact).max() < 1 << 24
    got, _ = _device(torch, sslib, Transform(sslib, M, bias), small, shape)
    assert np.array_equal(got.astype(np.int64), exact) and not np.signbit(got[got == 0]).any()


@pytest.mark.parametrize("with_bias", (False, True))
@pytest.mark.parametrize("shape", ALL)
def test_bit_for_bit_against_the_model_chain(sslib, shape, with_bias):
    """Finite normal inputs with -0.0 and denormals among rows, weights and bias: every output element is the chain of the header --
    K4 fmaf steps in ascending k, pad steps included -- bit for bit."""
    import torch

    cols, left, right, stride, out_dim = shape
    M, bias = matrix(out_dim, (left + 1 + right) * cols)
    clips, _ = block(cols)
    got, _ = _device(torch, sslib, Transform(sslib, M, bias if with_bias else None), clips, shape)
    _same_bits(got, want(shape, with_bias))


def test_a_block_off_the_16_byte_grid_gives_the_same_bits(sslib):
    """cols % 4 == 0 takes 16-byte loads of the rows only where vec is 16-byte aligned; one float off that grid the call runs on
    single loads, and gives the same rows."""
    import torch

    shape = cols, left, right, stride, out_dim = (40, 5, 5, 1, 40)
    M, bias = matrix(out_dim, 440)
    t = Transform(sslib, M, bias)
    clips, ro = block(cols)
    R = int(ro[-1])
    buf = torch.zeros(R * cols + 4, device="cuda")
    buf[1:1 + R * cols] = torch.from_numpy(np.concatenate(clips).reshape(-1)).cuda()
    out = _fill(torch, (R + 2 * GUARD, out_dim))
    d_ro = torch.from_numpy(ro).cuda()
    assert buf.data_ptr() % 16 == 0
    rc = sslib.ss_affine_splice_packed_device(t.h, buf.data_ptr() + 4, len(ro) - 1, d_ro.data_ptr(), R, d_ro.data_ptr(), R, cols, left, right, stride,
                                              out[GUARD:].data_ptr(), _stream())
    assert rc == 0, sslib.ss_last_error_string()
    torch.cuda.synchronize()
    assert _is_sentinel(out[:GUARD]) and _is_sentinel(out[GUARD + R:])
    _same_bits(out[GUARD:GUARD + R].cpu().numpy(), want(shape, True))


def test_a_negative_zero_survives_only_a_chain_without_pad_steps(sslib):
    """bias -0.0 under products that are all -0.0: K = 4 (no pad step) gives -0.0, K = 1 (three pad steps of +0 * +0) gives +0.0."""
    import torch

    for cols, bits in ((4, 0x80000000), (1, 0)):
        M, x = np.full((3, cols), -0.0, np.float32), [np.ones((5, cols), np.float32)]
        got, _ = _device(torch, sslib, Transform(sslib, M, np.full(3, -0.0, np.float32)), x, (cols, 0, 0, 1, 3))
        assert (u32(got) == bits).all(), (cols, u32(got))


@pytest.mark.parametrize("shape", ALL)
def test_within_the_bar_of_the_f64_restatement(sslib, shape):
    """Every element within (K4 + 1) * 2^-24 * (|bias_i| + sum_k |M_ik| |s_k|) of the product in f64 (inputs without denormals: the
    bar is one of relative roundings)."""
    import torch

    cols, left, right, stride, out_dim = shape
    M, bias = matrix(out_dim, (left + 1 + right) * cols, denormals=False)
    clips, _ = block(cols, denormals=False)
    got, oo = _device(torch, sslib, Transform(sslib, M, bias), clips, shape)
    worst = 0.0
    for b, c in enumerate(clips):
        if len(c):
            ref, bar = affine_f64(c, M, bias, left, right, stride)
            diff = np.abs(got[oo[b]:oo[b + 1]] - ref)
            assert (diff <= bar).all()  # (a bar of 0 -- a row of zeros under a zero bias -- wants the exact 0)
            worst = max(worst, float(np.divide(diff, bar, out=np.zeros_like(diff), where=bar > 0).max()))
    print(f"shape {shape}: largest |device - f64| / bar = {worst:.4f}")
    assert worst <= 1.0


def test_a_clip_does_not_depend_on_its_place_and_a_permutation_permutes(sslib):
    """One clip alone, and the same clip at other places of a block, behind other neighbours, at other phases of the 16-row tiles;
    then the block's clips in another order."""
    import torch

    shape = (13, 3, 3, 1, 40)
    M, bias = matrix(40, 91)
    t = Transform(sslib, M, bias)
    mine = rows(13, 77, seed=90)
    alone, _ = _device(torch, sslib, t, [mine], shape)
    _same_bits(alone, affine_ref(mine, M, bias, 3, 3, 1))
    a, b, c = rows(13, 7, seed=91), rows(13, 300, seed=92), rows(13, 1, seed=93)
    for clips, i in (([mine, a, b], 0), ([a, b, mine], 2), ([a, mine, b], 1), ([b, c, mine[:0], mine, a], 3), ([c, c, mine], 2)):
        got, oo = _device(torch, sslib, t, clips, shape)
        _same_bits(got[oo[i]:oo[i + 1]], alone)
    clips, _ = block(13)
    base, oo = _device(torch, sslib, t, clips, shape)
    perm = np.random.default_rng(3).permutation(len(clips))
    got, poo = _device(torch, sslib, t, [clips[p] for p in perm], shape)
    for j, p in enumerate(perm):
        _same_bits(got[poo[j]:poo[j + 1]], base[oo[p]:oo[p + 1]])


@pytest.mark.parametrize("shape", ((13, 3, 3, 1, 40), (80, 3, 3, 6, 32), (13, 0, 0, 1, 17)))
def test_the_host_form_and_the_python_front_equal_the_device_form(sslib, ss, shape):
    import torch

    cols, left, right, stride, out_dim = shape
    M, bias = matrix(out_dim, (left + 1 + right) * cols)
    clips, ro = block(cols)
    dev, oo = _device(torch, sslib, Transform(sslib, M, bias), clips, shape)
    x = np.concatenate(clips)
    t = ss.Affine(M, bias)
    host, hoo = ss.splice_affine_packed(x, ro, t, left, right, stride)
    _same_bits(host, dev)
    assert np.array_equal(hoo, oo)
    got, doo = ss.splice_affine_packed(torch.from_numpy(x).cuda(), ro, t, left, right, stride)
    _same_bits(got.cpu().numpy(), dev)
    assert np.array_equal(doo.cpu().numpy(), oo)
    kaldi = ss.Affine.from_kaldi(np.hstack([M, bias[:, None]]), in_dim=M.shape[1])  # [linear | offset]
    _same_bits(ss.splice_affine_packed(x, ro, kaldi, left, right, stride)[0], dev)
    one = rows(cols, 33, seed=5)
    _same_bits(ss.splice_affine(np.stack([one, one]), t, left, right, stride)[1], affine_ref(one, M, bias, left, right, stride))


def test_no_context_on_the_spliced_block_equals_the_fused_call(sslib, ss):
    """left = right = 0, stride = 1 on what ss_splice_packed_device wrote (plain transform-feats, the call behind a stream pool's
    splice) gives the bits of the fused call."""
    import torch

    for shape in ((13, 3, 3, 1, 40), (40, 0, 4, 3, 256)):
        cols, left, right, stride, out_dim = shape
        K = (left + 1 + right) * cols
        M, bias = matrix(out_dim, K)
        clips, ro = block(cols)
        fused, oo = _device(torch, sslib, Transform(sslib, M, bias), clips, shape)
        spliced, soo = ss.splice_packed(torch.from_numpy(np.concatenate(clips)).cuda(), ro, left, right, stride)
        two = ss.transform_feats_packed(spliced, soo.cpu().numpy(), ss.Affine(M, bias))
        _same_bits(two.cpu().numpy(), fused)


def test_a_side_stream_and_a_graph_replay_over_changed_tables_give_the_eager_bits(sslib):
    """The call is one kernel node with no allocation and no read-back once the handle is warm: captured once, it is replayed over
    other rows and other tables (other clip lengths, the same capacity) and gives what the eager call gives."""
    import torch

    shape = cols, left, right, stride, out_dim = (40, 5, 5, 1, 40)
    M, bias = matrix(out_dim, 440)
    t = Transform(sslib, M, bias)
    CAP, N = 400, 6
    x = torch.zeros((CAP, cols), device="cuda")
    out = _fill(torch, (CAP, out_dim))
    d_ro = torch.zeros(N + 1, dtype=torch.int64, device="cuda")

    def call(stream):
        rc = sslib.ss_affine_splice_packed_device(t.h, x.data_ptr(), N, d_ro.data_ptr(), CAP, d_ro.data_ptr(), CAP, cols, left, right, stride,
                                                  out.data_ptr(), C.c_void_p(stream))
        assert rc == 0, sslib.ss_last_error_string()

    def load(lens, seed):
        clips = [rows(cols, T, seed + i) for i, T in enumerate(lens)]
        x.zero_()
        x[:sum(lens)] = torch.from_numpy(np.concatenate(clips))
        d_ro.copy_(torch.from_numpy(_offsets(lens, 1)[0]))  # stride 1: the row table is the output table
        out.view(torch.int32).fill_(SENT_I32)
        return np.concatenate([affine_ref(c, M, bias, left, right, stride) for c in clips])

    side = torch.cuda.Stream()
    ref = load([30, 0, 100, 17, 1, 50], 20)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # the warm call (it uploads the handle's table), on a side stream
        call(side.cuda_stream)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    _same_bits(out[:len(ref)].cpu().numpy(), ref)
    assert _is_sentinel(out[len(ref):])
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call(torch.cuda.current_stream().cuda_stream)
    for k, lens in enumerate(([400, 0, 0, 0, 0, 0], [1, 2, 3, 4, 5, 6], [64, 64, 64, 64, 64, 64])):
        ref = load(lens, 30 + 10 * k)
        g.replay()
        torch.cuda.synchronize()
        _same_bits(out[:len(ref)].cpu().numpy(), ref)
        assert _is_sentinel(out[len(ref):])


def test_bad_clips_are_skipped_whole_and_a_nan_row_stays_in_its_context(sslib):
    """A reversed row pair, an output pair with one row too many and a clip that ends past total_rows: each is skipped whole -- its rows
    of out keep the sentinel -- and every other clip is exact.  (The output table does not decrease: it is where a row's clip is
    looked up.)  Then a NaN row: exactly the output rows whose context holds it are NaN, in every feature."""
    import torch

    shape = cols, left, right, stride, out_dim = (13, 2, 3, 2, 40)
    M, bias = matrix(out_dim, 6 * cols)
    t = Transform(sslib, M, bias)
    lens = [20, 9, 33, 5, 16, 7]
    clips = [rows(cols, T, seed=50 + i) for i, T in enumerate(lens)]
    ro, oo = _offsets(lens, stride)
    good, _ = _device(torch, sslib, t, clips, shape)
    cases = {"reversed": (1, lambda r, o: r.__setitem__(slice(1, 3), [r[2], r[1]])),  # clip 1 reversed (its neighbours' pairs break with it)
             "one_too_many": (3, None), "past_total_rows": (5, lambda r, o: r.__setitem__(6, r[6] + 1))}
    for name, (b, edit) in cases.items():
        r, o = ro.copy(), oo.copy()
        total_out = int(oo[-1])
        if edit:
            edit(r, o)
        else:  # clip 3 claims one output row more than ceil(T / stride): every later clip moves down a row and stays consistent
            o[b + 1:] += 1
            total_out += 1
        got, _ = _device(torch, sslib, t, clips, shape, ro=r, oo=o, total_out=total_out)
        for c in range(len(lens)):
            served = 0 <= r[c] <= r[c + 1] <= ro[-1] and o[c + 1] - o[c] == -(-(r[c + 1] - r[c]) // stride)
            mine = got[o[c]:o[c + 1]]
            if served and (r[c], r[c + 1]) == (ro[c], ro[c + 1]):
                _same_bits(mine, good[oo[c]:oo[c + 1]])
            else:
                assert not served and (u32(mine) == SENTINEL).all(), (name, c)
        assert not (np.array([0 <= r[c] <= r[c + 1] <= ro[-1] and o[c + 1] - o[c] == -(-(r[c + 1] - r[c]) // stride) for c in range(len(lens))])).all(), name
    # a NaN row in clip 2 (row 10 of 33) and one in the last row of clip 4
    hit = {2: 10, 4: 15}
    dirty = [c.copy() for c in clips]
    for b, row in hit.items():
        dirty[b][row] = np.nan
    got, _ = _device(torch, sslib, t, dirty, shape)
    for b, T in enumerate(lens):
        k = np.arange(-(-T // stride))
        centre = k * stride
        holds = np.zeros(len(k), bool)
        if b in hit:
            ctx = np.clip(centre[:, None] + np.arange(-left, right + 1)[None, :], 0, T - 1)
            holds = (ctx == hit[b]).any(axis=1)
        mask = np.isnan(got[oo[b]:oo[b + 1]])
        assert np.array_equal(mask, np.broadcast_to(holds[:, None], mask.shape)), b
        _same_bits(got[oo[b]:oo[b + 1]][~holds], good[oo[b]:oo[b + 1]][~holds])


def test_more_tiles_than_one_pass_of_the_grid(sslib):
    """About 300 000 rows x 13 columns in few clips: the workgroups stride over the block more than once.  Bit for bit the
    concatenation of calls on consecutive sub-blocks of whole clips, and every row written."""
    import torch

    shape = cols, left, right, stride, out_dim = (13, 3, 3, 1, 40)
    M, bias = matrix(out_dim, 91)
    t = Transform(sslib, M, bias)
    lens = [70001, 3, 99999, 0, 50000, 65537, 14461]
    assert sum(lens) == 300001
    ro, _ = _offsets(lens, 1)
    x = torch.randn((sum(lens), cols), device="cuda", generator=torch.Generator(device="cuda").manual_seed(7))
    d_ro = torch.from_numpy(ro).cuda()

    def call(first, last):
        """clips first .. last - 1 as a block of their own"""
        lo, hi = int(ro[first]), int(ro[last])
        out = _fill(torch, (hi - lo + 2 * GUARD, out_dim))
        table = (d_ro[first:last + 1] - lo).contiguous()
        rc = sslib.ss_affine_splice_packed_device(t.h, x[lo:].data_ptr(), last - first, table.data_ptr(), hi - lo, table.data_ptr(), hi - lo, cols, left,
                                                  right, stride, out[GUARD:].data_ptr(), _stream())
        assert rc == 0, sslib.ss_last_error_string()
        torch.cuda.synchronize()
        assert _is_sentinel(out[:GUARD]) and _is_sentinel(out[GUARD + hi - lo:])
        return out[GUARD:GUARD + hi - lo]

    whole = call(0, len(lens))
    assert not bool((_bits(whole) == SENT_I32).all(dim=1).any())  # every row was written
    parts = torch.cat([call(0, 2), call(2, 3), call(3, 5), call(5, 7)])
    assert torch.equal(_bits(whole), _bits(parts))
    head = whole[:64].cpu().numpy()  # and the block is the model's: its first rows
    _same_bits(head, affine_ref(x[:80].cpu().numpy(), M, bias, left, right, stride)[:64])
