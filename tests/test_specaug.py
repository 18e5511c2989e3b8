"""SpecAugment of packed rows on the device: ss_specaug_plan_packed_device, ss_mask_spans_packed[_device], ss_specaug_packed[_device]
and the Python front's spec_augment_packed, mask_spans_packed and SpecAugment.

Every comparison is on bit patterns against the numpy restatement of the header (tests/specaug_model.py): there is no tolerance
anywhere.  The inputs are salted with NaNs, -0.0, +-inf and denormals (splice_model.clip); out and spans are pre-filled with a
sentinel that no call can produce and sit between guards of it.
"""
import ctypes as C

import numpy as np
import pytest

from specaug_model import SENTINEL, apply_ref, clip, spans_ref, u32
from test_specaug_cpu import GRID, LENS, SEED

pytestmark = pytest.mark.gpu

GUARD = 64        # elements in front of and behind out and spans
SPAN_SENT = -99   # no span entry is below -1
VALUES = (0.0, -0.0, -1.5, float("nan"))
FLAT_ROUND = 64 * 1024 * 4  # elements one round of a clip's 64 workgroups covers in the flat walk (kFlatChunk = 1024 groups of 4 each)


def _signed(v):
    return int(v) - (1 << 32) if int(v) >= 1 << 31 else int(v)


def _stream():
    import torch

    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _table(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


def _block(torch, seed, epoch):
    """the 16-byte device block {seed, epoch}"""
    return torch.from_numpy(np.array([seed, epoch], np.uint64).view(np.int64)).cuda()


def _words(block):
    return [int(v) for v in block.cpu().numpy().view(np.uint64)]


def _bits_of(value):
    return int(np.array([value], np.float32).view(np.uint32)[0])


class Bufs:
    """out [total_rows x cols] and spans [n x n_masks x 2] between guards, everything pre-filled with its sentinel; `phase` = 1 starts
    out one float into its allocation"""

    def __init__(self, torch, total_rows, cols, n, n_masks, phase=0):
        self.shape, self.count, self.n, self.n_masks = (total_rows, cols), total_rows * cols, n, n_masks
        self.raw = torch.full((phase + GUARD + self.count + GUARD,), _signed(SENTINEL), dtype=torch.int32, device="cuda")
        self.out = self.raw[phase + GUARD:phase + GUARD + self.count]
        self.sp_raw = torch.full((GUARD + n * n_masks * 2 + GUARD,), SPAN_SENT, dtype=torch.int32, device="cuda")
        self.spans = self.sp_raw[GUARD:GUARD + n * n_masks * 2]

    def load(self, torch, xh):
        """the in-place call: the rows themselves sit between the guards"""
        self.out.copy_(torch.from_numpy(np.array(u32(xh).reshape(-1).view(np.int32))))
        return self

    def reset(self):
        self.raw.fill_(_signed(SENTINEL))
        self.sp_raw.fill_(SPAN_SENT)

    def result(self):
        """-> (bits [total_rows, cols], spans [n, n_masks, 2]) on the host, after checking that the guards are untouched"""
        import torch

        torch.cuda.synchronize()
        raw = self.raw.cpu().numpy().view(np.uint32)
        at = raw.size - GUARD - self.count
        assert (raw[:at] == SENTINEL).all() and (raw[at + self.count:] == SENTINEL).all(), "guard of out"
        sp = self.sp_raw.cpu().numpy()
        assert (sp[:GUARD] == SPAN_SENT).all() and (sp[sp.size - GUARD:] == SPAN_SENT).all(), "guard of spans"
        return raw[at:at + self.count].reshape(self.shape), sp[GUARD:sp.size - GUARD].reshape(self.n, self.n_masks, 2)


def _device_rows(torch, xh, phase=0):
    """the block on the device, `phase` floats into its allocation; a block without rows still has an address"""
    flat = torch.zeros(max(xh.size, 1) + phase, device="cuda")[phase:]
    flat[:xh.size].copy_(torch.from_numpy(np.array(xh, np.float32).reshape(-1)))
    return flat


def _augment(torch, lib, xh, ro, total_rows, block, base, nt, tw, ratio, nf, fw, value, inplace, phase=0, in_phase=0):
    """one combined call -> (bits, spans) on the host, guards checked"""
    cols, n = xh.shape[1], len(ro) - 1
    b = Bufs(torch, len(xh), cols, n, nt + nf, phase)
    x = b.load(torch, xh).out if inplace else _device_rows(torch, xh, in_phase)
    d_ro = torch.from_numpy(np.asarray(ro, np.int64)).cuda()
    rc = lib.ss_specaug_packed_device(x.data_ptr(), n, d_ro.data_ptr(), total_rows, cols, block.data_ptr(), base, nt, tw, ratio, nf, fw, value, b.out.data_ptr(),
                                      b.spans.data_ptr(), _stream())
    assert rc == 0, lib.ss_last_error_string()
    assert lib.ss_last_kernel_name().decode() == "ss_specaug_apply_kernel<%s>" % ("inplace" if inplace else "copy")
    return b.result()


def _mask(torch, lib, xh, ro, total_rows, spans, nt, nf, value, inplace, phase=0, in_phase=0):
    """one apply launch on a spans table from the host -> bits"""
    cols, n = xh.shape[1], len(ro) - 1
    b = Bufs(torch, len(xh), cols, n, nt + nf, phase)
    x = b.load(torch, xh).out if inplace else _device_rows(torch, xh, in_phase)
    d_ro = torch.from_numpy(np.asarray(ro, np.int64)).cuda()
    d_sp = torch.from_numpy(np.ascontiguousarray(spans, np.int32).reshape(-1)).cuda()
    rc = lib.ss_mask_spans_packed_device(x.data_ptr(), n, d_ro.data_ptr(), total_rows, cols, d_sp.data_ptr(), nt, nf, value, b.out.data_ptr(), _stream())
    assert rc == 0, lib.ss_last_error_string()
    bits, untouched = b.result()
    assert (untouched == SPAN_SENT).all() and np.array_equal(d_sp.cpu().numpy().reshape(np.shape(spans)), spans)  # the table is read only
    return bits


def _want(xh, ro, total_rows, spans, nt, nf, value, inplace):
    """the restatement: in place every uncovered row keeps its bits, out of place it keeps the sentinel"""
    held = None if inplace else np.full(xh.shape, SENTINEL, np.uint32)
    return apply_ref(u32(xh), ro, total_rows, spans, nt, nf, _bits_of(value), out=held)


def test_the_plan_is_the_restatement_over_the_grid(sslib):
    """ss_specaug_plan_packed_device over lengths 0 .. 300, cols 1 / 13 / 80, every mask count, width, ratio, clip_base and epoch of
    the grid the host call walks in tests/test_specaug_cpu.py; the block is left as it was."""
    import torch

    ro = _table(LENS)
    total, n = int(ro[-1]), len(LENS)
    d_ro = torch.from_numpy(ro).cuda()
    blocks = {e: _block(torch, SEED, e) for e in {g[-1] for g in GRID}}
    b = Bufs(torch, 1, 1, n, 32)
    for cols, (nt, nf), width, ratio, base, epoch in GRID:
        b.sp_raw.fill_(SPAN_SENT)
        rc = sslib.ss_specaug_plan_packed_device(blocks[epoch].data_ptr(), base, n, d_ro.data_ptr(), total, cols, nt, width, ratio, nf, width, b.spans.data_ptr(),
                                                 _stream())
        assert rc == 0, sslib.ss_last_error_string()
        _, got = b.result()
        used = n * (nt + nf)
        want = spans_ref((SEED, epoch), base, ro, total, cols, nt, width, ratio, nf, width)
        assert np.array_equal(got.reshape(-1, 2)[:used].reshape(want.shape), want), (cols, nt, nf, width, ratio, base, epoch)
        assert (got.reshape(-1, 2)[used:] == SPAN_SENT).all()
    for e, blk in blocks.items():
        assert _words(blk) == [SEED, e]  # the plan launch does not touch the epoch


@pytest.mark.parametrize("cols", (1, 13, 33, 80))
def test_the_combined_call_is_the_restatement_bit_for_bit(sslib, cols):
    """Eight clips of 0 .. 300 rows (63 / 64 / 65 rows: the 16-byte groups of the flat walk), policies from no mask to 16 + 16, four
    mask values (NaN and -0.0 are written as their bit patterns), in place and out of place: spans and rows equal the restatement, a
    masked element holds the mask value's bits and every other one its own (NaN payloads, denormals)."""
    import torch

    ro = _table(LENS)
    xh = np.concatenate([clip(cols, T, seed=i) for i, T in enumerate(LENS)])
    assert np.isnan(xh).any() and np.isinf(xh).any()
    masked_any = False
    for (nt, tw, ratio, nf, fw), base, epoch in (((2, 100, 1.0, 2, 27), 0, 0), ((0, 0, 1.0, 0, 0), 0, 1), ((1, 10, 0.2, 0, 0), 5, 2 ** 32 - 1),
                                                 ((0, 0, 0.0, 1, 1000), 5, 2 ** 32), ((16, 40, 1.0, 16, 3), 0, 7), ((3, 1000, 1.0, 2, 1), 2, 9)):
        want_spans = spans_ref((SEED, epoch), base, ro, len(xh), cols, nt, tw, ratio, nf, fw)
        for value in VALUES:
            got = {}
            for inplace in (False, True):
                block = _block(torch, SEED, epoch)
                bits, spans = _augment(torch, sslib, xh, ro, len(xh), block, base, nt, tw, ratio, nf, fw, value, inplace)
                assert np.array_equal(spans, want_spans), (nt, nf, value, inplace)
                want = _want(xh, ro, len(xh), want_spans, nt, nf, value, inplace)
                if not np.array_equal(bits, want):
                    bad = [b for b in range(len(LENS)) if not np.array_equal(bits[ro[b]:ro[b + 1]], want[ro[b]:ro[b + 1]])]
                    raise AssertionError((nt, tw, ratio, nf, fw, value, inplace, "clips", bad))
                assert _words(block) == [SEED, (epoch + 1) % 2 ** 64]
                got[inplace] = bits
            assert np.array_equal(got[False], got[True])  # every row is covered here: the two forms give the same bits
            masked_any |= bool((got[True] != u32(xh)).any())
    assert masked_any


@pytest.mark.parametrize("cols,rows", ((80, 3400), (13, 20400), (600, 500)))
def test_a_clip_longer_than_one_round_of_its_workgroups(sslib, cols, rows):
    """Three clips share the grid, so each has 64 workgroups; the long one has more elements than one round of them covers
    (FLAT_ROUND): the lanes move on by the uniform step.  cols = 600 with frequency spans of up to 520 columns also makes the in-place
    team of 256 lanes take several columns each."""
    import torch

    lens = [rows, 5, 130]
    assert rows * cols > FLAT_ROUND
    ro = _table(lens)
    xh = np.concatenate([clip(cols, T, seed=30 + i) for i, T in enumerate(lens)])
    nt, tw, nf, fw = 3, rows // 3, 3, 520 if cols == 600 else cols // 2
    want_spans = spans_ref((SEED, 11), 0, ro, len(xh), cols, nt, tw, 1.0, nf, fw)
    assert want_spans[0, :nt, 1].max() > 64 and (cols < 600 or want_spans[:, nt:, 1].max() > 256)
    for inplace in (False, True):
        bits, spans = _augment(torch, sslib, xh, ro, len(xh), _block(torch, SEED, 11), 0, nt, tw, 1.0, nf, fw, -1.5, inplace)
        assert np.array_equal(spans, want_spans) and np.array_equal(bits, _want(xh, ro, len(xh), want_spans, nt, nf, -1.5, inplace)), inplace


@pytest.mark.parametrize("cols", (13, 33))
def test_every_phase_of_the_input_and_the_output(sslib, cols):
    """vec starts one float into its allocation and out one float into its own (4-byte aligned only); cols is odd, so every clip's run
    starts at another 16-byte phase.  The bits are those of the aligned call, and the guards are untouched."""
    import torch

    lens = [70, 0, 65, 3, 64, 290]
    ro = _table(lens)
    xh = np.concatenate([clip(cols, T, seed=20 + i) for i, T in enumerate(lens)])
    want_spans = spans_ref((SEED, 3), 0, ro, len(xh), cols, 2, 30, 1.0, 2, 5)
    want = _want(xh, ro, len(xh), want_spans, 2, 2, -1.5, True)
    for inplace in (False, True):
        for phase in (0, 1):
            for in_phase in (0, 1) if not inplace else (0,):
                bits, spans = _augment(torch, sslib, xh, ro, len(xh), _block(torch, SEED, 3), 0, 2, 30, 1.0, 2, 5, -1.5, inplace, phase, in_phase)
                assert np.array_equal(spans, want_spans) and np.array_equal(bits, want), (inplace, phase, in_phase)
    shifted = _device_rows(torch, xh, 1)
    assert shifted.data_ptr() % 16 == 4


def test_hand_made_spans(sslib):
    """ss_mask_spans_packed_device on the caller's own table: the whole clip, every column, adjacent and overlapping spans, the last row
    and the last column, 16 + 16 spans, and spans that are out of range and therefore skipped whole."""
    import torch

    cols, lens = 13, [40, 9, 0, 66, 5]
    ro = _table(lens)
    xh = np.concatenate([clip(cols, T, seed=40 + i) for i, T in enumerate(lens)])
    n = len(lens)

    def table(nt, nf, per_clip):
        t = np.zeros((n, nt + nf, 2), np.int32)
        for b, pairs in per_clip.items():
            t[b, :len(pairs)] = pairs
        return t

    cases = {
        "the whole clip": (1, 0, table(1, 0, {0: [(0, 40)], 3: [(0, 66)], 4: [(0, 5)]})),
        "every column": (0, 1, table(0, 1, {b: [(0, cols)] for b in range(n)})),
        "adjacent and overlapping": (3, 3, table(3, 3, {0: [(3, 4), (7, 5), (10, 8), (2, 3), (5, 2), (6, 4)], 3: [(0, 1), (1, 1), (1, 64), (0, 6), (3, 3), (12, 1)]})),
        "the last row and the last column": (1, 1, table(1, 1, {b: [(T - 1, 1), (cols - 1, 1)] for b, T in enumerate(lens) if T})),
        "16 + 16": (16, 16, table(16, 16, {0: [(2 * k, 1) for k in range(16)] + [(k % cols, 1) for k in range(0, 32, 2)],
                                           3: [(4 * k, 3) for k in range(16)] + [(0, 0)] * 16})),
        # start < 0, width < 0, one past the extent (rows and columns), far out, and a (-1, 0) of a plan; one good span beside them
        "out of range": (4, 4, table(4, 4, {0: [(-1, 3), (5, -1), (38, 3), (4, 2), (-1, 0), (12, 2), (2 ** 31 - 1, 2 ** 31 - 1), (1, 2)],
                                            1: [(0, 10), (9, 1), (-2 ** 31, 5), (8, 1), (0, 14), (13, 1), (13, 0), (-2 ** 31, -2 ** 31)]})),
    }
    for name, (nt, nf, spans) in cases.items():
        for inplace in (False, True):
            bits = _mask(torch, sslib, xh, ro, len(xh), spans, nt, nf, -1.5, inplace)
            assert np.array_equal(bits, _want(xh, ro, len(xh), spans, nt, nf, -1.5, inplace)), (name, inplace)
    m = _bits_of(-1.5)
    whole = _mask(torch, sslib, xh, ro, len(xh), cases["the whole clip"][2], 1, 0, -1.5, True)
    assert (whole[ro[0]:ro[1]] == m).all() and (whole[ro[3]:] == m).all() and np.array_equal(whole[ro[1]:ro[2]], u32(xh)[ro[1]:ro[2]])
    assert (_mask(torch, sslib, xh, ro, len(xh), cases["every column"][2], 0, 1, -1.5, False) == m).all()
    skipped = _mask(torch, sslib, xh, ro, len(xh), cases["out of range"][2], 4, 4, -1.5, True)
    want = u32(xh).copy()
    want[4:6] = m
    want[0:40, 1:3] = m
    want[40 + 8] = m  # (13, 0) is in range and masks nothing
    assert np.array_equal(skipped, want)
    # one plan applied to two blocks
    other = np.concatenate([clip(cols, T, seed=50 + i) for i, T in enumerate(lens)])
    plan = spans_ref((SEED, 0), 0, ro, len(xh), cols, 2, 20, 1.0, 2, 4)
    a, b = (_mask(torch, sslib, x, ro, len(xh), plan, 2, 2, 0.0, False) for x in (xh, other))
    assert np.array_equal(a, _want(xh, ro, len(xh), plan, 2, 2, 0.0, False)) and np.array_equal(b, _want(other, ro, len(xh), plan, 2, 2, 0.0, False))


#        b0 good | b1 reversed | b2 good | b3 ends below 0 | b4 starts below 0 | b5 no rows | b6 past the end | b7 reversed | b8 .. b11 good (b10 no rows)
BAD_HEAD = [10, 17, 4, 10, -2, 4, 4, 60, 17, 25, 31, 31, 36]
BAD_LAST = {"good": [45], "reversed": [30], "negative": [-5, 3], "past_the_end": [51]}


@pytest.mark.parametrize("last", sorted(BAD_LAST))
def test_bad_segments_are_contained(sslib, last):
    """Reversed, negative and past-the-end segments, in the interior and as the last clip, over a block allocated exactly to size; rows
    0 .. 3 and 45 .. 49 are in no clip.  A bad clip's spans are (-1, 0), its rows and the rows in no clip are untouched (out of place:
    unwritten), and every good clip has the spans and the bits of a call on that clip alone."""
    import torch

    ro = np.array(BAD_HEAD + BAD_LAST[last], np.int64)
    cols, total_rows = 13, 50
    n = len(ro) - 1
    good = [b for b in range(n) if 0 <= ro[b] <= ro[b + 1] <= total_rows]
    assert good[:7] == [0, 2, 5, 8, 9, 10, 11] and (n - 1 in good) == (last == "good") and len(good) < n
    xh = clip(cols, total_rows, seed=50)
    covered = np.zeros(total_rows, bool)
    for b in good:
        assert not covered[ro[b]:ro[b + 1]].any()  # the good clips do not overlap
        covered[ro[b]:ro[b + 1]] = True
    policy = (2, 4, 1.0, 2, 5)
    want_spans = spans_ref((SEED, 4), 0, ro, total_rows, cols, 2, 4, 1.0, 2, 5)
    for inplace in (False, True):
        bits, spans = _augment(torch, sslib, xh, ro, total_rows, _block(torch, SEED, 4), 0, *policy, -1.5, inplace)
        assert np.array_equal(spans, want_spans) and np.array_equal(bits, _want(xh, ro, total_rows, want_spans, 2, 2, -1.5, inplace)), inplace
        for b in range(n):
            assert (spans[b] == (-1, 0)).all() == (b not in good), b
        assert np.array_equal(bits[~covered], u32(xh)[~covered]) if inplace else (bits[~covered] == SENTINEL).all()
        for b in good:  # the clip alone, as clip `b` of its own call
            T = int(ro[b + 1] - ro[b])
            if T:
                alone, alone_spans = _augment(torch, sslib, np.array(xh[ro[b]:ro[b + 1]]), [0, T], T, _block(torch, SEED, 4), b, *policy, -1.5, inplace)
                assert np.array_equal(alone_spans[0], spans[b]) and np.array_equal(alone, bits[ro[b]:ro[b + 1]]), (inplace, b)
    assert (bits != u32(xh))[covered].any()


def test_a_clips_masks_do_not_depend_on_its_place(sslib):
    """Clips [A, B, C] at clip_base 0 and [B, C] at clip_base 1 give B and C the same spans and the same bits."""
    import torch

    cols = 33
    A, B, Cc = clip(cols, 71, seed=60), clip(cols, 130, seed=61), clip(cols, 64, seed=62)
    policy = (2, 50, 1.0, 2, 9)
    for inplace in (False, True):
        abc, s_abc = _augment(torch, sslib, np.concatenate([A, B, Cc]), _table([71, 130, 64]), 265, _block(torch, SEED, 8), 0, *policy, 0.0, inplace)
        bc, s_bc = _augment(torch, sslib, np.concatenate([B, Cc]), _table([130, 64]), 194, _block(torch, SEED, 8), 1, *policy, 0.0, inplace)
        assert np.array_equal(s_abc[1:], s_bc) and np.array_equal(abc[71:], bc)
        assert not np.array_equal(s_abc[:2], s_bc)  # ... and not those of the clips in front of them
        assert (bc != u32(np.concatenate([B, Cc]))).any()


def test_only_the_combined_call_advances_the_epoch(sslib):
    import torch

    cols, lens = 13, [20, 31]
    ro = _table(lens)
    xh = np.concatenate([clip(cols, T, seed=70 + i) for i, T in enumerate(lens)])
    x, d_ro = _device_rows(torch, xh), torch.from_numpy(ro).cuda()
    for epoch in (0, 41, 2 ** 32 - 1, 2 ** 64 - 1):  # the carry into the high dword, and the wrap
        block = _block(torch, SEED, epoch)
        b = Bufs(torch, len(xh), cols, 2, 4)
        assert sslib.ss_specaug_plan_packed_device(block.data_ptr(), 0, 2, d_ro.data_ptr(), len(xh), cols, 2, 10, 1.0, 2, 4, b.spans.data_ptr(), _stream()) == 0
        assert sslib.ss_mask_spans_packed_device(x.data_ptr(), 2, d_ro.data_ptr(), len(xh), cols, b.spans.data_ptr(), 2, 2, 0.0, b.out.data_ptr(), _stream()) == 0
        two_calls, two_spans = b.result()
        assert _words(block) == [SEED, epoch]  # the plan-only and the apply-only call leave the block alone
        bits, spans = _augment(torch, sslib, xh, ro, len(xh), block, 0, 2, 10, 1.0, 2, 4, 0.0, False)
        assert _words(block) == [SEED, (epoch + 1) % 2 ** 64]
        assert np.array_equal(spans, two_spans) and np.array_equal(bits, two_calls)  # the combined call is the two launches
        again, spans2 = _augment(torch, sslib, xh, ro, len(xh), block, 0, 2, 10, 1.0, 2, 4, 0.0, False)
        assert _words(block) == [SEED, (epoch + 2) % 2 ** 64]
        assert np.array_equal(spans2, spans_ref((SEED, (epoch + 1) % 2 ** 64), 0, ro, len(xh), cols, 2, 10, 1.0, 2, 4)) and not np.array_equal(spans2, spans)


def test_a_captured_graph_draws_fresh_masks_on_every_replay(sslib):
    """The combined call, in place, captured after a warm-up outside the capture and replayed three times on a restored input with no
    host involvement in between: spans and rows are the restatement's at epochs e, e + 1, e + 2 (e + 1 carries into the high dword)."""
    import torch

    cols, lens = 13, [70, 0, 33, 130]
    ro = _table(lens)
    R, n = int(ro[-1]), len(lens)
    xh = np.concatenate([clip(cols, T, seed=80 + i) for i, T in enumerate(lens)])
    d_ro = torch.from_numpy(ro).cuda()
    e = 2 ** 32 - 2
    block = _block(torch, SEED, e - 1)  # the warm-up call takes one epoch
    b = Bufs(torch, R, cols, n, 4).load(torch, xh)

    def call(stream):
        rc = sslib.ss_specaug_packed_device(b.out.data_ptr(), n, d_ro.data_ptr(), R, cols, block.data_ptr(), 0, 2, 30, 1.0, 2, 5, -0.0, b.out.data_ptr(),
                                            b.spans.data_ptr(), C.c_void_p(stream))
        assert rc == 0, sslib.ss_last_error_string()

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up outside the capture
        call(side.cuda_stream)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert _words(block) == [SEED, e]
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call(torch.cuda.current_stream().cuda_stream)
    assert _words(block) == [SEED, e]  # capturing runs nothing
    seen = []
    for k in range(3):
        b.reset()
        b.load(torch, xh)
        g.replay()
        bits, spans = b.result()
        want_spans = spans_ref((SEED, e + k), 0, ro, R, cols, 2, 30, 1.0, 2, 5)
        assert np.array_equal(spans, want_spans), k
        assert np.array_equal(bits, _want(xh, ro, R, want_spans, 2, 2, -0.0, True)), k
        assert _words(block) == [SEED, e + k + 1]
        seen.append(spans.tobytes())
    assert len(set(seen)) == 3


def test_host_forms_and_python_front_equal_the_device_calls(ss, sslib):
    import torch

    cols, lens = 33, [0, 1, 129, 70, 7]
    ro = _table(lens)
    xh = np.concatenate([clip(cols, T, seed=90 + i) for i, T in enumerate(lens)])
    xh = np.concatenate([xh, clip(cols, 3, seed=99)])  # three rows behind the last clip: in no clip
    R, n, epoch = len(xh), len(lens), 2 ** 32 - 1
    policy = dict(time_masks=2, time_width=40, time_ratio=0.5, freq_masks=3, freq_width=6, clip_base=4)
    args = (2, 40, 0.5, 3, 6)
    for value in (-1.5, float("nan")):
        dev, dev_spans = _augment(torch, sslib, xh, ro, R, _block(torch, SEED, epoch), 4, *args, value, False)
        dev_in, _ = _augment(torch, sslib, xh, ro, R, _block(torch, SEED, epoch), 4, *args, value, True)
        assert np.array_equal(dev_spans, spans_ref((SEED, epoch), 4, ro, R, cols, *args))
        # the host forms, into host buffers with a spare element behind them
        for inplace in (False, True):
            rng = np.array([SEED, epoch], np.uint64)
            spans = np.full(n * 5 * 2 + 1, SPAN_SENT, np.int32)
            out = np.full(R * cols + 1, SENTINEL, np.uint32)
            src = out if inplace else xh
            if inplace:
                out[:-1] = u32(xh).reshape(-1)
            rc = sslib.ss_specaug_packed(src.ctypes.data, n, ro.ctypes.data, R, cols, rng.ctypes.data, 4, *args, value, out.ctypes.data, spans.ctypes.data)
            assert rc == 0, sslib.ss_last_error_string()
            assert rng.tolist() == [SEED, epoch + 1] and spans[-1] == SPAN_SENT and out[-1] == SENTINEL
            assert np.array_equal(spans[:-1].reshape(n, 5, 2), dev_spans)
            assert np.array_equal(out[:-1].reshape(R, cols), dev_in if inplace else dev), inplace  # the uncovered rows keep what the buffer held
            out2 = np.full(R * cols + 1, SENTINEL, np.uint32)
            if inplace:
                out2[:-1] = u32(xh).reshape(-1)
            rc = sslib.ss_mask_spans_packed((out2 if inplace else xh).ctypes.data, n, ro.ctypes.data, R, cols, spans.ctypes.data, 2, 3, value, out2.ctypes.data)
            assert rc == 0, sslib.ss_last_error_string()
            assert np.array_equal(out2, out)
        # the Python front on tensors: a SpecAugment, in place and out of place, and its block handed in directly
        xd, d_ro = torch.from_numpy(xh).cuda(), torch.from_numpy(ro).cuda()
        aug = ss.SpecAugment(SEED, epoch)
        assert (aug.seed, aug.epoch) == (SEED, epoch)
        for table in (d_ro, ro, list(ro)):
            aug.epoch = epoch
            got, sp = aug(xd, table, mask_value=value, **policy)
            assert torch.is_tensor(got) and got.is_cuda and got.shape == xd.shape and sp.dtype == torch.int32 and tuple(sp.shape) == (n, 5, 2)
            covered = slice(0, int(ro[-1]))
            assert np.array_equal(u32(got.cpu().numpy())[covered], dev[covered]) and np.array_equal(sp.cpu().numpy(), dev_spans)
            assert aug.epoch == epoch + 1 and aug.seed == SEED
        work = xd.clone()
        got, sp = ss.spec_augment_packed(work, d_ro, _block(torch, SEED, epoch), mask_value=value, out=work, **policy)
        assert got is work and np.array_equal(u32(work.cpu().numpy()), dev_in) and np.array_equal(sp.cpu().numpy(), dev_spans)
        again = ss.mask_spans_packed(xd, d_ro, sp, 2, 3, value)
        assert np.array_equal(u32(again.cpu().numpy())[covered], dev[covered])
        work = xd.clone()
        assert ss.mask_spans_packed(work, ro, dev_spans, 2, 3, value, out=work) is work and np.array_equal(u32(work.cpu().numpy()), dev_in)
        assert np.array_equal(u32(xd.cpu().numpy()), u32(xh))  # the input of an out-of-place call is read only
        # ... and on numpy arrays: the rng array is advanced in place, a SpecAugment too
        rng = np.array([SEED, epoch], np.uint64)
        got, sp = ss.spec_augment_packed(xh, ro, rng, mask_value=value, **policy)
        assert isinstance(got, np.ndarray) and np.array_equal(u32(got)[covered], dev[covered]) and np.array_equal(sp, dev_spans) and rng.tolist() == [SEED, epoch + 1]
        aug.epoch = epoch
        work = np.array(xh)
        got, sp = ss.spec_augment_packed(work, ro, aug, mask_value=value, out=work, **policy)
        assert got is work and np.array_equal(u32(work), dev_in) and np.array_equal(sp, dev_spans) and aug.epoch == epoch + 1
        assert np.array_equal(u32(ss.mask_spans_packed(xh, ro, dev_spans, 2, 3, value))[covered], dev[covered])
        assert np.array_equal(ss.spec_augment_spans(aug, ro, cols, total_rows=R, **policy), spans_ref((SEED, epoch + 1), 4, ro, R, cols, *args))
    # every clip empty: nothing to mask, the spans are still drawn and the epoch advances
    aug = ss.SpecAugment(5, 0)
    out, sp = aug(torch.zeros((0, cols), device="cuda"), [0, 0, 0])
    assert out.shape == (0, cols) and np.array_equal(sp.cpu().numpy(), spans_ref((5, 0), 0, [0, 0, 0], 0, cols, 2, 100, 1.0, 2, 27)) and aug.epoch == 1
