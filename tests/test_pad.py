"""Padded-batch collation on the device: ss_pad_packed_device / ss_pad_packed and the Python front's pad_packed and pad.

Every comparison is on bit patterns against the numpy restatement of the header (tests/pad_model.py): float32 bit for bit, the
16-bit types bit for bit off-NaN with a NaN exactly where a NaN went in.  The inputs are salted with NaNs, -0.0, +-inf and
denormals (splice_model.clip); out and lengths are pre-filled with a sentinel that no call can produce and sit between guards of it.
"""
import ctypes as C

import numpy as np
import pytest

from pad_model import BITS_DTYPE, DTYPE_CODE, DTYPES, LAYOUT_CODE, LAYOUTS, PAD_ROUNDS, clip, pad_ref, same, u32

pytestmark = pytest.mark.gpu

TILE_T = 128  # kTileT, mfcc-rust_amd/csrc/ss_pad.hip: "constexpr unsigned kTileT = 128, kTileC = 32;  // the BCT tile: time rows x columns"
GUARD = 64   # elements in front of and behind out and lengths
# Bit patterns the stage cannot write: the float32 one is in no input (splice_model.SENTINEL); the 16-bit ones are signalling NaNs,
# and a NaN the conversions produce is quiet.  No pad value of these tests is one.
SENT = {"float32": 0xDEADBEEF, "float16": 0x7D55, "bfloat16": 0x7FA5}
LEN_SENT = -77
PADS = (0.0, -1.5, float(PAD_ROUNDS))
# empty, a lone row, two rows, 63 / 64 / 65 (the flat walk's 16-byte groups and half a tile), one below, at and above a tile edge, more
# than two tiles (the issue's 130 raised to the tile of 128 rows)
LENS = [0, 1, 2, 63, 64, 65, TILE_T - 1, TILE_T, TILE_T + 1, 2 * TILE_T + 2, 7]
MAX_ROWS = (1, 64, 65, 131, 200, TILE_T, TILE_T + 1, 2 * TILE_T + 3, 300)


def _signed(v, bits):
    return v - (1 << bits) if v >= 1 << (bits - 1) else v


def _stream():
    import torch

    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _table(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


class Bufs:
    """out and lengths between guards, everything pre-filled with the sentinel; `phase` = 1 starts out one element into its allocation"""

    def __init__(self, torch, n, max_rows, cols, layout, dtype, phase=0):
        self.dtype, self.n = dtype, n
        self.shape = (n, max_rows, cols) if layout == "btc" else (n, cols, max_rows)
        self.count = n * max_rows * cols
        tdt, bits = (torch.int32, 32) if dtype == "float32" else (torch.int16, 16)
        self.raw = torch.full((phase + GUARD + self.count + GUARD,), _signed(SENT[dtype], bits), dtype=tdt, device="cuda")
        self.out = self.raw[phase + GUARD:phase + GUARD + self.count]
        self.len_raw = torch.full((GUARD + n + GUARD,), LEN_SENT, dtype=torch.int32, device="cuda")
        self.lengths = self.len_raw[GUARD:GUARD + n]

    def result(self):
        """-> (bits, lengths) on the host, after checking that the guards are untouched and that no element of out or lengths is"""
        import torch

        torch.cuda.synchronize()
        raw = self.raw.cpu().numpy().view(BITS_DTYPE[self.dtype])
        at = raw.size - GUARD - self.count
        assert (raw[:at] == SENT[self.dtype]).all() and (raw[at + self.count:] == SENT[self.dtype]).all(), "guard of out"
        lr = self.len_raw.cpu().numpy()
        assert (lr[:GUARD] == LEN_SENT).all() and (lr[GUARD + self.n:] == LEN_SENT).all(), "guard of lengths"
        bits, lengths = raw[at:at + self.count].reshape(self.shape), lr[GUARD:GUARD + self.n]
        assert not (bits == SENT[self.dtype]).any() and not (lengths == LEN_SENT).any(), "an element was not written"
        return bits, lengths


def _raw(lib, x, n, d_ro, total_rows, cols, max_rows, layout, dtype, pad, out, lengths, stream=None):
    return lib.ss_pad_packed_device(x.data_ptr(), n, d_ro.data_ptr(), total_rows, cols, max_rows, LAYOUT_CODE[layout], DTYPE_CODE[dtype], pad,
                                    out.data_ptr(), lengths.data_ptr(), stream if stream is not None else _stream())


def _pad(torch, lib, x, d_ro, total_rows, cols, max_rows, layout, dtype, pad, phase=0):
    """one device call on a device block and table -> (bits, lengths) on the host, guards checked"""
    n = d_ro.numel() - 1
    b = Bufs(torch, n, max_rows, cols, layout, dtype, phase)
    assert _raw(lib, x, n, d_ro, total_rows, cols, max_rows, layout, dtype, pad, b.out, b.lengths) == 0, lib.ss_last_error_string()
    return b.result()


def _pad_host(torch, lib, xh, ro, max_rows, layout, dtype, pad, total_rows=None):
    """the same from host arrays; the block is allocated exactly to size (a block without rows still needs an address: one spare row)"""
    x = torch.from_numpy(np.array(xh, np.float32) if len(xh) else np.zeros((1, xh.shape[1]), np.float32)).cuda()
    total = len(xh) if total_rows is None else total_rows
    return _pad(torch, lib, x, torch.from_numpy(np.asarray(ro, np.int64)).cuda(), total, xh.shape[1], max_rows, layout, dtype, pad)


@pytest.mark.parametrize("cols", (1, 13, 33, 64, 65, 80, 240))
def test_the_batch_is_the_restatement_bit_for_bit(sslib, cols):
    """One block of eleven clips -- none, one and two rows, 63 / 64 / 65, one below, at and one above a tile of TILE_T time rows, more
    than two tiles -- for max_rows that truncates (1, 64, 65, 131, 200), is a clip's length exactly (64, 65, TILE_T, TILE_T + 1), is
    odd, is one above the longest clip (2 TILE_T + 3) and leaves an all-pad tail behind every clip (300); both layouts, the three
    element types, three pad values.  Eleven clips share the grid's 8192 workgroups, so every clip's groups and tiles are spread over
    several workgroups."""
    import torch

    assert LENS[-2] == 258 and max(LENS) <= 300
    ro = _table(LENS)
    xh = np.concatenate([clip(cols, T, seed=i) for i, T in enumerate(LENS)])
    assert np.isnan(xh).any() and np.isinf(xh).any()
    x, d_ro = torch.from_numpy(xh).cuda(), torch.from_numpy(ro).cuda()
    for max_rows in MAX_ROWS:
        for layout in LAYOUTS:
            for dtype in DTYPES:
                for pad in PADS:
                    bits, lengths = _pad(torch, sslib, x, d_ro, len(xh), cols, max_rows, layout, dtype, pad)
                    want, nan, want_len = pad_ref(xh, ro, len(xh), max_rows, layout, dtype, pad)
                    assert np.array_equal(lengths, want_len), (max_rows, layout, dtype)
                    if not same(bits, want, nan, dtype):
                        bad = [b for b in range(len(LENS)) if not same(bits[b], want[b], nan[b], dtype)]
                        raise AssertionError((max_rows, layout, dtype, pad, "clips", bad))


@pytest.mark.parametrize("layout", LAYOUTS)
def test_every_phase_of_the_input_and_the_output(sslib, layout):
    """vec starts one float into its allocation (4-byte aligned only) and out one element into its own (2-byte aligned for the halves,
    4-byte for float32); cols = 13 and max_rows = 65 (and 257: three tiles) are odd, so the clips' blocks and, channels first, every
    output row start at another 16-byte phase.  The bits are those of the aligned call, and the guards are untouched."""
    import torch

    cols = 13
    lens = [70, 0, 65, 3, 64, 290]
    ro = _table(lens)
    xh = np.concatenate([clip(cols, T, seed=20 + i) for i, T in enumerate(lens)])
    aligned = torch.from_numpy(xh).cuda()
    shifted = torch.zeros(xh.size + 1, device="cuda")[1:].view(len(xh), cols)
    shifted.copy_(aligned)
    assert shifted.data_ptr() % 16 == 4
    d_ro = torch.from_numpy(ro).cuda()
    for max_rows in (65, 2 * TILE_T + 1):  # and the same over three tiles of an odd row
        for dtype in DTYPES:
            base, base_len = _pad(torch, sslib, aligned, d_ro, len(xh), cols, max_rows, layout, dtype, -1.5)
            want, nan, want_len = pad_ref(xh, ro, len(xh), max_rows, layout, dtype, -1.5)
            assert same(base, want, nan, dtype) and np.array_equal(base_len, want_len), (max_rows, dtype)
            for x in (aligned, shifted):
                for phase in (0, 1):
                    bits, lengths = _pad(torch, sslib, x, d_ro, len(xh), cols, max_rows, layout, dtype, -1.5, phase=phase)
                    assert np.array_equal(bits, base) and np.array_equal(lengths, base_len), (max_rows, dtype, phase)  # NaN payloads included


@pytest.mark.parametrize("layout,dtype,cols,max_rows", [("btc", "float32", 13, 150), ("bct", "bfloat16", 13, 150), ("bct", "float16", 80, 131),
                                                        ("btc", "bfloat16", 33, 65), ("bct", "float32", 65, 64),
                                                        ("btc", "float32", 240, 1100), ("bct", "bfloat16", 240, 1100)])
def test_a_clips_block_does_not_depend_on_its_place(sslib, layout, dtype, cols, max_rows):
    """Permuting the clips permutes the blocks, a one-row spacer clip changes no other block, and a clip alone gives the block it had
    in the batch -- at other row offsets, block phases and workgroup splits.  The two cases with max_rows = 1100 and cols = 240 give
    a clip more 16-byte groups (float32, flat: 65 steps of 1024) and more tiles (channels first: 9 x 8) than the 64 workgroups a clip
    can get: there a workgroup takes several."""
    import torch

    lens = [2 * TILE_T + 22, 7, 0, 300, 1] if max_rows < 1000 else [300, 7]
    clips = [clip(cols, T, seed=40 + i) for i, T in enumerate(lens)]

    def run(order):
        chosen = [clips[i] if i >= 0 else clip(cols, 1, seed=59) for i in order]
        return _pad_host(torch, sslib, np.concatenate(chosen), _table([len(c) for c in chosen]), max_rows, layout, dtype, PAD_ROUNDS)

    ident = list(range(len(lens)))
    base, base_len = run(ident)
    want, nan, want_len = pad_ref(np.concatenate(clips), _table(lens), sum(lens), max_rows, layout, dtype, PAD_ROUNDS)
    assert same(base, want, nan, dtype) and np.array_equal(base_len, want_len)
    perm = ident[::-1] if len(lens) == 2 else [3, 0, 4, 2, 1]
    spaced = ident[:1] + [-1] + ident[1:]  # a spacer behind the first clip: every later clip moves by one odd row
    for order in (perm, spaced) + tuple([i] for i in ident):
        bits, lengths = run(order)
        for at, i in enumerate(order):
            if i >= 0:
                assert np.array_equal(bits[at], base[i]) and lengths[at] == base_len[i], (order, i)


def _bad_tables():
    from test_splice import LAST  # the catalogue of bad last clips: reversed, negative, past total_rows (and the good one)

    #       b0 good | b1 reversed | b2 good | b3 ends below 0 | b4 starts below 0 | b5 .. b8 good | b9 no rows | b10 good | the last clip(s)
    head = [0, 7, 4, 10, -2, 6, 12, 19, 25, 31, 31, 36]
    return {name: np.array(head + add_ro, np.int64) for name, (add_ro, _, _, _) in LAST.items()}


@pytest.mark.parametrize("last", ("good", "negative", "past_the_end", "reversed"))
def test_bad_segments_are_contained(sslib, last):
    """Reversed, negative and past-the-end segments, in the interior and as the last clip, over a block allocated exactly to size: a bad
    clip's block is all pad and its length -1, an empty clip's is all pad and 0, every other clip is what it is in a call on the good
    clips alone, every element is rewritten and the guards are untouched."""
    import torch

    ro = _bad_tables()[last]
    cols, total_rows, max_rows = 13, 50, 5
    n = len(ro) - 1
    good = [b for b in range(n) if 0 <= ro[b] <= ro[b + 1] <= total_rows]
    assert good[:8] == [0, 2, 5, 6, 7, 8, 9, 10] and (n - 1 in good) == (last == "good") and len(good) < n
    xh = clip(cols, total_rows, seed=50)
    x, d_ro = torch.from_numpy(xh.copy()).cuda(), torch.from_numpy(ro).cuda()
    clean_x = np.concatenate([xh[ro[b]:ro[b + 1]] for b in good])
    clean_ro = _table([int(ro[b + 1] - ro[b]) for b in good])
    for layout in LAYOUTS:
        for dtype in DTYPES:
            bits, lengths = _pad(torch, sslib, x, d_ro, total_rows, cols, max_rows, layout, dtype, -1.5)
            want, nan, want_len = pad_ref(xh, ro, total_rows, max_rows, layout, dtype, -1.5)
            assert np.array_equal(lengths, want_len) and same(bits, want, nan, dtype), (layout, dtype)
            assert [int(v) for v in lengths] == [min(int(ro[b + 1] - ro[b]), max_rows) if b in good else -1 for b in range(n)]
            pad_bits = want[1].reshape(-1)[0]
            clean, clean_len = _pad_host(torch, sslib, clean_x, clean_ro, max_rows, layout, dtype, -1.5)
            for i, b in enumerate(good):
                assert np.array_equal(bits[b], clean[i]) and lengths[b] == clean_len[i], (layout, dtype, b)
            for b in set(range(n)) - set(good):
                assert (bits[b] == pad_bits).all(), (layout, dtype, b)
    assert np.array_equal(u32(x.cpu().numpy()), u32(xh)) and np.array_equal(d_ro.cpu().numpy(), ro)  # the inputs are read only


def test_the_tick_batch_of_a_stream_pool(sslib):
    """The row_offsets of a stream-pool call are a valid table: 37 entries of 0 - 4 rows with max_rows = the largest chunk give the
    [n_active x 4 x 80] batch of a streaming model."""
    import torch

    rng = np.random.default_rng(5)
    lens = rng.integers(0, 5, 37)
    lens[:5] = [0, 4, 1, 0, 3]
    ro = _table(lens)
    xh = clip(80, int(ro[-1]), seed=60)
    bits, lengths = _pad_host(torch, sslib, xh, ro, 4, "btc", "bfloat16", 0.0)
    want, nan, want_len = pad_ref(xh, ro, len(xh), 4, "btc", "bfloat16", 0.0)
    assert bits.shape == (37, 4, 80) and same(bits, want, nan, "bfloat16") and np.array_equal(lengths, lens.astype(np.int32)) and np.array_equal(lengths, want_len)


def test_host_form_and_python_front_equal_the_device_form(ss, sslib):
    import torch

    cols, lens = 33, [0, 1, TILE_T + 1, 2 * TILE_T + 3, 7]
    ro = _table(lens)
    xh = np.concatenate([clip(cols, T, seed=70 + i) for i, T in enumerate(lens)])
    xd, d_ro = torch.from_numpy(xh).cuda(), torch.from_numpy(ro).cuda()
    tdt = {"float32": torch.float32, "float16": torch.float16, "bfloat16": torch.bfloat16}
    for layout in LAYOUTS:
        for dtype in DTYPES:
            max_rows = TILE_T + 12
            dev, dev_len = _pad(torch, sslib, xd, d_ro, len(xh), cols, max_rows, layout, dtype, -1.5)
            assert sslib.ss_last_kernel_name().decode() == "ss_pad_packed_kernel<%s,%s>" % (layout, {"float32": "f32", "float16": "f16", "bfloat16": "bf16"}[dtype])
            # the host form, into a host buffer with a spare element behind it
            host = np.full(dev.size + 1, SENT[dtype], BITS_DTYPE[dtype])
            host_len = np.full(len(lens) + 1, LEN_SENT, np.int32)
            rc = sslib.ss_pad_packed(xh.ctypes.data, len(lens), ro.ctypes.data, len(xh), cols, max_rows, LAYOUT_CODE[layout], DTYPE_CODE[dtype], -1.5,
                                     host.ctypes.data, host_len.ctypes.data)
            assert rc == 0, sslib.ss_last_error_string()
            assert np.array_equal(host[:-1].reshape(dev.shape), dev) and host[-1] == SENT[dtype]
            assert np.array_equal(host_len[:-1], dev_len) and host_len[-1] == LEN_SENT
            # the Python front: numpy in, tensors in (a device table and a host table), the dtype objects, the list form
            got_np, len_np = ss.pad_packed(xh, ro, max_rows, layout, dtype, -1.5)
            assert isinstance(got_np, np.ndarray) and got_np.dtype == {"float32": np.float32, "float16": np.float16, "bfloat16": np.uint16}[dtype]
            assert got_np.shape == dev.shape and np.array_equal(got_np.view(BITS_DTYPE[dtype]), dev) and np.array_equal(len_np, dev_len) and len_np.dtype == np.int32
            for table in (d_ro, ro, list(ro)):
                for dt in (dtype, tdt[dtype]):
                    got_t, len_t = ss.pad_packed(xd, table, max_rows, layout, dt, -1.5)
                    assert torch.is_tensor(got_t) and got_t.is_cuda and got_t.dtype == tdt[dtype] and len_t.is_cuda and len_t.dtype == torch.int32
                    raw = got_t.view(torch.int32 if dtype == "float32" else torch.int16).cpu().numpy().view(BITS_DTYPE[dtype])
                    assert raw.shape == dev.shape and np.array_equal(raw, dev) and np.array_equal(len_t.cpu().numpy(), dev_len)
            assert np.array_equal(ss.pad_packed(xh, ro, max_rows, layout, tdt[dtype], -1.5)[0].view(BITS_DTYPE[dtype]), dev)
            # max_rows=None: the longest clip of a host table
            longest, len_l = ss.pad_packed(xd, ro, None, layout, dtype, -1.5)
            want, nan, want_len = pad_ref(xh, ro, len(xh), max(lens), layout, dtype, -1.5)
            raw = longest.view(torch.int32 if dtype == "float32" else torch.int16).cpu().numpy().view(BITS_DTYPE[dtype])
            assert same(raw, want, nan, dtype) and np.array_equal(len_l.cpu().numpy(), want_len) and len_l.cpu().tolist() == lens
            with pytest.raises(ValueError, match="max_rows"):
                ss.pad_packed(xd, d_ro, None, layout, dtype)
            # the list form, of tensors and of arrays
            parts = [xh[ro[i]:ro[i + 1]] for i in range(len(lens))]
            got_l, len_ll = ss.pad([torch.from_numpy(p.copy()).cuda() for p in parts], max_rows, layout, dtype, -1.5)
            assert np.array_equal(got_l.view(torch.int32 if dtype == "float32" else torch.int16).cpu().numpy().view(BITS_DTYPE[dtype]), dev)
            assert np.array_equal(len_ll.cpu().numpy(), dev_len)
            got_l, len_ll = ss.pad(parts, max_rows, layout, dtype, -1.5)
            assert np.array_equal(got_l.view(BITS_DTYPE[dtype]), dev) and np.array_equal(len_ll, dev_len)
    # every clip empty: all pad, no row is read
    out, lengths = ss.pad_packed(torch.zeros((0, cols), device="cuda"), [0, 0, 0], 3, "bct", "bfloat16", 1.0)
    assert out.shape == (2, cols, 3) and (out == 1.0).all() and lengths.cpu().tolist() == [0, 0]


def test_the_chain_from_the_selection_to_the_batch_replays_as_one_graph(ss, sslib):
    """ss_select_rows_packed_device -> ss_cmvn_packed_device -> ss_pad_packed_device (channels first, bfloat16) on d_out_offsets with
    total_rows as the bound, a linear chain captured in one graph and replayed twice over other mask contents with no read in
    between: each replay is numpy's selection, ss_cmvn_packed_device on the host-made table and the restatement of the collation."""
    import torch

    from vad_model import select_ref

    cols, max_rows = 13, TILE_T + 12
    lens = [300, 0, 1, 90, 45, TILE_T + 3]
    off = _table(lens)
    R, n = int(off[-1]), len(lens)
    rng = np.random.default_rng(11)
    xh = (rng.standard_normal((R, cols)) * 3 + 1).astype(np.float32)  # cmvn is arithmetic: finite rows
    x, d_off = torch.from_numpy(xh).cuda(), torch.from_numpy(off).cuda()
    mask = torch.zeros(R, dtype=torch.uint8, device="cuda")
    oo = torch.full((n + 1,), -77, dtype=torch.int64, device="cuda")
    sel, norm = torch.zeros((R, cols), device="cuda"), torch.zeros((R, cols), device="cuda")
    b = Bufs(torch, n, max_rows, cols, "bct", "bfloat16")

    def chain(stream):
        st = C.c_void_p(stream)
        assert sslib.ss_select_rows_packed_device(x.data_ptr(), n, d_off.data_ptr(), R, cols, mask.data_ptr(), oo.data_ptr(), sel.data_ptr(), st) == 0
        assert sslib.ss_cmvn_packed_device(sel.data_ptr(), n, oo.data_ptr(), R, cols, 1, norm.data_ptr(), st) == 0, sslib.ss_last_error_string()
        assert _raw(sslib, norm, n, oo, R, cols, max_rows, "bct", "bfloat16", 0.0, b.out, b.lengths, stream=st) == 0, sslib.ss_last_error_string()

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up outside the capture
        chain(side.cuda_stream)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        chain(torch.cuda.current_stream().cuda_stream)
    for k in range(2):
        mh = (rng.random(R) < (0.7, 0.35)[k]).astype(np.uint8)
        mask.copy_(torch.from_numpy(mh))
        b.raw.fill_(_signed(SENT["bfloat16"], 16))
        b.len_raw.fill_(LEN_SENT)
        g.replay()
        bits, lengths = b.result()  # the first read of anything
        sel_h, oo_h = select_ref(xh, off, mh)
        K = int(oo_h[-1])
        assert 0 < K < R and np.array_equal(oo.cpu().numpy(), oo_h) and np.array_equal(u32(sel[:K].cpu().numpy()), u32(sel_h))
        d_sel, ref, d_oo = torch.from_numpy(sel_h).cuda(), torch.empty((K, cols), device="cuda"), torch.from_numpy(oo_h).cuda()
        assert sslib.ss_cmvn_packed_device(d_sel.data_ptr(), n, d_oo.data_ptr(), K, cols, 1, ref.data_ptr(), _stream()) == 0
        torch.cuda.synchronize()
        ref_h = ref.cpu().numpy()
        assert np.array_equal(u32(norm[:K].cpu().numpy()), u32(ref_h)), k
        want, nan, want_len = pad_ref(ref_h, oo_h, K, max_rows, "bct", "bfloat16", 0.0)
        assert same(bits, want, nan, "bfloat16") and np.array_equal(lengths, want_len), k
        assert np.array_equal(lengths, np.minimum(np.diff(oo_h), max_rows)) and (lengths < np.array(lens)).any()


def test_against_torch_on_kaldi_fbank_rows(ss):
    """NaN-free rows of kaldi_fbank_packed of three short clips: channels first in bfloat16 is torch's pad_sequence, transpose and
    conversion, element for element."""
    import torch
    from torch.nn.utils.rnn import pad_sequence

    n_samples = [4000, 1200, 2777]
    sig = torch.from_numpy(np.concatenate([_signal(80 + i, n) for i, n in enumerate(n_samples)])).cuda()
    rows, fo = ss.kaldi_fbank_packed(sig, n_samples, num_mel_bins=80)
    torch.cuda.synchronize()
    fo_h = fo.cpu().numpy() if torch.is_tensor(fo) else np.asarray(fo)
    lens = np.diff(fo_h).tolist()
    assert len(lens) == 3 and min(lens) > 0 and rows.shape == (sum(lens), 80) and torch.isfinite(rows).all()
    got, lengths = ss.pad_packed(rows, fo, max(lens), layout="bct", dtype=torch.bfloat16)
    want = pad_sequence(torch.split(rows, lens), batch_first=True).transpose(1, 2).to(torch.bfloat16)
    assert got.shape == (3, 80, max(lens)) and got.dtype == torch.bfloat16 and torch.equal(got, want)
    assert lengths.cpu().tolist() == lens
    got_btc, _ = ss.pad_packed(rows, fo, max(lens), dtype=torch.float16)
    assert torch.equal(got_btc, pad_sequence(torch.split(rows, lens), batch_first=True).to(torch.float16))


def _signal(seed, n):
    rng = np.random.default_rng(seed)
    t = np.arange(n, dtype=np.float64) / 16000.0
    return (0.3 * np.sin(2 * np.pi * (200.0 + 37.0 * seed) * t) + 0.05 * rng.standard_normal(n)).astype(np.float32)
