"""The arithmetic of the shapes of tests/test_large_blocks.py, from tests/large_blocks_model.py alone: no device and, but for the
last test (an argument rule that the dense-stride cases rest on, decided on the host), no library.

For every GPU case: the first element of the first tail clip lies at or past element 2^32 of each block the case stresses and at
or past byte 2^32 of the other big blocks; every count the header bounds is below 2^31; the peak device memory (every block in
full, plus scratch and pools) is at most 40 GiB; and the filler in front is just long enough.  These are conditions, not
measurements: a case that misses one is wrong here, before anything runs."""
import ctypes as C

import numpy as np
import pytest

import large_blocks_model as M

CASE_IDS = sorted(M.CASES)


def test_the_constants_are_the_documented_shapes():
    assert M.BIG == 2 ** 32 + 2 ** 22 and M.TWO32 == 2 ** 32 and M.CAP_BYTES == 40 * 2 ** 30
    assert M.TAIL_ROWS == (1, 63, 700, 2049, 4100) and M.FILLER_ROWS == 8192
    assert M.SAMPLE_LENS == (16000, 12345, 1, 48000, 801)
    assert all(h <= n and h % 160 == 0 and n - h < 160 for h, n in zip(M.HOP_LENS, M.SAMPLE_LENS))
    assert M.DENSE_LD == 2 ** 32 + 2
    w = M.WHISPER_BLOCK
    assert (w["n_clips"], w["n_mels"], w["n_frames"]) == (11200, 128, 3000)


@pytest.mark.parametrize("name", CASE_IDS)
def test_stressed_blocks_pass_element_two_to_the_32_and_the_others_byte_two_to_the_32(name):
    case = M.CASES[name]
    assert any(b.role == "stress" for b in case.blocks), "a case that stresses no block checks nothing"
    for b in case.blocks:
        assert 0 <= b.tail < b.elems, (name, b.name)
        if b.role == "stress":
            assert b.tail >= M.TWO32, (name, b.name, b.tail)
        elif b.role == "bytes":
            assert b.tail_byte >= M.TWO32, (name, b.name, b.tail_byte)
        else:
            # one byte per row: cannot reach 2^32 while total_rows < 2^31
            assert b.role == "small" and b.elem_bytes == 1 and b.elems < M.LIMIT31, (name, b.name)


@pytest.mark.parametrize("name", CASE_IDS)
def test_counts_stay_inside_the_headers_limits(name):
    case = M.CASES[name]
    for key in ("total_rows", "n_clips", "cols", "out_rows", "pool_streams", "state_len", "block", "batch"):
        if key in case.counts:
            assert 0 < case.counts[key] < M.LIMIT31, (name, key)
    if name == "whisper_output_block":
        assert case.counts["n_clips"] <= 1048576  # SS_WHISPER_MAX_CLIPS
        assert case.counts["n_clips"] * -(-M.WHISPER_BLOCK["n_frames"] // 16) < 0xFFFFFFFF  # the 32-bit unit counter
    if name.startswith("pad_"):
        assert case.block("out").elems * case.block("out").elem_bytes < 2 ** 63
    if "cols" in case.counts and name.startswith(("splice", "add_deltas")):
        assert 3 * case.counts["cols"] < M.LIMIT31  # W * cols / (order + 1) * cols


@pytest.mark.parametrize("name", CASE_IDS)
def test_peak_device_memory_is_at_most_40_gib(name):
    case = M.CASES[name]
    assert case.peak_bytes <= M.CAP_BYTES, (name, case.peak_bytes / 2 ** 30)
    # the library's own share is part of that sum: the GPU file adds it to what torch reserved
    own = sum(b.bytes for b in case.blocks if b.name == "scratch") + (case.extra_bytes if not any(b.name == "scratch" for b in case.blocks) else 0)
    assert 0 <= case.library_bytes <= own, name


@pytest.mark.parametrize("name", [n for n in CASE_IDS if M.CASES[n].filler and "layout" in M.CASES[n].filler])
def test_the_filler_reaches_element_two_to_the_32_and_no_further_than_needed(name):
    case = M.CASES[name]
    lay, per = case.filler["layout"], case.filler["elems_per_filler"]
    assert lay.n_filler * per >= M.TWO32 > (lay.n_filler - 1) * per
    off = lay.offsets()
    assert off[0] == 0 and len(off) == lay.n_clips + 1 and np.all(np.diff(off) >= 0) and off[-1] == lay.total_rows
    assert np.all(np.diff(off[:lay.n_filler + 1]) == M.FILLER_ROWS)
    assert tuple(np.diff(off[lay.n_filler:])) == M.TAIL_ROWS and off[lay.n_filler] == lay.tail_row0
    assert tuple(np.diff(lay.small_offsets())) == M.TAIL_ROWS
    stressed = [b for b in case.blocks if b.role == "stress"]
    assert all(b.tail in (lay.tail_row0 * (b.elems // lay.total_rows), lay.n_filler * per) for b in stressed)


def test_the_resample_output_case():
    case = M.CASES["resample_output_side"]
    nf, per = case.filler["n_filler"], case.filler["elems_per_filler"]
    assert nf * per >= M.TWO32 > (nf - 1) * per and per == 2 * M.RESAMPLE_FILLER
    assert case.counts["filler_len"] < M.LIMIT31 and 2 * case.counts["filler_len"] < M.LIMIT31  # a clip is shorter than 2^31 in and out
    assert case.block("out").tail == 2 * case.block("x").tail  # 1 -> 2: out_len(L) = 2 L


def test_sample_side_tails():
    for name, (lens, eb) in M.SAMPLE_CASES.items():
        b = M.CASES[name].block("x")
        n = sum(lens)
        assert len(lens) == 5 and n <= M.N_TAIL
        assert b.elems == M.BIG and b.elem_bytes == eb and b.tail == M.sample_base(name) >= M.TWO32
        assert M.BIG - M.N_TAIL <= b.tail and b.tail + n <= M.BIG  # inside the seeded tail of the buffer
        assert name in M.SAMPLE_ALIGN or b.tail + n == M.BIG       # at the buffer's end
        assert ("i16" in name) == (eb == 2)
    assert M.sample_base("resample_stream") % 441 == 0
    # the lengths: the five of tests/test_packed_mel.py; those of tests/test_packed.py (a whole frame in the third clip); whole hops and periods
    assert M.FRAME_LENS == (16000, 12345, 640, 48000, 801)
    for lens, unit in ((M.HOP_LENS, 160), (M.MEL_HOP_LENS, 512), (M.PERIOD_LENS, 441)):
        assert all(h % unit == 0 and h <= n < h + unit for h, n in zip(lens, M.SAMPLE_LENS))
    assert M.sample_tail().shape == (M.N_TAIL,) and M.sample_tail_i16().dtype == np.int16
    out = M.CASES["resample_stream"].block("out")
    assert out.elems == M.BIG // 441 * 160 and out.tail == M.sample_base("resample_stream") // 441 * 160


def test_dense_strides_and_long_clips():
    for name in ("dense_kaldi_fbank", "dense_whisper", "dense_resample_in", "dense_resample_out"):
        b = M.CASES[name].block("wide")
        row = 2 * M.DENSE_ROW if name == "dense_resample_out" else M.DENSE_ROW
        assert b.elems == 2 * M.DENSE_LD + row and b.tail == 2 * M.DENSE_LD  # row 2 starts past element 2^33
        assert M.DENSE_LD % 2 == 0 and M.DENSE_LD > M.TWO32
    rows = -(-M.BIG // 39)
    assert M.LONG_ROWS == rows
    for stage in M.LONG_CLIP_STAGES:
        case = M.CASES["long_" + stage]
        assert case.counts["total_rows"] == rows and rows * 39 >= M.BIG
        out_rows = case.counts["out_rows"]
        assert out_rows == rows + (M.LONG_PAD_EXTRA if stage.startswith("pad") else 0)
        (a0, a1), (m0, m1), (e0, e1) = M.long_windows(out_rows, 39)
        assert (a0, a1) == (0, 64) and e1 == out_rows and e1 - e0 == 64 and m1 - m0 == 64
        assert m0 * 39 < M.TWO32 < m1 * 39 and m1 < rows  # the window holds the row with element 2^32, inside the clip
        assert all(b.tail == (M.TWO32 // 39 + 1) * (b.elems // (out_rows if b.name == "out" else rows)) for b in case.blocks)
    tile = M.long_tile(39)
    assert np.array_equal(M.tiled_rows(tile, 1000, 1100)[30], tile[6])  # row 1030 is tile row 6
    # select_rows on the long clip: the kept rows pass element 2^32 of out too, and kept row j is row j + j // 4095
    kept = M.long_select_kept()
    assert kept * 39 >= M.TWO32 + 64 * 39 and kept == sum(1 for r in range(rows % 4096)) + (rows // 4096) * 4095
    j = np.arange(0, 3 * 4095)
    r = M.long_select_source(j)
    assert np.array_equal(r, np.array([x for x in range(3 * 4096) if x % 4096 != 4095]))
    assert int(M.long_select_source(kept - 1)) == rows - 1 - (1 if (rows - 1) % 4096 == 4095 else 0)
    # the bct layout: column 38's run of max_rows elements holds element 2^32 of out
    mr = rows + M.LONG_PAD_EXTRA
    assert 38 * mr < M.TWO32 < 39 * mr and M.TWO32 - 38 * mr + 32 < rows


def test_tail_inputs_are_seeded_and_small():
    a, b = M.tail_rows_block(39), M.tail_rows_block(39)
    assert a.shape == (sum(M.TAIL_ROWS), 39) and a.dtype == np.float32 and np.array_equal(a, b)
    assert M.tail_rows_block(13).shape == (sum(M.TAIL_ROWS), 13)
    assert 0.05 < float(np.abs(a).mean()) < 0.12  # standard_normal * 0.1


def test_a_dense_resample_batch_ends_with_its_last_row_not_a_whole_stride_behind_it(sslib):
    """ss_resample* reject out overlapping x.  What a dense call touches is (batch - 1) * ld + n_samples floats of x and (batch - 1) *
    ld_out + out_len of out: a buffer that starts right behind the last row is not part of the batch, although it lies inside batch *
    ld.  The rule is decided before the device is looked for, so the host form shows it anywhere: SS_ERR_ARG (3) for an overlap,
    SS_OK or -- without a device -- SS_ERR_HIP (4) otherwise."""
    rs = C.c_void_p()
    assert sslib.ss_resampler_create(8000, 16000, 6, 0.99, C.byref(rs)) == 0
    try:
        B, n, out_len, wide = 3, 100, 200, 1000
        buf = np.zeros(8192, np.float32)
        at = lambda i: buf[i:].ctypes.data  # noqa: E731

        def call(x_at, ld, out_at, ld_out):
            return sslib.ss_resample(rs, at(x_at), B, n, ld, at(out_at), ld_out)

        x_span, out_span = (B - 1) * wide + n, (B - 1) * wide + out_len
        assert x_span < B * wide and out_span < B * wide
        # out right behind the last row of a strided x; x right behind the last row of a strided out
        assert call(0, wide, x_span, out_len) in (0, 4)
        assert call(out_span, n, 0, wide) in (0, 4)
        # genuine overlaps: out begins on the last sample of x; out lies in the gap between two rows of x; x begins on the last output
        assert call(0, wide, x_span - 1, out_len) == 3
        assert call(0, wide, n + 10, out_len) == 3
        assert call(out_span - 1, n, 0, wide) == 3
        assert call(0, n, 0, out_len) == 3  # in place
    finally:
        sslib.ss_resampler_destroy(rs)
