"""What tests/test_large_blocks_cpu.py and tests/test_large_blocks.py share: the shapes of the blocks past 2^32 elements and 2^32
samples, in plain Python and numpy, no device.  Every GPU case is one entry of CASES: the blocks it allocates (each in full), which
of them it stresses (the first element of the first tail clip lies at or past ELEMENT 2^32), which others it only carries past BYTE
2^32, and what it needs beside them (scratch, pools).  tests/test_large_blocks_cpu.py holds every entry to the conditions; the GPU
file takes its sizes from here and nowhere else.

Row side: a block is filler clips of FILLER_ROWS rows of zeros followed by the five tail clips of TAIL_ROWS rows.  Sample side: the
five clips of SAMPLE_LENS samples sit at the end of a buffer of BIG samples whose front is zeros.
"""
import numpy as np

TWO32 = 2 ** 32
LIMIT31 = 2 ** 31          # total_rows, n_clips, cols and every out-row count must stay below it (the header's rule)
BIG = 2 ** 32 + 2 ** 22    # elements or samples
CAP_BYTES = 40 * 2 ** 30   # peak device memory of one case
FILLER_ROWS = 8192
TAIL_ROWS = (1, 63, 700, 2049, 4100)          # 63 once caught the SpecAugment miscompile; 2049 crosses kCmvnSplitRows
SAMPLE_LENS = (16000, 12345, 1, 48000, 801)   # the clips of test_sample_offsets_past_two_to_the_31
FRAME_LENS = (16000, 12345, 640, 48000, 801)  # ... and of its twin for the frame paths, where a clip needs one whole frame
HOP_LENS = (16000, 12320, 0, 48000, 800)      # cut to whole hops of 160 (the pools take whole hops; no hop is legal)
MEL_HOP_LENS = (15872, 12288, 0, 47616, 512)  # ... of 512, the hop of the 2048-point mel configuration
PERIOD_LENS = (15876, 11907, 0, 47628, 441)   # ... to whole periods of 441 samples (44.1 kHz -> 16 kHz)
N_TAIL = 80000                                # seeded samples at the end of a sample block: at least every case's clips
TAIL_GROUPS = (0, 1, 0, 1, 0)
PAD_MAX_ROWS = 8192
WHISPER_BLOCK = dict(n_clips=11200, n_mels=128, n_frames=3000)
DENSE_LD = 2 ** 32 + 2
LONG_TILE = 1024           # rows of the seeded tile a long clip repeats
F32, BF16 = 4, 2


def ceil_div(a, b):
    return -(-a // b)


def fillers_for(elems_per_filler):
    """the fewest filler clips whose elements reach element 2^32"""
    return ceil_div(TWO32, elems_per_filler)


class Block:
    """One device allocation of a case: `elems` elements of `elem_bytes`, the first tail element at index `tail`.
    role: 'stress' (tail at or past element 2^32), 'bytes' (tail at or past byte 2^32) or 'small'."""

    def __init__(self, name, elems, elem_bytes, tail, role):
        self.name, self.elems, self.elem_bytes, self.tail, self.role = name, int(elems), int(elem_bytes), int(tail), role

    @property
    def bytes(self):
        return self.elems * self.elem_bytes

    @property
    def tail_byte(self):
        return self.tail * self.elem_bytes


class Case:
    """library_bytes: what of the peak the library allocates for itself (stream-ordered scratch), the rest being the test's tensors"""

    def __init__(self, name, blocks, counts, extra_bytes=0, filler=None, note="", library_bytes=0):
        self.name, self.blocks, self.counts, self.extra_bytes, self.filler, self.note = name, blocks, counts, int(extra_bytes), filler, note
        self.library_bytes = int(library_bytes)

    def block(self, name):
        return next(b for b in self.blocks if b.name == name)

    @property
    def peak_bytes(self):
        return sum(b.bytes for b in self.blocks) + self.extra_bytes


class RowLayout:
    """n_filler clips of FILLER_ROWS rows, then the tail clips"""

    def __init__(self, n_filler, tail_rows=TAIL_ROWS, filler_rows=FILLER_ROWS):
        self.n_filler, self.tail_rows, self.filler_rows = int(n_filler), tuple(tail_rows), int(filler_rows)
        self.n_clips = self.n_filler + len(self.tail_rows)
        self.tail_row0 = self.n_filler * self.filler_rows
        self.total_rows = self.tail_row0 + sum(self.tail_rows)

    def offsets(self):
        front = np.arange(self.n_filler + 1, dtype=np.int64) * self.filler_rows
        return np.concatenate([front, self.tail_row0 + np.cumsum(self.tail_rows, dtype=np.int64)])

    def small_offsets(self):
        return np.concatenate([[0], np.cumsum(self.tail_rows)]).astype(np.int64)


def tail_rows_block(cols, seed=2026):
    """the five tail clips' rows [sum(TAIL_ROWS), cols]: standard_normal * 0.1"""
    return (np.random.default_rng(seed + cols).standard_normal((sum(TAIL_ROWS), cols)) * 0.1).astype(np.float32)


def sample_tail(seed=7):
    """the last N_TAIL samples of the float sample block; a case's clips are its last sum(lens) samples"""
    return (np.random.default_rng(seed).standard_normal(N_TAIL) * 0.05).astype(np.float32)


def sample_tail_i16(seed=7):
    return np.random.default_rng(seed).integers(-32768, 32768, N_TAIL).astype(np.int16)


def long_tile(cols, seed=99):
    return (np.random.default_rng(seed + cols).standard_normal((LONG_TILE, cols)) * 0.1).astype(np.float32)


# ---- the cases ----

def _row_case(name, cols, out_cols, out_bytes=F32, extra=0, out_role="stress", in_role=None, note=""):
    """filler + tail rows of `cols` floats in, rows of `out_cols` elements out (0: no row-shaped output)"""
    widest = max(cols, out_cols)
    lay = RowLayout(fillers_for(FILLER_ROWS * widest))
    if in_role is None:
        in_role = "stress" if cols == widest else "bytes"
    blocks = [Block("in", lay.total_rows * cols, F32, lay.tail_row0 * cols, in_role)]
    if out_cols:
        blocks.append(Block("out", lay.total_rows * out_cols, out_bytes, lay.tail_row0 * out_cols, out_role if out_cols == widest else "bytes"))
    counts = dict(total_rows=lay.total_rows, n_clips=lay.n_clips, cols=cols, out_rows=lay.total_rows)
    return Case(name, blocks, counts, extra, dict(layout=lay, elems_per_filler=FILLER_ROWS * widest), note)


def _cases():
    c = {}
    L39 = RowLayout(fillers_for(FILLER_ROWS * 39))
    n39 = L39.total_rows * 39
    small_tables = 64 * L39.n_clips  # offset tables, group ids, spans, counts: well under a megabyte each; bounded here
    # section 2: one-shot packed calls, cols 39 in and out
    for name in ("cmvn", "cmvn_var", "cmvnw", "power_to_db", "cmvn_apply", "cmvn_grouped", "cmvn_grouped_global", "specaug", "mask_spans"):
        extra = small_tables + (L39.n_clips * 2 * 39 * 8 if "group" in name else 0)
        c[name] = _row_case(name, 39, 39, extra=extra)
    # the two-launch form: its scratch block is as large as the block, so vec and out are ONE allocation (out == vec; the first
    # launch has read all of vec into the scratch before the second writes out) -- three distinct blocks past 2^32 elements
    # would be 48 GiB
    cw = _row_case("cmvnw_var", 39, 0, extra=n39 * F32 + small_tables, note="in place: out == vec, scratch as large as the block")
    cw.blocks.append(Block("scratch", n39, F32, L39.tail_row0 * 39, "stress"))
    cw.extra_bytes = small_tables
    cw.library_bytes = n39 * F32  # the scratch block is the library's own
    c["cmvnw_var"] = cw
    c["specaug_inplace"] = _row_case("specaug_inplace", 39, 0, extra=small_tables)
    c["cmvn_stats"] = _row_case("cmvn_stats", 39, 0, extra=small_tables + L39.n_clips * 2 * 39 * 8)
    # one mask byte per row: a byte block cannot pass 2^32 below 2^31 rows -- it is neither stressed nor carried past byte 2^32
    vad = _row_case("vad_energy", 39, 0, extra=small_tables)
    vad.blocks.append(Block("mask", L39.total_rows, 1, L39.tail_row0, "small"))
    c["vad_energy"] = vad
    sel = _row_case("select_rows", 39, 39, extra=small_tables + 64 * L39.n_clips * 4)
    sel.blocks.append(Block("mask", L39.total_rows, 1, L39.tail_row0, "small"))
    c["select_rows"] = sel
    # the library's smaller scratch blocks (part of `extra` above): per-clip statistics, run counts, one key word per clip
    for name in ("cmvn_stats", "cmvn_grouped", "cmvn_grouped_global"):
        c[name].library_bytes = L39.n_clips * 2 * 39 * 8
    sel.library_bytes = 64 * L39.n_clips * 4
    c["power_to_db"].library_bytes = L39.n_clips * 4
    # the widening stages: cols 13 in, 39 out
    c["add_deltas"] = _row_case("add_deltas", 13, 39, extra=small_tables)
    c["splice"] = _row_case("splice", 13, 39, extra=small_tables)
    # pad: clip b's block starts at element b * max_rows * cols of out
    for layout in ("btc", "bct"):
        for dt, eb in (("float32", F32), ("bfloat16", BF16)):
            name = f"pad_{layout}_{dt}"
            lay = L39
            blocks = [Block("in", n39, F32, lay.tail_row0 * 39, "stress"),
                      Block("out", lay.n_clips * PAD_MAX_ROWS * 39, eb, lay.n_filler * PAD_MAX_ROWS * 39, "stress")]
            c[name] = Case(name, blocks, dict(total_rows=lay.total_rows, n_clips=lay.n_clips, cols=39, out_rows=PAD_MAX_ROWS),
                           small_tables, dict(layout=lay, elems_per_filler=PAD_MAX_ROWS * 39))
    # section 3: pool calls from fresh streams; every entry owns its own slot of a zeroed pool
    def pool_case(name, cols, out_cols, state_len):
        k = _row_case(name, cols, out_cols)
        lay = k.filler["layout"]
        k.extra_bytes = small_tables + lay.n_clips * state_len * F32
        k.counts["pool_streams"] = lay.n_clips
        k.counts["state_len"] = state_len
        return k
    c["cmvn_stream"] = pool_case("cmvn_stream", 39, 39, (CMVN_STREAM_WIN - 1) * 39 + 1)
    c["add_deltas_stream"] = pool_case("add_deltas_stream", 13, 39, 2 * 4 * 13 + 1)
    c["splice_stream"] = pool_case("splice_stream", 13, 39, 2 * 13 + 1)
    vs = pool_case("vad_energy_stream", 39, 0, 2 * VAD_CONTEXT + 4)
    vs.blocks.append(Block("mask", L39.total_rows, 1, L39.tail_row0, "small"))
    c["vad_energy_stream"] = vs
    # section 4: the sample side.  Outputs stay compact (a few thousand rows): `extra` bounds them at 64 MiB
    n_tail = sum(SAMPLE_LENS)
    for name, (lens, eb) in SAMPLE_CASES.items():
        c[name] = Case(name, [Block("x", BIG, eb, sample_base(name), "stress")], dict(n_clips=len(lens)), 64 * 2 ** 20)
    # the resample pool writes entry i's outputs at so[i] / o * n of out [total_in / o * n]: the output block follows the input's offsets
    o, n = RESAMPLE_STREAM_RATIO
    c["resample_stream"].blocks.append(Block("out", BIG // o * n, F32, sample_base("resample_stream") // o * n, "bytes"))
    w = WHISPER_BLOCK
    blk = w["n_mels"] * w["n_frames"]
    c["whisper_output_block"] = Case("whisper_output_block", [Block("out", w["n_clips"] * blk, F32, (w["n_clips"] - 5) * blk, "stress")],
                                     dict(n_clips=w["n_clips"], block=blk), w["n_clips"] * blk + 64 * 2 ** 20,
                                     note="extra: the one-byte-per-element mask of the device-side comparison")
    # resample, output side: filler clips of RESAMPLE_FILLER samples in front push oo of the tail past 2^32 (1/2: two outputs
    # per sample, so the input passes byte 2^32 and sample 2^31)
    nf = fillers_for(2 * RESAMPLE_FILLER)
    c["resample_output_side"] = Case("resample_output_side",
                                     [Block("x", nf * RESAMPLE_FILLER + n_tail, F32, nf * RESAMPLE_FILLER, "bytes"),
                                      Block("out", 2 * (nf * RESAMPLE_FILLER + n_tail), F32, 2 * nf * RESAMPLE_FILLER, "stress")],
                                     dict(n_clips=nf + 5, filler_len=RESAMPLE_FILLER), 64 * 2 ** 20,
                                     dict(n_filler=nf, elems_per_filler=2 * RESAMPLE_FILLER))
    # section 5: three rows at a stride of 2^32 + 2
    for name in ("dense_kaldi_fbank", "dense_whisper", "dense_resample_in", "dense_resample_out"):
        row = 2 * DENSE_ROW if name == "dense_resample_out" else DENSE_ROW  # 1 -> 2: the out rows are twice as long
        c[name] = Case(name, [Block("wide", 2 * DENSE_LD + row, F32, 2 * DENSE_LD, "stress")], dict(batch=3), 64 * 2 ** 20)
    # section 6: one clip of ceil(BIG / 39) rows
    # (`tail` of a long clip's block: the first row that lies wholly past element 2^32 of the widest block, inside the clip)
    rows = LONG_ROWS
    mid = TWO32 // 39 + 1
    for name in LONG_CLIP_STAGES:
        cols = 13 if name in ("splice", "add_deltas") else 39
        out_rows = rows + LONG_PAD_EXTRA if name.startswith("pad") else rows
        blocks = [Block("in", rows * cols, F32, mid * cols, "stress" if cols == 39 else "bytes")]
        if name != "specaug_inplace":
            blocks.append(Block("out", out_rows * 39, F32, mid * 39, "stress"))
        if name == "select_rows":
            blocks.append(Block("mask", rows, 1, mid, "small"))
        c["long_" + name] = Case("long_" + name, blocks, dict(total_rows=rows, n_clips=1, cols=cols, out_rows=out_rows), 2 ** 20,
                                 note="stress: the row that holds element 2^32 lies inside the clip")
    return c


CMVN_STREAM_WIN = 5
VAD_CONTEXT = 2
RESAMPLE_FILLER = 2 ** 20
DENSE_ROW = 48000
RESAMPLE_STREAM_RATIO = (441, 160)
# the sample side: case -> (clip lengths, bytes per sample).  The frame paths give a clip shorter than a frame no row and refuse it
# (SS_ERR_SHORT_SIGNAL): they take FRAME_LENS, the clips of tests/test_packed.py; the pools take whole hops or periods.
SAMPLE_CASES = {
    "kaldi_fbank": (FRAME_LENS, F32), "kaldi_mfcc": (FRAME_LENS, F32), "lmfe": (FRAME_LENS, F32), "mfcc": (FRAME_LENS, F32),
    "mfcc_i16": (FRAME_LENS, 2), "mfe_i16": (FRAME_LENS, 2),
    "whisper_f32": (SAMPLE_LENS, F32), "whisper_bf16": (SAMPLE_LENS, F32),
    "resample_441_160": (SAMPLE_LENS, F32), "resample_1_2": (SAMPLE_LENS, F32),
    "resample_i16_441_160": (SAMPLE_LENS, 2), "resample_i16_1_2": (SAMPLE_LENS, 2),
    "log_mel_cfg3": (SAMPLE_LENS, F32), "log_mel_chirpz400": (SAMPLE_LENS, F32), "mel": (SAMPLE_LENS, F32), "stft": (SAMPLE_LENS, F32),
    "mel_i16": (SAMPLE_LENS, 2), "stft_i16": (SAMPLE_LENS, 2),
    "kstream_fbank": (HOP_LENS, F32), "kstream_fbank_i16": (HOP_LENS, 2), "mfcc_stream": (HOP_LENS, F32),
    "mel_stream": (MEL_HOP_LENS, F32), "resample_stream": (PERIOD_LENS, F32),
}
SAMPLE_ALIGN = {"resample_stream": 441}  # the resample pool takes entries that start on a whole period of the buffer


def sample_base(name):
    """the first sample of the first tail clip of a sample-side case: the clips end at the buffer's end (or as near as the case's
    alignment allows)"""
    lens, _ = SAMPLE_CASES[name]
    a = SAMPLE_ALIGN.get(name, 1)
    return (BIG - sum(lens)) // a * a


LONG_ROWS = ceil_div(BIG, 39)  # one clip whose own element count passes 2^32
LONG_PAD_EXTRA = 3             # pad rows behind the long clip: max_rows = LONG_ROWS + 3
LONG_SELECT_PERIOD = 4096      # the long clip's mask drops one row in 4096: the kept rows still pass element 2^32
# the stages that got the long clip: those whose call on one clip of 2^28 elements, times sixteen, stays under five seconds
LONG_CLIP_STAGES = ("specaug", "mask_spans", "power_to_db", "select_rows", "pad_btc", "pad_bct", "splice", "add_deltas", "specaug_inplace")
CASES = _cases()


# ---- what the stages give on a block of zeros and near a position of a tiled long clip ----

def tiled_rows(tile, lo, hi):
    """rows lo .. hi of the clip that repeats `tile`"""
    return tile[np.arange(lo, hi) % len(tile)]


def long_select_kept(rows=None):
    """rows the long clip's mask keeps: row r is dropped iff r % LONG_SELECT_PERIOD == LONG_SELECT_PERIOD - 1"""
    rows = LONG_ROWS if rows is None else rows
    return rows - rows // LONG_SELECT_PERIOD


def long_select_source(j):
    """the clip's row that becomes kept row j"""
    j = np.asarray(j, np.int64)
    return j + j // (LONG_SELECT_PERIOD - 1)


def long_windows(rows, cols):
    """the three windows of 64 rows: the clip's start, across the row that holds element 2^32, its end"""
    mid = TWO32 // cols
    return ((0, 64), (mid - 32, mid + 32), (rows - 64, rows))
