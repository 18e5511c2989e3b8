"""The fused log-mel calls (ss_log_mel_spectrogram*) on the device.

The bar in every test is torch.equal against the two-step path on the same input: the existing ss_mel_spectrogram*_device call, then
ss_power_to_db_packed_device over its result with every clip as its own segment (cols = num_filters, offsets = the row offsets) and
the same ref / amin / top_db.  Each test also asserts what ss_last_kernel_name() reports: a dB build carries `db` in its template
list, the composed path (a mel kernel without a dB build + the in-place pass) reports the mel kernel's name + "+db".

Inputs: 0.1-amplitude noise clips, one all-zero clip and one clip that is a single loud tone (0.9 at 1 kHz), all exactly
representable as int16 * 2^-15 so that the float and the int16 forms see the same samples.

(ref, amin, top_db) cases: (1, 1e-10, None), (1, 1e-10, 80), (0.25, 1e-3, 20) -- and (1, 1e-10, 20), added for the assertion that the
floor bites.  With amin = 1e-3 it cannot: the mel values of these shapes are small -- on the CPU oracle the noise clips peak at
1.4e-5 (cfg3) and 7e-5 (512 points), below amin, so every element of such a clip is the same number, and the tone peaks at 0.019
(cfg3) .. 0.092 (512 points, hop 256), 12.8 .. 19.6 dB above amin, inside a 20 dB floor; no input within [-1, 1] -- the range of
int16 * 2^-15 -- changes that.  With amin = 1e-10 and top_db = 20 the oracle's share of elements at the floor is 0.12 / 0.31
(cfg3 noise clips of 16500 / 5000 samples), 0.99 (cfg3 tone), 0.12 (512-point noise) and 0.93 (400 / 512-point tones): strictly
between 0 and 1, which is what _assert_floor_bites checks on the device result.
"""
import contextlib
import ctypes as C

import numpy as np
import pytest

from common import CONFIGS

CFG3 = dict(CONFIGS["cfg3"])
MEL512 = dict(fft_points=512, frame_length=0.01, frame_stride=0.005)  # the 512-point mel kernel's shape (ss_mel_c256)
CHIRPZ400 = dict(fft_points=400, frame_length=0.01)
HOP256 = dict(fft_points=512, frame_length=0.016)
PCM_SCALE = 2.0 ** -15
DB_CASES = [(1.0, 1e-10, None), (1.0, 1e-10, 80.0), (0.25, 1e-3, 20.0), (1.0, 1e-10, 20.0)]
DB_IDS = ["nofloor", "top80", "ref.25_amin1e-3_top20", "top20"]
BITES = (1.0, 1e-10, 20.0)  # the case in which the floor clamps part of the tone clip and of a long noise clip (module docstring)
PACKED_LENS = [700, 2048, 5000, 16000, 16500]  # rows 2, 4, 10, 32, 33: odd and even counts, a clip shorter than a window, straddling pairs
PACKED_KINDS = ["noise", "zero", "noise", "tone", "noise"]


def _td(top_db):
    return -1.0 if top_db is None else float(top_db)


def _clip(kind, n, seed, sr=16000):
    if kind == "zero":
        x = np.zeros(n)
    elif kind == "tone":
        x = 0.9 * np.sin(2 * np.pi * 1000.0 * np.arange(n) / sr)
    else:
        x = np.random.default_rng(seed).standard_normal(n) * 0.1
    return np.clip(np.round(x * 32768.0), -32768, 32767).astype(np.int16)


def _pcm(torch, kinds, lengths):
    """The clips as one packed int16 device tensor."""
    return torch.from_numpy(np.concatenate([_clip(k, n, 100 + i) for i, (k, n) in enumerate(zip(kinds, lengths))])).cuda()


def _inputs(torch, pcm, fmt):
    """(device tensor, trailing scale arguments, entry-point infix) of the fused call; the two-step path always takes the floats."""
    return (pcm, [PCM_SCALE], "_i16") if fmt == "i16" else (pcm.float() * PCM_SCALE, [], "")


def _cfg(ss, **kw):
    from speechsauce_amd import _lib

    return ss.SpeechConfig(_lib.make_params(**kw))


def _offsets(ss, cfg, lens):
    so = ss._sample_offsets(np.asarray(lens, dtype=np.int64), int(sum(lens)), "t")
    return so, ss._row_offsets(cfg, so)


def _blocks(flat, ro, M):
    return [flat[M * int(ro[b]):M * int(ro[b + 1])] for b in range(len(ro) - 1)]


def _assert_floor_bites(blocks, top_db, which):
    """The share of elements equal to their clip's floor (max - top_db, formed in f32 as the floor pass forms it) is strictly between
    0 and 1 for the clips `which`."""
    for b in which:
        blk = blocks[b].cpu().numpy()
        floor = np.float32(blk.max()) - np.float32(top_db)
        share = float(np.mean(blk == floor))
        print(f"clip {b}: share at the floor {share:.3f}")
        assert 0.0 < share < 1.0, (b, share)
        assert blk.min() == floor


# ---- the two paths -------------------------------------------------------------------------------------------------------------

def _two_step_packed(torch, lib, cfg, xf, n, dso, dro, rows, db):
    M = cfg.params.num_filters
    mel = torch.full((M * rows,), float("nan"), device="cuda")
    assert lib.ss_mel_spectrogram_packed_device(cfg.handle, xf.data_ptr(), n, dso.data_ptr(), dro.data_ptr(), rows, mel.data_ptr(), None) == 0
    name = lib.ss_last_kernel_name()
    out = torch.full_like(mel, float("nan"))
    assert lib.ss_power_to_db_packed_device(mel.data_ptr(), n, dro.data_ptr(), rows, M, db[0], db[1], _td(db[2]), out.data_ptr(), None) == 0
    torch.cuda.synchronize()
    return out, name


def _fused_packed(torch, lib, cfg, x, sc, infix, n, dso, dro, rows, db, out=None, stream=None):
    M = cfg.params.num_filters
    if out is None:
        out = torch.full((M * rows,), float("nan"), device="cuda")
    rc = getattr(lib, f"ss_log_mel_spectrogram_packed{infix}_device")(cfg.handle, x.data_ptr(), n, dso.data_ptr(), *sc, dro.data_ptr(), rows,
                                                                     db[0], db[1], _td(db[2]), out.data_ptr(), stream)
    assert rc == 0, lib.ss_last_error_string()
    return out


def _two_step_dense(torch, lib, cfg, xf, ch, L, db):
    M = cfg.params.num_filters
    R, _ = cfg.stft_rows(L)
    mel = torch.full((ch, M, R), float("nan"), device="cuda")
    assert lib.ss_mel_spectrogram_device(cfg.handle, xf.data_ptr(), ch, L, L, mel.data_ptr(), None) == 0
    name = lib.ss_last_kernel_name()
    table = (torch.arange(ch + 1, dtype=torch.int64) * R).cuda()  # every clip its own segment
    out = torch.full_like(mel, float("nan"))
    assert lib.ss_power_to_db_packed_device(mel.data_ptr(), ch, table.data_ptr(), ch * R, M, db[0], db[1], _td(db[2]), out.data_ptr(), None) == 0
    torch.cuda.synchronize()
    return out, name


def _fused_dense(torch, lib, cfg, x, sc, infix, ch, L, db, stream=None):
    M = cfg.params.num_filters
    R, _ = cfg.stft_rows(L)
    out = torch.full((ch, M, R), float("nan"), device="cuda")
    rc = getattr(lib, f"ss_log_mel_spectrogram{infix}_device")(cfg.handle, x.data_ptr(), ch, L, L, *sc, db[0], db[1], _td(db[2]), out.data_ptr(),
                                                              stream)
    assert rc == 0, lib.ss_last_error_string()
    return out


_REFERENCE = {}  # (test key, db) -> the two-step result, computed once and shared by the float and the int16 case


def _reference(key, make):
    if key not in _REFERENCE:
        _REFERENCE[key] = make()
    return _REFERENCE[key]


# ---- packed, twelve-wave build ---------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("fmt", ["f32", "i16"])
@pytest.mark.parametrize("db", DB_CASES, ids=DB_IDS)
def test_packed_twelve_wave_build(ss, sslib, db, fmt):
    import torch

    cfg = _cfg(ss, **CFG3)
    M = cfg.params.num_filters
    so, ro = _offsets(ss, cfg, PACKED_LENS)
    assert np.diff(ro).tolist() == [2, 4, 10, 32, 33]
    dso, dro = torch.from_numpy(so).cuda(), torch.from_numpy(ro).cuda()
    rows, n = int(ro[-1]), len(PACKED_LENS)
    pcm = _pcm(torch, PACKED_KINDS, PACKED_LENS)
    want, mel_name = _reference(("packed12", db), lambda: _two_step_packed(torch, sslib, cfg, pcm.float() * PCM_SCALE, n, dso, dro, rows, db))
    assert mel_name == b"ss_mel_c1024v<w12,mel6321>"
    x, sc, infix = _inputs(torch, pcm, fmt)
    got = _fused_packed(torch, sslib, cfg, x, sc, infix, n, dso, dro, rows, db)
    torch.cuda.synchronize()
    name = sslib.ss_last_kernel_name()
    assert name == (b"ss_mel_c1024vi<w12,mel6321,db>" if fmt == "i16" else b"ss_mel_c1024v<w12,mel6321,db>"), name
    cfg.device_status()
    assert not torch.isnan(got).any()
    assert torch.equal(got, want)
    if db == BITES:
        _assert_floor_bites(_blocks(got, ro, M), db[2], (3, 4))


# ---- dense, twelve-wave build ----------------------------------------------------------------------------------------------------

DENSE12 = (144, 16500)  # 144 clips x 17 row pairs = 2448 units > 2048: the parent's own rule picks the twelve-wave build (asserted)


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", ["f32", "i16"])
@pytest.mark.parametrize("db", DB_CASES, ids=DB_IDS)
def test_dense_twelve_wave_build(ss, sslib, db, fmt):
    import torch

    ch, L = DENSE12
    cfg = _cfg(ss, **CFG3)
    M = cfg.params.num_filters
    R, _ = cfg.stft_rows(L)
    assert R == 33  # the last pair of every clip is half real
    pcm = _reference("dense12_pcm", lambda: _pcm(torch, ["zero", "tone"] + ["noise"] * (ch - 2), [L] * ch))
    want, mel_name = _reference(("dense12", db), lambda: _two_step_dense(torch, sslib, cfg, pcm.float() * PCM_SCALE, ch, L, db))
    assert mel_name == b"ss_mel_c1024<w12,mel6321>"  # the smallest batch idea rests on this: asserted, not assumed
    x, sc, infix = _inputs(torch, pcm, fmt)
    got = _fused_dense(torch, sslib, cfg, x, sc, infix, ch, L, db)
    torch.cuda.synchronize()
    name = sslib.ss_last_kernel_name()
    assert name == (b"ss_mel_c1024i<w12,mel6321,db>" if fmt == "i16" else b"ss_mel_c1024<w12,mel6321,db>"), name
    assert not torch.isnan(got).any()
    assert torch.equal(got, want)
    if db == BITES:
        _assert_floor_bites([got[b].reshape(-1) for b in range(ch)], db[2], (1, 2, ch - 1))


# ---- composed path: a mel kernel without a dB build, then the in-place pass ----------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("fmt", ["f32", "i16"])
@pytest.mark.parametrize("shape", ["cfg3_eight_waves", "mel512"])
@pytest.mark.parametrize("db", DB_CASES, ids=DB_IDS)
def test_composed_path(ss, sslib, db, shape, fmt):
    import torch

    kw, L, mel_kernel = (CFG3, 16500, b"ss_mel_c1024") if shape == "cfg3_eight_waves" else (MEL512, 16000, b"ss_mel_c256")
    ch = 4
    cfg = _cfg(ss, **kw)
    pcm = _pcm(torch, ["noise", "zero", "tone", "noise"], [L] * ch)
    want, mel_name = _reference((shape, db), lambda: _two_step_dense(torch, sslib, cfg, pcm.float() * PCM_SCALE, ch, L, db))
    assert mel_name == mel_kernel
    x, sc, infix = _inputs(torch, pcm, fmt)
    got = _fused_dense(torch, sslib, cfg, x, sc, infix, ch, L, db)
    torch.cuda.synchronize()
    name = sslib.ss_last_kernel_name()
    assert name == mel_kernel + b"+db" and name.endswith(b"+db"), name
    assert torch.equal(got, want)
    if db == BITES:
        _assert_floor_bites([got[b].reshape(-1) for b in range(ch)], db[2], (2, 3))


# ---- generic kernel ----------------------------------------------------------------------------------------------------------------

@contextlib.contextmanager
def _generic_library(sslib, sslab, forced):
    """The library a generic-kernel case runs on: the product library where the call runs the generic kernel by itself, the lab
    library with ss_debug_force_generic where a dedicated kernel would take it (the dense 512-point shape)."""
    from speechsauce_amd import _lib

    if not forced:
        yield sslib
        return
    with _lib.use_library(sslab):
        sslab.ss_debug_force_generic(1)
        try:
            yield sslab
        finally:
            sslab.ss_debug_force_generic(0)


GENERIC = {"chirpz400": (CHIRPZ400, b"10,chirpz", 400), "512_hop256": (HOP256, b"8", 512)}


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", ["f32", "i16"])
@pytest.mark.parametrize("case", list(GENERIC))
@pytest.mark.parametrize("db", DB_CASES, ids=DB_IDS)
def test_generic_kernel_packed(ss, sslib, sslab, db, case, fmt):
    import torch

    kw, tl, W = GENERIC[case]
    lens, kinds = [W - 100, 3000, 4000], ["noise", "tone", "noise"]  # three clips, the first shorter than the window
    with _generic_library(sslib, sslab, False) as lib:
        cfg = _cfg(ss, **kw)
        M = cfg.params.num_filters
        so, ro = _offsets(ss, cfg, lens)
        dso, dro = torch.from_numpy(so).cuda(), torch.from_numpy(ro).cuda()
        rows = int(ro[-1])
        pcm = _pcm(torch, kinds, lens)
        want, mel_name = _reference(("gp", case, db), lambda: _two_step_packed(torch, lib, cfg, pcm.float() * PCM_SCALE, 3, dso, dro, rows, db))
        assert mel_name == b"ss_front_generic_varrows<" + tl + b">", mel_name
        x, sc, infix = _inputs(torch, pcm, fmt)
        got = _fused_packed(torch, lib, cfg, x, sc, infix, 3, dso, dro, rows, db)
        torch.cuda.synchronize()
        name = lib.ss_last_kernel_name()
        assert name == b"ss_front_generic_varrows" + (b"i" if fmt == "i16" else b"") + b"<" + tl + b",db>", name
        cfg.device_status()
    assert torch.equal(got, want)
    if db == BITES:
        _assert_floor_bites(_blocks(got, ro, M), db[2], (1, 2))


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", ["f32", "i16"])
@pytest.mark.parametrize("L", [4000, 300], ids=["L4000", "shorter_than_the_window"])
@pytest.mark.parametrize("case", list(GENERIC))
@pytest.mark.parametrize("db", DB_CASES, ids=DB_IDS)
def test_generic_kernel_dense(ss, sslib, sslab, db, case, L, fmt):
    import torch

    kw, tl, W = GENERIC[case]
    ch = 3
    with _generic_library(sslib, sslab, case == "512_hop256") as lib:  # (the dense 512-point call has a dedicated kernel: forced)
        cfg = _cfg(ss, **kw)
        pcm = _pcm(torch, ["noise", "zero", "tone"], [L] * ch)
        want, mel_name = _reference(("gd", case, L, db), lambda: _two_step_dense(torch, lib, cfg, pcm.float() * PCM_SCALE, ch, L, db))
        assert mel_name == b"ss_front_generic<" + tl + b">", mel_name
        x, sc, infix = _inputs(torch, pcm, fmt)
        got = _fused_dense(torch, lib, cfg, x, sc, infix, ch, L, db)
        torch.cuda.synchronize()
        name = lib.ss_last_kernel_name()
        assert name == b"ss_front_generic" + (b"_i16" if fmt == "i16" else b"") + b"<" + tl + b",db>", name
    assert torch.equal(got, want)
    if db == BITES and L == 4000:
        _assert_floor_bites([got[b].reshape(-1) for b in range(ch)], db[2], (0, 2))


# ---- position independence --------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("kernel", ["twelve_wave", "generic"])
@pytest.mark.parametrize("db", DB_CASES[1:], ids=DB_IDS[1:])
def test_packed_blocks_do_not_depend_on_position(ss, sslib, sslab, db, kernel):
    import torch

    from speechsauce_amd import _lib

    kw = CFG3 if kernel == "twelve_wave" else CHIRPZ400
    lens = PACKED_LENS if kernel == "twelve_wave" else [300, 3000, 4000, 1234, 160]
    cfg = _cfg(ss, **kw)
    M = cfg.params.num_filters
    clips = [_clip(k, n, 200 + i) for i, (k, n) in enumerate(zip(PACKED_KINDS, lens))]

    def run(order):
        ls = [lens[i] for i in order]
        so, ro = _offsets(ss, cfg, ls)
        x = torch.from_numpy(np.concatenate([clips[i] for i in order])).cuda().float() * PCM_SCALE
        out = _fused_packed(torch, sslib, cfg, x, [], "", len(ls), torch.from_numpy(so).cuda(), torch.from_numpy(ro).cuda(), int(ro[-1]), db)
        torch.cuda.synchronize()
        return dict(zip(order, _blocks(out, ro, M)))

    base = run([0, 1, 2, 3, 4])
    perm = run([3, 0, 4, 2, 1])
    for b in range(5):
        assert torch.equal(base[b], perm[b]), b
    # a clip's block is the dense call on that clip alone, on the same kernel family (the twelve-wave build is forced for the one-clip
    # dense call: its own rule would pick eight waves, which round a few FMAs differently)
    with _lib.use_library(sslab):
        sslab.ss_debug_mel_tile(3)
        try:
            lcfg = _cfg(ss, **kw)
            for b in range(5):
                x = torch.from_numpy(clips[b]).cuda().float() * PCM_SCALE
                alone = _fused_dense(torch, sslab, lcfg, x, [], "", 1, lens[b], db)
                torch.cuda.synchronize()
                name = sslab.ss_last_kernel_name()
                assert name == (b"ss_mel_c1024<w12,mel6321,db>" if kernel == "twelve_wave" else b"ss_front_generic<10,chirpz,db>"), name
                assert torch.equal(alone.reshape(-1), base[b]), b
        finally:
            sslab.ss_debug_mel_tile(0)


# ---- launches ----------------------------------------------------------------------------------------------------------------------

def _hip_runtime():
    """The HIP runtime this process has loaded (torch's), for the stream-capture calls the graph-shape check needs."""
    with open("/proc/self/maps") as f:
        paths = {line.split()[-1] for line in f if "libamdhip64" in line}
    assert paths, "no HIP runtime loaded"
    return C.CDLL(sorted(paths)[0])


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["packed12", "dense12", "packed_generic", "dense_generic"])
def test_without_a_floor_the_call_is_one_launch(ss, sslib, layout):
    """top_db = None: the captured device form is ONE kernel node, no memory nodes, no edges."""
    import torch

    db = (1.0, 1e-10, None)
    packed = layout.startswith("packed")
    cfg = _cfg(ss, **(CFG3 if layout.endswith("12") else CHIRPZ400))
    if packed:
        lens = PACKED_LENS
        so, ro = _offsets(ss, cfg, lens)
        dso, dro = torch.from_numpy(so).cuda(), torch.from_numpy(ro).cuda()
        x = _pcm(torch, PACKED_KINDS, lens).float() * PCM_SCALE
        out = torch.empty((cfg.params.num_filters * int(ro[-1]),), device="cuda")
        call = lambda st: _fused_packed(torch, sslib, cfg, x, [], "", len(lens), dso, dro, int(ro[-1]), db, out=out, stream=st)
    else:
        ch, L = DENSE12 if layout == "dense12" else (3, 4000)
        x = _pcm(torch, ["noise"] * ch, [L] * ch).float() * PCM_SCALE
        call = lambda st: _fused_dense(torch, sslib, cfg, x, [], "", ch, L, db, stream=st)
    call(None)  # warm-up outside the capture
    torch.cuda.synchronize()
    assert b",db>" in sslib.ss_last_kernel_name()
    hip = _hip_runtime()
    raw, graph = torch.cuda.Stream(), C.c_void_p()
    assert hip.hipStreamBeginCapture(C.c_void_p(raw.cuda_stream), 2) == 0  # hipStreamCaptureModeRelaxed
    call(C.c_void_p(raw.cuda_stream))
    assert hip.hipStreamEndCapture(C.c_void_p(raw.cuda_stream), C.byref(graph)) == 0
    n_nodes, n_edges = C.c_size_t(), C.c_size_t()
    assert hip.hipGraphGetNodes(graph, None, C.byref(n_nodes)) == 0
    assert hip.hipGraphGetEdges(graph, None, None, C.byref(n_edges)) == 0
    assert hip.hipGraphDestroy(graph) == 0
    assert (n_nodes.value, n_edges.value) == (1, 0)


@pytest.mark.gpu
def test_graph_of_the_floored_packed_call_replays_on_new_input(ss, sslib):
    import torch

    db = (1.0, 1e-10, 80.0)
    lens = [16000, 7777, 640, 32001, 20000, 1]
    n = int(sum(lens))
    cfg = _cfg(ss, **CFG3)
    so, ro = _offsets(ss, cfg, lens)
    dso, dro = torch.from_numpy(so).cuda(), torch.from_numpy(ro).cuda()
    rows = int(ro[-1])

    def signal(seed):
        g = torch.Generator(device="cuda")
        g.manual_seed(seed)
        return torch.randn(n, generator=g, device="cuda", dtype=torch.float32).mul_(0.05)

    x = signal(9)
    out = torch.empty((rows * cfg.params.num_filters,), device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):  # warm-up off the capture
        _fused_packed(torch, sslib, cfg, x, [], "", len(lens), dso, dro, rows, db, out=out, stream=C.c_void_p(s.cuda_stream))
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        _fused_packed(torch, sslib, cfg, x, [], "", len(lens), dso, dro, rows, db, out=out,
                      stream=C.c_void_p(torch.cuda.current_stream().cuda_stream))
    for seed in (21, 22):
        x.copy_(signal(seed))
        g.replay()
        torch.cuda.synchronize()
        eager = _fused_packed(torch, sslib, cfg, x, [], "", len(lens), dso, dro, rows, db)
        want, _ = _two_step_packed(torch, sslib, cfg, x, len(lens), dso, dro, rows, db)
        assert torch.equal(out, eager) and torch.equal(out, want)
    cfg.device_status()


# ---- bad device row offsets ----------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("kw", [CFG3, HOP256], ids=["twelve_wave", "generic"])
def test_bad_row_offsets_raise_the_error_word_and_touch_nothing_else(ss, sslib, kw):
    """One clip's ro entry is wrong: the existing error-word protocol -- SS_ERR_DEVICE from the call's next status, nothing written
    outside d_out, the skipped clip's rows left alone by the launch AND by the floor pass, the other clips as in the two-step path."""
    import torch

    db = (1.0, 1e-10, 80.0)
    lens = [16000, 8000, 4000, 12000]
    cfg = _cfg(ss, **kw)  # a fresh config: its error word is its own
    M = cfg.params.num_filters
    so, ro = _offsets(ss, cfg, lens)
    rows = int(ro[-1])
    dso, dro = torch.from_numpy(so).cuda(), torch.from_numpy(ro).cuda()
    x = _pcm(torch, ["noise", "tone", "noise", "noise"], lens).float() * PCM_SCALE
    good, _ = _two_step_packed(torch, sslib, cfg, x, 4, dso, dro, rows, db)
    assert sslib.ss_config_device_status(cfg.handle) == 0
    good = good.cpu().numpy()
    bad = ro.copy()
    bad[2:] += 1  # clip 1 claims one row too many; the clips behind it start one row late but are consistent in themselves
    total, pad = int(bad[-1]), 4096
    block = torch.full((M * total + 2 * pad,), float("nan"), device="cuda")  # (NaN: a floor pass over it would not leave it NaN)
    dbad = torch.from_numpy(bad).cuda()
    _fused_packed(torch, sslib, cfg, x, [], "", 4, dso, dbad, total, db, out=block[pad:])  # rc == 0: the check is the kernel's
    torch.cuda.synchronize()
    assert sslib.ss_config_device_status(cfg.handle) == 6  # SS_ERR_DEVICE, read and cleared
    assert sslib.ss_config_device_status(cfg.handle) == 0
    blk = block.cpu().numpy()
    assert np.isnan(blk[:pad]).all() and np.isnan(blk[-pad:]).all()
    body = blk[pad:-pad]
    assert np.array_equal(body[:M * ro[1]], good[:M * ro[1]])  # clip 0
    assert np.isnan(body[M * bad[1]:M * bad[2]]).all()  # clip 1: skipped by the launch and by the floor pass
    for b in (2, 3):  # one row later, the same bits
        assert np.array_equal(body[M * bad[b]:M * bad[b + 1]], good[M * ro[b]:M * ro[b + 1]]), b


# ---- host, list and Python forms -----------------------------------------------------------------------------------------------------

def _front_kw(kw):
    m = dict(frame_length=kw.get("frame_length", 0.02), frame_stride=kw.get("frame_stride", 0.01), num_filters=kw.get("num_filters", 40),
             fft_length=kw.get("fft_points", 512))
    if "high_frequency" in kw:
        m["high_frequency"] = kw["high_frequency"]
    return m


@pytest.mark.gpu
@pytest.mark.parametrize("kw", [CFG3, CHIRPZ400], ids=["cfg3", "chirpz400"])
@pytest.mark.parametrize("db", DB_CASES, ids=DB_IDS)
def test_host_list_and_python_forms_equal_the_device_form(ss, sslib, db, kw):
    import torch

    ref, amin, top_db = db
    fkw = dict(_front_kw(kw), ref=ref, amin=amin, top_db=top_db)
    cfg = _cfg(ss, **kw)
    M = cfg.params.num_filters
    lens = PACKED_LENS
    so, ro = _offsets(ss, cfg, lens)
    dso, dro = torch.from_numpy(so).cuda(), torch.from_numpy(ro).cuda()
    pcm = _pcm(torch, PACKED_KINDS, lens)
    xf = pcm.float() * PCM_SCALE
    dev = _fused_packed(torch, sslib, cfg, xf, [], "", len(lens), dso, dro, int(ro[-1]), db)
    torch.cuda.synchronize()
    # packed: Python on the device, on the host (float and int16), and the list form
    out_d, ro_d = ss.log_mel_spectrogram_packed(xf, lens, 16000, **fkw)
    out_h, ro_h = ss.log_mel_spectrogram_packed(xf.cpu().numpy(), lens, 16000, **fkw)
    out_i, _ = ss.log_mel_spectrogram_packed(pcm.cpu().numpy(), lens, 16000, pcm_scale=PCM_SCALE, **fkw)
    out_di, _ = ss.log_mel_spectrogram_packed(pcm, lens, 16000, pcm_scale=PCM_SCALE, **fkw)
    torch.cuda.synchronize()
    assert np.array_equal(ro_h, ro) and np.array_equal(ro_d.cpu().numpy(), ro)
    assert torch.equal(out_d, dev) and torch.equal(out_di, dev)
    assert isinstance(out_h, np.ndarray) and np.array_equal(out_h, dev.cpu().numpy()) and np.array_equal(out_i, dev.cpu().numpy())
    clips = [xf[int(so[b]):int(so[b + 1])] for b in range(len(lens))]
    lst = ss.log_mel_spectrogram_list(clips, 16000, **fkw)
    lst_h = ss.log_mel_spectrogram_list([c.cpu().numpy() for c in clips], 16000, **fkw)
    for b, blk in enumerate(_blocks(dev, ro, M)):
        assert lst[b].shape == (M, int(ro[b + 1] - ro[b]))
        assert torch.equal(lst[b].reshape(-1), blk) and np.array_equal(lst_h[b].reshape(-1), blk.cpu().numpy()), b
    # dense: the device form through ctypes, the Python front on the device and on the host (float and int16), 1-D and 2-D
    ch, L = 3, 4000
    pcm2 = _pcm(torch, ["noise", "zero", "tone"], [L] * ch).reshape(ch, L)
    xf2 = pcm2.float() * PCM_SCALE
    dev2 = _fused_dense(torch, sslib, cfg, xf2, [], "", ch, L, db)
    torch.cuda.synchronize()
    assert torch.equal(ss.log_mel_spectrogram(xf2, 16000, **fkw), dev2)
    assert torch.equal(ss.log_mel_spectrogram(pcm2, 16000, pcm_scale=PCM_SCALE, **fkw), dev2)
    assert np.array_equal(ss.log_mel_spectrogram(xf2.cpu().numpy(), 16000, **fkw), dev2.cpu().numpy())
    assert np.array_equal(ss.log_mel_spectrogram(pcm2.cpu().numpy(), 16000, pcm_scale=PCM_SCALE, **fkw), dev2.cpu().numpy())
    one = ss.log_mel_spectrogram(xf2[2], 16000, **fkw)
    assert one.shape == dev2.shape[1:] and torch.equal(one, dev2[2])  # a clip's floor is its own: alone or in a batch
