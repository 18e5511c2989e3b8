#!/usr/bin/env python3
"""Worst observed parity errors per BASELINE configuration and signal class, HIP path (through the C ABI) against the
f64-accumulating oracle, with the oracle's own f32 reference-shaped port measured the same way beside it.

    python tools/parity_report.py profiles/r02/parity.json        (on the GPU box)

Metrics per (config, signal), all over one clip:
  max_norm      max|got - want| / max|want| over the whole block (the round-1 metric)
  col0_norm     the same over column 0 alone (ln E when dc_elimination is on)          -- MFCC only
  rest_norm     the same over columns 1.. alone (the cepstra proper)                   -- MFCC only
  elem_rel      max over elements with |want| > 1e-3 max|want| of |got - want| / |want| (columns 1.. for MFCC)
  col_norm      max over the columns c of max_t|got - want| / max_t|want|: every cepstral column against its OWN maximum
                over the frames, so a wrong DCT row cannot hide behind ln E or a louder column                -- MFCC only
  band_norm     the same per mel band over the rows, over the bands whose own maximum is at least BAND_FLOOR of the block
                maximum (power within 40 dB of the loudest band: below that the f32 noise floor of any FFT, ~1e-7 of the peak
                amplitude, alone exceeds 1e-4 relative); band_left_out is the share of bands that restriction leaves out,
                taken from `want` alone                                        -- mel spectrogram and the mfe feature block
`port_*` are the same numbers for oracle/ss_oracle.c's single-thread f32 port: what f32 arithmetic in the reference's
own operation order costs against the f64 oracle.  tests/test_gpu_parity_strict.py asserts on these metrics.

    python tools/parity_report.py --families profiles/parity_families.json        (on the GPU box)

One small configuration per kernel family behind the dispatcher (FAMILIES), all signal classes of a family as the clips of
ONE batch call per output kind, the kernel the call reached by name, and the metrics above per clip.  The signal classes are
those of signals() with a tone that is never bin-centred, an impulse train at the family's hop and a tilted-noise class
(family_signals).  tests/test_parity_families_cpu.py holds the f32 port to the same metrics (which cases are well-posed),
tests/test_gpu_parity_families.py the kernels.

    python tools/parity_report.py --variants profiles/parity_variants.json        (on the GPU box)

The same per switch set (VARIANTS) and alternative frame length (LENGTHS) of every family: EXPECT lists, per family, the rows
and the kernel -- prefix and tags of ss_last_kernel_name() -- that the MFCC, the mfe and the mel call of each row must reach
(each tag is a template argument: other device code).  Per row the report holds the kernels reached, the worst value with its
signal class and the bar per bar metric, and the cases that do not count.  tests/test_parity_variants_cpu.py is the CPU side,
tests/test_gpu_parity_variants.py holds the kernels to the bars.
"""
import datetime
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "mfcc-rust_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

from common import CONFIGS, N_SAMPLES  # noqa: E402


def signals(n, sr):
    """Golden signals plus quiet clips and a clip with silent frames (digital silence between bursts)."""
    t = np.arange(n)
    noise = (np.random.default_rng(0).standard_normal(n) * 0.1).astype(np.float32)
    gaps = noise.copy()
    gaps[n // 5: 2 * n // 5] = 0.0
    gaps[3 * n // 5: 7 * n // 10] = 0.0
    return {
        "noise": noise,
        "sine1k": (0.5 * np.sin(2 * np.pi * 1000.0 * t / sr)).astype(np.float32),
        "dc": np.full(n, 0.25, np.float32),
        "impulse": np.where(t % 160 == 0, 1.0, 0.0).astype(np.float32),
        "quiet_1e-3": (noise * 1e-3).astype(np.float32),
        "quiet_1e-5": (noise * 1e-5).astype(np.float32),
        "silent_frames": gaps,
    }


BAND_FLOOR = 1e-4  # band_norm looks at the bands whose own maximum is at least this share of the block maximum


def metrics(got, want, mfcc, band_axis=0):
    """band_axis: where the mel bands are in a block that is not MFCC (0: mel spectrogram [n_mels, rows]; 1: mfe features
    [frames, n_filters])."""
    got = np.asarray(got, np.float64)
    want = np.asarray(want, np.float64)
    out = {"max_norm": float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-300))}
    body_g, body_w = (got[:, 1:], want[:, 1:]) if mfcc else (got, want)
    if mfcc:
        out["col0_norm"] = float(np.abs(got[:, 0] - want[:, 0]).max() / max(np.abs(want[:, 0]).max(), 1e-300))
        out["rest_norm"] = float(np.abs(body_g - body_w).max() / max(np.abs(body_w).max(), 1e-300))
    big = np.abs(body_w) > 1e-3 * np.abs(body_w).max()
    out["elem_rel"] = float((np.abs(body_g - body_w)[big] / np.abs(body_w)[big]).max()) if big.any() else 0.0
    # every column / band against its own maximum over the frames / rows (axis 0 below)
    g, w = (got, want) if mfcc or band_axis == 1 else (got.T, want.T)
    err, ref = np.abs(g - w).max(axis=0), np.abs(w).max(axis=0)
    if mfcc:
        out["col_norm"] = float((err / np.maximum(ref, 1e-300)).max())
    else:
        keep = (ref >= BAND_FLOOR * ref.max()) & (ref > 0.0)
        out["band_norm"] = float((err[keep] / ref[keep]).max()) if keep.any() else 0.0
        out["band_left_out"] = float(1.0 - keep.mean())
    return out


def run(ss, oracle):
    rep = {}
    for name, kw in CONFIGS.items():
        n, sr = N_SAMPLES[name], kw["sample_rate"]
        p = oracle.make_params(**kw)
        mfcc = name != "cfg3"
        py_kw = dict(frame_length=kw.get("frame_length", 0.02), frame_stride=kw.get("frame_stride", 0.01),
                     num_cepstral=kw.get("num_cepstral", 13), num_filters=kw.get("num_filters", 40),
                     fft_length=kw.get("fft_points", 512), high_frequency=kw.get("high_frequency"))
        rep[name] = {}
        for sname, x in signals(n, sr).items():
            if mfcc:
                got, want, port = ss.mfcc(x, sr, **py_kw), oracle.mfcc(p, x), oracle.port_mfcc(p, x)
            else:
                got, want, port = ss.mel_spectrogram(x, sr, **py_kw), oracle.mel_spectrogram(p, x), oracle.port_mel_spectrogram(p, x)
            m = metrics(got, want, mfcc)
            m.update({"port_" + k: v for k, v in metrics(port, want, mfcc).items()})
            rep[name][sname] = m
    return rep


# ---------------------------------------------------------------------------------------------------------------------
# one small configuration per kernel family
# ---------------------------------------------------------------------------------------------------------------------

def _frame(sr, fft, flen, step, M, C, kernel, tag=""):
    return dict(path="frame", sr=sr, fft=fft, flen=flen, step=step, M=M, C=C, kernel=kernel, tag=tag)


def _stft(sr, fft, hop, M, kernel, tag="", high_frequency=None):
    return dict(path="stft", sr=sr, fft=fft, hop=hop, M=M, kernel=kernel, tag=tag, high_frequency=high_frequency)


# `kernel`: what ss_last_kernel_name() must start with; `tag`: what it must also contain (the chirp-z build of the generic
# kernel reports ss_front_generic<LOG2C,chirpz>).  The shapes are those tests/test_gpu_parity.py's edge-signal tests send to
# these kernels: the smallest that still cross quad, pair and wave boundaries.
FAMILIES = {
    "mfcc_c256x2": _frame(8000, 256, 160, 80, 40, 13, "ss_mfcc_c256x2"),
    "mfcc_c256": _frame(16000, 512, 320, 160, 40, 13, "ss_mfcc_c256<"),
    "mfcc_c256w": _frame(16000, 512, 400, 160, 80, 13, "ss_mfcc_c256w<"),
    "mfcc_c512": _frame(22050, 1024, 1024, 256, 64, 20, "ss_mfcc_c512"),
    "mfcc_c1024": _frame(44100, 2048, 2048, 512, 128, 20, "ss_mfcc_c1024"),
    "mfcc_c2048": _frame(44100, 4096, 4096, 1024, 256, 40, "ss_mfcc_c2048"),
    "front_generic": _frame(16000, 128, 128, 64, 20, 12, "ss_front_generic<"),
    "front_generic_chirpz": _frame(16000, 400, 400, 160, 40, 13, "ss_front_generic<", tag="chirpz"),
    "mel_c256": _stft(16000, 512, 256, 40, "ss_mel_c256"),
    "mel_c512": _stft(16000, 1024, 512, 80, "ss_mel_c512"),
    "mel_c1024": _stft(16000, 2048, 512, 128, "ss_mel_c1024", high_frequency=8000.0),
    "mel_c2048": _stft(44100, 4096, 1024, 256, "ss_mel_c2048"),
    "mel_generic_chirpz": _stft(16000, 400, 200, 40, "ss_front_generic", tag="chirpz"),
}
TONE_HZ = 1000.0 * np.sqrt(2.0)
ROWS = 25  # frames / rows per clip, plus an odd tail of 3 samples
# the metrics the bars are set on, per output kind
BAR_METRICS = {"mfcc": ("col0_norm", "rest_norm", "col_norm"), "mfe": ("band_norm",), "mel": ("band_norm",)}
ALWAYS_COUNTED = ("noise", "tilted", "quiet_1e-3", "quiet_1e-5", "silent_frames")
TOL = 1e-4


def family_kinds(fam):
    return ("mfcc", "mfe") if fam["path"] == "frame" else ("mel",)


def family_hop(fam):
    return fam["step"] if fam["path"] == "frame" else fam["hop"]


def variant_family(fam, variant):
    """The family with the frame length / filter count of a LENGTHS row in place of its own."""
    over = {k: variant[k] for k in ("flen", "M") if variant is not None and variant.get(k) is not None}
    return dict(fam, **over) if over else fam


def family_samples(fam, variant=None):
    """Samples per clip.  Centred framing keeps this count (the oracle then gives 1 + n // hop rows)."""
    fam = variant_family(fam, variant)
    return (fam["flen"] if fam["path"] == "frame" else fam["fft"]) + (ROWS - 1) * family_hop(fam) + 3


def family_signals(fam):
    """The classes of signals() for a family's clip, with three changes.  The tone starts at 1000 sqrt(2) Hz and glides
    up one octave over the clip: it rests on no bin centre (a bin-centred tone has exact zeros in f64 where f32 has rounding
    noise: after ln the comparison is ill-posed), and its frames differ -- a stationary tone gives every frame the same
    cepstra, so a column that happens to be near zero is near zero in all frames and col_norm, which divides by the column's
    own maximum, is ill-conditioned (the f32 port: 2.3e-4 in column 33 of the 4096-point family on the fixed tone, at an
    absolute error of 1.3e-6).  The impulse train runs at the family's hop.  `tilted` is noise whose power falls about 40 dB
    across the band."""
    n, sr, hop = family_samples(fam), fam["sr"], family_hop(fam)
    t = np.arange(n)
    white = np.random.default_rng(0).standard_normal(n)
    noise = (white * 0.1).astype(np.float32)
    spec = np.fft.rfft(white) * 10.0 ** (-2.0 * np.arange(n // 2 + 1) / (n // 2))  # amplitude 1 .. 1e-2: 40 dB in power
    tilted = np.fft.irfft(spec, n)
    gaps = noise.copy()
    gaps[n // 5: 2 * n // 5] = 0.0
    gaps[3 * n // 5: 7 * n // 10] = 0.0
    return {
        "noise": noise,
        "tilted": (tilted * (0.1 / tilted.std())).astype(np.float32),
        "tone": (0.5 * np.sin(2 * np.pi * TONE_HZ * (t + 0.5 * t * t / n) / sr)).astype(np.float32),
        "dc": np.full(n, 0.25, np.float32),
        "impulse": np.where(t % hop == 0, 1.0, 0.0).astype(np.float32),
        "quiet_1e-3": (noise * 1e-3).astype(np.float32),
        "quiet_1e-5": (noise * 1e-5).astype(np.float32),
        "silent_frames": gaps,
    }


def family_kwargs(fam, variant=None):
    """(keywords of oracle.make_params, keywords of the Python front's calls); `variant`: a row of variant_rows() -- its
    switches go to both, its frame length / filter count replace the family's."""
    fam = variant_family(fam, variant)
    sr = fam["sr"]
    if fam["path"] == "frame":
        okw = dict(sample_rate=sr, fft_points=fam["fft"], frame_length=fam["flen"] / sr, frame_stride=fam["step"] / sr,
                   num_cepstral=fam["C"], num_filters=fam["M"])
    else:
        okw = dict(sample_rate=sr, fft_points=fam["fft"], frame_length=fam["hop"] / sr, frame_stride=fam["hop"] / sr, num_filters=fam["M"])
        if fam["high_frequency"] is not None:
            okw["high_frequency"] = fam["high_frequency"]
    if variant is not None:
        okw.update(variant["switches"])
    skw = {{"fft_points": "fft_length"}.get(k, k): v for k, v in okw.items() if k != "sample_rate"}
    return okw, skw


MFE_DROPS = ("num_cepstral", "dc_elimination", "dct_norm")  # what the Python front's mfe calls do not take


def family_reference(oracle, fam, X, port=False, variant=None):
    """{kind: [S, ...] f64 oracle block} for the clips X [S, n]; port=True: the f32 port's, None where it refuses the
    configuration (fft_points that are not a power of two)."""
    p = oracle.make_params(**family_kwargs(fam, variant)[0])
    try:
        if fam["path"] == "stft":
            return {"mel": np.asarray((oracle.port_mel_spectrogram if port else oracle.mel_spectrogram)(p, X), np.float64)}
        return {"mfcc": np.stack([np.asarray((oracle.port_mfcc if port else oracle.mfcc)(p, x), np.float64) for x in X]),
                "mfe": np.stack([np.asarray((oracle.port_mfe if port else oracle.mfe)(p, x)[0], np.float64) for x in X])}
    except oracle.OracleError as e:
        if port and e.code == oracle.ORC_ERR_BAD_CONFIG:
            return None
        raise


def family_outputs(ss, fam, X, variant=None):
    """{kind: [S, ...] block} of ONE batch call per output kind on the clips X [S, n], and {kind: kernel name}."""
    skw = family_kwargs(fam, variant)[1]
    last = ss._lib.lib().ss_last_kernel_name
    out, names = {}, {}
    if fam["path"] == "stft":
        out["mel"] = np.asarray(ss.mel_spectrogram(X, fam["sr"], **skw))
        names["mel"] = last().decode()
        return out, names
    out["mfcc"] = np.asarray(ss.mfcc_batch(X, fam["sr"], **skw))
    names["mfcc"] = last().decode()
    out["mfe"] = np.asarray(ss.mfe_batch(X, fam["sr"], **{k: v for k, v in skw.items() if k not in MFE_DROPS})[0])
    names["mfe"] = last().decode()
    return out, names


def reaches(fam, name):
    return name.startswith(fam["kernel"]) and fam["tag"] in name


def block_metrics(kind, got, want):
    return metrics(got, want, kind == "mfcc", band_axis=1 if kind == "mfe" else 0)


def port_families(oracle, families=None, variant=None):
    """{family: {signal: {kind: metrics of the f32 port against the f64 oracle}}}; None for a family the port refuses.
    `variant`: every family of `families` under that row of variant_rows()."""
    rep = {}
    for name, fam in (families or FAMILIES).items():
        sig = family_signals(variant_family(fam, variant))
        X = np.stack(list(sig.values()))
        want, port = family_reference(oracle, fam, X, variant=variant), family_reference(oracle, fam, X, port=True, variant=variant)
        rep[name] = None if port is None else {s: {k: block_metrics(k, port[k][i], want[k][i]) for k in want} for i, s in enumerate(sig)}
    return rep


def _keys(name, variant):
    """Where a report keeps (family, variant) and the 128-point generic family under the same switches: the family name
    alone without a variant (port_families), (family, variant name) with one (port_variants)."""
    return (name, "front_generic") if variant is None else ((name, variant["name"]), ("front_generic", variant["name"]))


def counted(port_rep, name, variant=None):
    """The (signal, kind, metric) cases of a family that count: the port's own value is at most TOL.  The chirp-z families
    have no port: they take the signal classes of which every case counts for the 128-point generic family (under the same
    variant), minus `dc`."""
    key, generic = _keys(name, variant)
    if port_rep.get(key) is None:
        base = port_rep[generic]
        ok = [s for s, kinds in base.items() if s != "dc" and all(kinds[k][m] <= TOL for k in kinds for m in BAR_METRICS[k])]
        return {(s, k, m) for s in ok for k in family_kinds(FAMILIES[name]) for m in BAR_METRICS[k]}
    return {(s, k, m) for s, kinds in port_rep[key].items() for k in kinds for m in BAR_METRICS[k] if kinds[k][m] <= TOL}


def bars(port_rep, name, variant=None):
    """{(kind, metric): bar}: max(TOL, 1.5 x the port's worst value over the family's counted cases) -- the HIP path may not
    be worse than the reference's own arithmetic; TOL where there is no port."""
    fam = FAMILIES[name]
    key = _keys(name, variant)[0]
    out = {(k, m): TOL for k in family_kinds(fam) for m in BAR_METRICS[k]}
    if port_rep.get(key) is not None:
        for s, k, m in counted(port_rep, name, variant):
            out[(k, m)] = max(out[(k, m)], 1.5 * port_rep[key][s][k][m])
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the switch and frame-length builds of every family
# ---------------------------------------------------------------------------------------------------------------------

_LIB = dict(mfcc_window="hann", spectrum_exponent=2, mel_scale="slaney", mel_norm="slaney", dct_norm="ortho")
# switch-set name -> keywords (of oracle.make_params and of the Python front alike)
VARIANTS = {
    "win": dict(mfcc_window="hann"),
    "vorbis": dict(mfcc_window="vorbis"),
    "pre": dict(preemph_coef=0.97),
    "winpre": dict(mfcc_window="hann", preemph_coef=0.97),
    "pow2": dict(spectrum_exponent=2),
    "ortho": dict(dct_norm="ortho"),
    "slaney": dict(mel_scale="slaney", mel_norm="slaney"),
    "htk": dict(mel_scale="htk"),
    "lib": dict(_LIB),
    "nodc": dict(dc_elimination=False),
    "band": dict(low_frequency=300.0),
    "padded": dict(framing="padded"),
    "center_reflect": dict(framing="center", pad_mode="reflect"),
    "center_constant": dict(framing="center", pad_mode="constant"),
    "center_lib": dict(_LIB, framing="center", pad_mode="reflect"),
    "center_pre": dict(framing="center", pad_mode="reflect", preemph_coef=0.97),
}
# Alternative frame lengths (and one filter count) per family: one per first-pass class of the family's launcher.
#   ss_mfcc_c256x2: flen <= 160 -> 10 inputs, else 16            ss_mfcc_c256 / ss_mfcc_c256w: <= 320 -> 10, <= 416 -> 13, else 16
#   ss_mfcc_c256: flen == 320 is the `exact` build, 40 filters the symmetric-DCT builds (M = 39: `res2`, the default bank's tap counts
#   without the symmetric DCT; M = 26: other tap counts, the run-time bank build)
#   ss_mfcc_c512 / ss_mfcc_c1024: the frame length is a run-time argument     ss_mfcc_c2048: flen == 4096 is `exact`
LENGTHS = {
    "mfcc_c256x2": (dict(flen=200),),
    "mfcc_c256": (dict(flen=256), dict(flen=400), dict(flen=512), dict(M=26), dict(M=39)),
    "mfcc_c256w": (dict(flen=320), dict(flen=512)),
    "mfcc_c512": (dict(flen=700),),
    "mfcc_c1024": (dict(flen=1500),),
    "mfcc_c2048": (dict(flen=3000),),
    "front_generic": (dict(flen=100),),
}
# The switch tags each frame family's launcher has builds for (template arguments: different device code); every one of them
# must be named by a row of the family that stays on its kernel.
LAUNCHER_TAGS = {
    "mfcc_c256x2": ("10", "16", "pow2", "mfe", "win"),
    "mfcc_c256": ("win", "pre", "mfe", "pow2", "fullp", "center", "10", "13", "16", "exact", "bank421", "sym", "res2"),
    "mfcc_c256w": ("10", "13", "16", "pow2", "mfe", "win"),
    "mfcc_c512": ("pow2", "mfe", "win", "lib"),
    "mfcc_c1024": ("pow2", "mfe", "win", "lib", "pre"),
    "mfcc_c2048": ("exact", "pow2", "mfe", "win", "pre"),
    "front_generic": (),
    "front_generic_chirpz": ("chirpz",),
}


def _k(prefix, tags=""):
    """What ss_last_kernel_name() must report: the prefix, and the tags that must be among those between its < >."""
    return (prefix, tuple(t for t in tags.split(",") if t))


def _same(kernel, *names):
    return {n: kernel for n in names}


_X2, _C, _W, _K5, _G1, _H2, _GEN = ("ss_mfcc_c256x2<", "ss_mfcc_c256<", "ss_mfcc_c256w<", "ss_mfcc_c512", "ss_mfcc_c1024",
                                    "ss_mfcc_c2048", "ss_front_generic<")
# family -> row name -> (MFCC kernel, mfe kernel) / (mel kernel,).  A row name is a VARIANTS name, "flenN" / "MN" (a LENGTHS
# entry alone) or "flenN+win".  Written from the launchers (launch_frames / launch_stft in ss_api.hip and each kernel file's
# launch_*): a build the family's kernel does not have sends the call down the ladder -- in ss_mfcc_c256's launcher `fullp` or
# `center` with the mfe output or fused pre-emphasis, a window or pre-emphasis off the 320-sample frame, power spectra with the
# mfe output (the wide-bank kernel takes those); padded framing everywhere and centred frames on the 256- and 4096-point
# kernels (the generic kernel takes those).  The MFCC and the mfe call are different builds.
EXPECT = {
    "mfcc_c256x2": {
        **_same((_k(_X2, "10,win"), _k(_X2, "10,mfe,win")), "win", "vorbis", "winpre"),
        **_same((_k(_X2, "10"), _k(_X2, "10,mfe")), "pre", "ortho", "nodc", "band", "slaney"),
        "pow2": (_k(_X2, "10,pow2"), _k(_X2, "10,pow2,mfe")),
        "flen200": (_k(_X2, "16"), _k(_X2, "16,mfe")),
        "flen200+win": (_k(_X2, "16,win"), _k(_X2, "16,mfe,win")),
    },
    "mfcc_c256": {
        **_same((_k(_C, "10,exact,bank421,win"), _k(_C, "10,exact,bank421,mfe,win")), "win", "vorbis"),
        "pre": (_k(_C, "10,exact,bank421,pre"), _k(_C, "10,exact,bank421,mfe,pre")),
        "winpre": (_k(_C, "10,exact,bank421,win,pre"), _k(_C, "10,exact,bank421,mfe,win,pre")),
        "pow2": (_k(_C, "10,exact,pow2"), _k(_W, "10,pow2,mfe")),
        **_same((_k(_C, "10,exact,bank421,sym"), _k(_C, "10,exact,bank421,mfe")), "ortho", "nodc", "band"),
        **_same((_k(_C, "16,fullp"), _k(_W, "10,mfe")), "slaney", "htk"),
        "lib": (_k(_C, "16,pow2,win,fullp"), _k(_W, "10,pow2,mfe,win")),
        "padded": (_k(_GEN, "8"), _k(_GEN, "8")),
        **_same((_k(_C, "16,center"), _k(_W, "10,mfe")), "center_reflect", "center_constant"),
        "center_lib": (_k(_C, "16,pow2,win,fullp,center"), _k(_W, "10,pow2,mfe,win")),
        "center_pre": (_k(_W, "10"), _k(_W, "10,mfe")),
        "flen256": (_k(_C, "10"), _k(_W, "10,mfe")),
        "flen400": (_k(_C, "13,bank421,sym"), _k(_W, "13,mfe")),
        "flen400+win": (_k(_W, "13,win"), _k(_W, "13,mfe,win")),
        "flen512": (_k(_C, "16"), _k(_W, "16,mfe")),
        "M26": (_k(_C, "10,exact"), _k(_W, "10,mfe")),  # tap counts 6 / 2: not the default bank's 4 / 2 / 1
        "M39": (_k(_C, "10,exact,bank421,res2"), _k(_C, "10,exact,bank421,mfe")),  # 4 / 2 / 1, but not the 40 filters of `sym`
    },
    "mfcc_c256w": {
        **_same((_k(_W, "13,win"), _k(_W, "13,mfe,win")), "win", "vorbis", "winpre"),
        **_same((_k(_W, "13"), _k(_W, "13,mfe")), "pre", "ortho", "slaney", "htk", "nodc", "band", "center_reflect", "center_constant",
                "center_pre"),
        "pow2": (_k(_W, "13,pow2"), _k(_W, "13,pow2,mfe")),
        **_same((_k(_W, "13,pow2,win"), _k(_W, "13,pow2,mfe,win")), "lib", "center_lib"),
        "padded": (_k(_GEN, "8"), _k(_GEN, "8")),
        "flen320": (_k(_W, "10"), _k(_W, "10,mfe")),
        "flen512": (_k(_W, "16"), _k(_W, "16,mfe")),
        "flen512+win": (_k(_W, "16,win"), _k(_W, "16,mfe,win")),
    },
    "mfcc_c512": {
        **_same((_k(_K5, "win"), _k(_K5, "mfe,win")), "win", "vorbis", "winpre", "flen700+win"),
        **_same((_k(_K5), _k(_K5, "mfe")), "pre", "ortho", "nodc", "band", "flen700"),
        "pow2": (_k(_K5, "pow2"), _k(_K5, "pow2,mfe")),
        **_same((_k(_K5, "lib"), _k(_K5, "mfe,lib")), "slaney", "htk", "center_reflect", "center_constant", "center_pre"),
        **_same((_k(_K5, "pow2,win,lib"), _k(_K5, "pow2,mfe,win,lib")), "lib", "center_lib"),
    },
    "mfcc_c1024": {
        **_same((_k(_G1, "win"), _k(_G1, "mfe,win")), "win", "vorbis", "flen1500+win"),
        **_same((_k(_G1), _k(_G1, "mfe")), "ortho", "nodc", "band", "flen1500"),
        "pre": (_k(_G1, "lib,pre"), _k(_G1, "mfe,lib,pre")),
        "winpre": (_k(_G1, "win,lib,pre"), _k(_G1, "mfe,win,lib,pre")),
        "center_pre": (_k(_G1, "lib,pre"), _k(_G1, "mfe,lib,pre")),
        "pow2": (_k(_G1, "pow2"), _k(_G1, "pow2,mfe")),
        **_same((_k(_G1, "lib"), _k(_G1, "mfe,lib")), "slaney", "htk", "center_reflect", "center_constant"),
        **_same((_k(_G1, "pow2,win,lib"), _k(_G1, "pow2,mfe,win,lib")), "lib", "center_lib"),
    },
    "mfcc_c2048": {
        **_same((_k(_H2, "exact,win"), _k(_H2, "exact,mfe,win")), "win", "vorbis"),
        "pre": (_k(_H2, "pre"), _k(_H2, "mfe,pre")),
        "winpre": (_k(_H2, "win,pre"), _k(_H2, "mfe,win,pre")),
        "pow2": (_k(_H2, "exact,pow2"), _k(_H2, "exact,pow2,mfe")),
        **_same((_k(_H2, "exact"), _k(_H2, "exact,mfe")), "ortho", "nodc", "band"),
        "flen3000": (_k(_H2), _k(_H2, "mfe")),
        "flen3000+win": (_k(_H2, "win"), _k(_H2, "mfe,win")),
    },
    "front_generic": _same((_k(_GEN, "6"), _k(_GEN, "6")), *VARIANTS, "flen100", "flen100+win"),
    "front_generic_chirpz": _same((_k(_GEN, "chirpz"), _k(_GEN, "chirpz")), "win", "pre", "pow2", "slaney", "center_reflect"),
    "mel_c256": _same((_k("ss_mel_c256"),), "slaney", "htk", "band"),
    "mel_c512": _same((_k("ss_mel_c512"),), "slaney", "htk", "band"),
    "mel_c1024": {**_same((_k("ss_mel_c1024", "fullp"),), "slaney", "htk"), "band": (_k("ss_mel_c1024"),)},
    # a bank up to fs / 2 does not fit the 4096-point kernel's P rows of 1025 bins: the generic kernel
    "mel_c2048": {**_same((_k(_GEN, "11"),), "slaney", "htk"), "band": (_k("ss_mel_c2048"),)},
    "mel_generic_chirpz": _same((_k("ss_front_generic", "chirpz"),), "slaney"),
}


def variant_rows(families=None):
    """{(family, row name): row}.  A row: family, name, switches (keywords), flen / M (None: the family's own) and
    kernels {kind: (prefix, tags)}."""
    rows = {}
    for fname, table in EXPECT.items():
        if families is not None and fname not in families:
            continue
        for vname, kernels in table.items():
            shape, _, sw = vname.partition("+")
            if shape in VARIANTS:
                shape, sw = "", shape
            row = dict(family=fname, name=vname, switches=dict(VARIANTS[sw]) if sw else {}, flen=None, M=None,
                       kernels=dict(zip(family_kinds(FAMILIES[fname]), kernels)))
            if shape:
                row["flen" if shape.startswith("flen") else "M"] = int(shape.lstrip("flenM"))
            rows[(fname, vname)] = row
    return rows


def kernel_tags(name):
    """The tags between the < > of a kernel name."""
    return set(name[name.index("<") + 1: name.rindex(">")].split(",")) if "<" in name else set()


def reaches_variant(expect, name):
    return name.startswith(expect[0]) and set(expect[1]) <= kernel_tags(name)


def port_variants(oracle, rows):
    """The f32 port under every row: {(family, row name): as port_families}.  A row of a family without a port (chirp-z) brings
    the 128-point generic family under the same row name along: counted() takes its classes."""
    rep = {}
    for (fname, vname), row in rows.items():
        rep[(fname, vname)] = port_families(oracle, {fname: FAMILIES[fname]}, variant=row)[fname]
        if rep[(fname, vname)] is None and ("front_generic", vname) not in rep:
            base = variant_rows(("front_generic",))[("front_generic", vname)]
            rep[("front_generic", vname)] = port_families(oracle, {"front_generic": FAMILIES["front_generic"]}, variant=base)["front_generic"]
    return rep


def run_variants(ss, oracle, rows=None):
    """run_families over the rows of variant_rows(): {"family/row": config, kernels reached and expected, cases}."""
    rep = {}
    for (fname, vname), row in (rows or variant_rows()).items():
        fam = FAMILIES[fname]
        sig = family_signals(variant_family(fam, row))
        X = np.stack(list(sig.values()))
        got, kernels = family_outputs(ss, fam, X, row)
        want = family_reference(oracle, fam, X, variant=row)
        cases = {s: {k: block_metrics(k, got[k][i], want[k][i]) for k in want} for i, s in enumerate(sig)}
        rep[f"{fname}/{vname}"] = {"switches": row["switches"], "flen": row["flen"], "M": row["M"], "kernels": kernels,
                                   "expected": {k: [e[0], list(e[1])] for k, e in row["kernels"].items()}, "cases": cases}
    return rep


def variants_doc(rep, port_rep, rows=None):
    """The report as written to profiles/parity_variants.json: per (family, row) the kernels reached, the counted cases' worst
    value per bar metric with its bar, and the cases that do not count."""
    out = {}
    for (fname, vname), row in (rows or variant_rows()).items():
        r = rep[f"{fname}/{vname}"]
        cnt, bar = counted(port_rep, fname, row), bars(port_rep, fname, row)
        worst = {}
        for (k, m), b in sorted(bar.items()):
            v, s = max((r["cases"][s][k][m], s) for s, kk, mm in cnt if (kk, mm) == (k, m))
            worst[f"{k}.{m}"] = {"worst": v, "at": s, "bar": b}
        out[f"{fname}/{vname}"] = {
            "kernels": r["kernels"],
            "worst": worst,
            "not_counted": sorted(f"{s}.{k}.{m}" for s in r["cases"] for k in r["cases"][s] for m in BAR_METRICS[k] if (s, k, m) not in cnt)}
    return {"date": datetime.date.today().isoformat(), "kernel_library": "mfcc-rust_amd/lib/libspeechsauce_amd.so",
            "bar": "max(1e-4, 1.5 x the f32 port's worst value over the (family, variant)'s counted cases); 1e-4 without a port",
            "variants": out}


def run_families(ss, oracle, families=None):
    """Per family: all signal classes as the clips of one batch call per output kind, the kernel each call reached, and per
    clip and kind the metrics with the port's `port_*` twins beside them (None where the port refuses the configuration)."""
    rep = {}
    for name, fam in (families or FAMILIES).items():
        sig = family_signals(fam)
        X = np.stack(list(sig.values()))
        got, kernels = family_outputs(ss, fam, X)
        want, port = family_reference(oracle, fam, X), family_reference(oracle, fam, X, port=True)
        cases = {}
        for i, s in enumerate(sig):
            cases[s] = {}
            for k in want:
                m = block_metrics(k, got[k][i], want[k][i])
                pm = block_metrics(k, port[k][i], want[k][i]) if port is not None else dict.fromkeys(m)
                m.update({"port_" + key: v for key, v in pm.items()})
                cases[s][k] = m
        rep[name] = {"config": {k: v for k, v in fam.items() if v is not None and v != ""}, "kernels": kernels, "cases": cases}
    return rep


def families_doc(rep, port_rep):
    """The report as written to profiles/parity_families.json: per family the kernels, the counted cases' worst value per bar
    metric with its bar, and every case."""
    worst = {}
    for name, r in rep.items():
        cnt, bar = counted(port_rep, name), bars(port_rep, name)
        worst[name] = {f"{k}.{m}": {"worst": max(r["cases"][s][k][m] for s, kk, mm in cnt if (kk, mm) == (k, m)), "bar": b}
                       for (k, m), b in sorted(bar.items())}
        r["not_counted"] = sorted(f"{s}.{k}.{m}" for s in r["cases"] for k in r["cases"][s] for m in BAR_METRICS[k] if (s, k, m) not in cnt)
    return {"date": datetime.date.today().isoformat(), "kernel_library": "mfcc-rust_amd/lib/libspeechsauce_amd.so",
            "bar": "max(1e-4, 1.5 x the f32 port's worst value over the family's counted cases); 1e-4 without a port",
            "worst": worst, "families": rep}


if __name__ == "__main__":
    import oracle_c
    import speechsauce_amd as ss

    if len(sys.argv) > 1 and sys.argv[1] == "--families":
        out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "parity_families.json")
        doc = families_doc(run_families(ss, oracle_c), port_families(oracle_c))
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        json.dump(doc, open(out, "w"), indent=1)
        print(json.dumps(doc["worst"], indent=1))
        for name, r in doc["families"].items():
            assert all(reaches(FAMILIES[name], k) for k in r["kernels"].values()), (name, r["kernels"])
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "--variants":
        out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "parity_variants.json")
        rows = variant_rows()
        rep = run_variants(ss, oracle_c, rows)
        doc = variants_doc(rep, port_variants(oracle_c, rows), rows)
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        json.dump(doc, open(out, "w"), indent=1)
        bad = 0
        for key, v in doc["variants"].items():
            over = {m: w for m, w in v["worst"].items() if not w["worst"] <= w["bar"]}
            off = {k: (n, rep[key]["expected"][k]) for k, n in v["kernels"].items() if not reaches_variant(rep[key]["expected"][k], n)}
            print(key, v["kernels"], " ".join(f"{m}={w['worst']:.2e}/{w['bar']:.2e}" for m, w in v["worst"].items()),
                  *(["OVER THE BAR", over] if over else []), *(["NOT THE EXPECTED KERNEL", off] if off else []), flush=True)
            bad += bool(off)
        sys.exit(1 if bad else 0)  # (a value over its bar is reported; tests/test_gpu_parity_variants.py judges it)
    rep = run(ss, oracle_c)
    worst = {c: {k: max(v[k] for v in sig.values()) for k in next(iter(sig.values()))} for c, sig in rep.items()}
    doc = {"kernel_library": "mfcc-rust_amd/lib/libspeechsauce_amd.so", "tolerance": "1e-4 (BASELINE.json north_star)", "worst": worst, "cases": rep}
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r02", "parity.json")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    json.dump(doc, open(out, "w"), indent=1)
    print(json.dumps(worst, indent=1))
