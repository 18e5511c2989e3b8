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


def family_samples(fam):
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


def family_kwargs(fam):
    """(keywords of oracle.make_params, keywords of the Python front's calls)"""
    sr = fam["sr"]
    if fam["path"] == "frame":
        okw = dict(sample_rate=sr, fft_points=fam["fft"], frame_length=fam["flen"] / sr, frame_stride=fam["step"] / sr,
                   num_cepstral=fam["C"], num_filters=fam["M"])
    else:
        okw = dict(sample_rate=sr, fft_points=fam["fft"], frame_length=fam["hop"] / sr, frame_stride=fam["hop"] / sr, num_filters=fam["M"])
        if fam["high_frequency"] is not None:
            okw["high_frequency"] = fam["high_frequency"]
    skw = {{"fft_points": "fft_length"}.get(k, k): v for k, v in okw.items() if k != "sample_rate"}
    return okw, skw


def family_reference(oracle, fam, X, port=False):
    """{kind: [S, ...] f64 oracle block} for the clips X [S, n]; port=True: the f32 port's, None where it refuses the
    configuration (fft_points that are not a power of two)."""
    p = oracle.make_params(**family_kwargs(fam)[0])
    try:
        if fam["path"] == "stft":
            return {"mel": np.asarray((oracle.port_mel_spectrogram if port else oracle.mel_spectrogram)(p, X), np.float64)}
        return {"mfcc": np.stack([np.asarray((oracle.port_mfcc if port else oracle.mfcc)(p, x), np.float64) for x in X]),
                "mfe": np.stack([np.asarray((oracle.port_mfe if port else oracle.mfe)(p, x)[0], np.float64) for x in X])}
    except oracle.OracleError as e:
        if port and e.code == oracle.ORC_ERR_BAD_CONFIG:
            return None
        raise


def family_outputs(ss, fam, X):
    """{kind: [S, ...] block} of ONE batch call per output kind on the clips X [S, n], and {kind: kernel name}."""
    skw = family_kwargs(fam)[1]
    last = ss._lib.lib().ss_last_kernel_name
    out, names = {}, {}
    if fam["path"] == "stft":
        out["mel"] = np.asarray(ss.mel_spectrogram(X, fam["sr"], **skw))
        names["mel"] = last().decode()
        return out, names
    out["mfcc"] = np.asarray(ss.mfcc_batch(X, fam["sr"], **skw))
    names["mfcc"] = last().decode()
    out["mfe"] = np.asarray(ss.mfe_batch(X, fam["sr"], **{k: v for k, v in skw.items() if k != "num_cepstral"})[0])
    names["mfe"] = last().decode()
    return out, names


def reaches(fam, name):
    return name.startswith(fam["kernel"]) and fam["tag"] in name


def block_metrics(kind, got, want):
    return metrics(got, want, kind == "mfcc", band_axis=1 if kind == "mfe" else 0)


def port_families(oracle, families=None):
    """{family: {signal: {kind: metrics of the f32 port against the f64 oracle}}}; None for a family the port refuses."""
    rep = {}
    for name, fam in (families or FAMILIES).items():
        sig = family_signals(fam)
        X = np.stack(list(sig.values()))
        want, port = family_reference(oracle, fam, X), family_reference(oracle, fam, X, port=True)
        rep[name] = None if port is None else {s: {k: block_metrics(k, port[k][i], want[k][i]) for k in want} for i, s in enumerate(sig)}
    return rep


def counted(port_rep, name):
    """The (signal, kind, metric) cases of a family that count: the port's own value is at most TOL.  The chirp-z families
    have no port: they take the signal classes of which every case counts for the 128-point generic family, minus `dc`."""
    if port_rep.get(name) is None:
        base = port_rep["front_generic"]
        ok = [s for s, kinds in base.items() if s != "dc" and all(kinds[k][m] <= TOL for k in kinds for m in BAR_METRICS[k])]
        return {(s, k, m) for s in ok for k in family_kinds(FAMILIES[name]) for m in BAR_METRICS[k]}
    return {(s, k, m) for s, kinds in port_rep[name].items() for k in kinds for m in BAR_METRICS[k] if kinds[k][m] <= TOL}


def bars(port_rep, name):
    """{(kind, metric): bar}: max(TOL, 1.5 x the port's worst value over the family's counted cases) -- the HIP path may not
    be worse than the reference's own arithmetic; TOL where there is no port."""
    fam = FAMILIES[name]
    out = {(k, m): TOL for k in family_kinds(fam) for m in BAR_METRICS[k]}
    if port_rep.get(name) is not None:
        for s, k, m in counted(port_rep, name):
            out[(k, m)] = max(out[(k, m)], 1.5 * port_rep[name][s][k][m])
    return out


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
    rep = run(ss, oracle_c)
    worst = {c: {k: max(v[k] for v in sig.values()) for k in next(iter(sig.values()))} for c, sig in rep.items()}
    doc = {"kernel_library": "mfcc-rust_amd/lib/libspeechsauce_amd.so", "tolerance": "1e-4 (BASELINE.json north_star)", "worst": worst, "cases": rep}
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r02", "parity.json")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    json.dump(doc, open(out, "w"), indent=1)
    print(json.dumps(worst, indent=1))
