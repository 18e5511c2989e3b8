"""µs per call of the Whisper log-mel front end (whisper_log_mel / whisper_log_mel_packed: ss_whisper_c200) beside today's route to
the same numbers, from one process.

    python tools/whisper_rate.py [--clips 256] [--mels 80] [--reps 5] [--rounds 5] [--ring 2] [--pcm16]

Today's route: log_mel_spectrogram(_packed) on fft_length = 400 with a 160-sample hop, centred reflect frames, the Slaney bank with
Slaney norm and top_db = 80 (the chirp-z build of the generic kernel and its dB floor), plus the torch steps that turn its decibels
into the model input: drop the frames past the window, (dB / 10 + 4) / 4, pad to the window with the clip's constant, convert.  The
gather indices of the ragged leg are formed once outside the timed region, which favours that route.
Shapes: `--clips` clips x 30 s (dense), then `--clips` clips of 1 .. 30 s packed, both in the 3000-frame window; f32 and bf16 output.
bytes_per_call of the new call: the live samples once, out once, and the f32 log10 block of the live frames twice (written by the
transform launch, read by the floor launch); hbm_fraction reads it against 8.0 TB/s.
Protocol: every leg is warmed up, then `--rounds` rounds alternate the legs, each timed with HIP events around back-to-back calls on
one stream; every call takes the next of a ring of `--ring` input blocks.  Reported per leg: the median over the rounds, the fastest and
the slowest round; per shape the ratio of the medians and whether the min-max ranges of the two sides overlap.
Prints one JSON line.  Measuring only: not collected by pytest, not part of bench.py.

--pcm16: the same two shapes and output types fed signed 16-bit PCM, three legs each under the same protocol (at least five rounds):
  *_float (a)          whisper_log_mel(_packed) on a ready float buffer
  *_convert_float (b)  pcm.to(float32).mul_(scale) and then that float call: what a caller with an int16 corpus ran before
  *_pcm (c)            whisper_log_mel(_packed)(..., pcm_scale=2^-15) on the int16 buffer
Every leg reports min / median / max over the rounds; then (c) over (b), (c) over (a), and whether (c)'s median lies above (b)'s by more
than the spread (max - min) of (b)'s rounds -- the PCM build being slower than what it replaces.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mfcc-rust_amd"))

HBM_PEAK = 8.0e12
WINDOW = 3000
ROUTE = dict(frame_length=0.01, fft_length=400, mel_scale="slaney", mel_norm="slaney", pad_mode="reflect", top_db=80.0)


def first_silent(length, n_frames):
    L = min(length, n_frames * 160)
    return 0 if L == 0 else min(max(2, -(-(L + 200) // 160)), n_frames)


def pcm16_report(args):
    """the --pcm16 run: see the module docstring"""
    import numpy as np
    import torch

    import speechsauce_amd as ss

    n, M, scale = args.clips, args.mels, 2.0 ** -15
    rounds = max(5, args.rounds)
    rng = np.random.default_rng(0)
    at = [0]
    res = {"pcm16": True, "scale": scale, "clips": n, "n_mels": M, "window_frames": WINDOW, "reps": args.reps, "rounds": rounds, "ring": args.ring,
           "device": torch.cuda.get_device_name()}

    def rings(shape):
        pcm = [torch.randint(-32768, 32768, shape, device="cuda", dtype=torch.int32).to(torch.int16) for _ in range(args.ring)]
        return pcm, [p.to(torch.float32).mul_(scale) for p in pcm]

    lens = rng.integers(16000, WINDOW * 160 + 1, n)
    shapes = {"dense30": rings((n, WINDOW * 160)), "ragged": rings((int(lens.sum()),))}
    res["ragged_seconds_mean"] = float(lens.mean() / 16000)

    def call(shape, x, dtype, **kw):
        if shape == "dense30":
            return ss.whisper_log_mel(x, n_mels=M, n_frames=WINDOW, dtype=dtype, **kw)
        return ss.whisper_log_mel_packed(x, lens, n_mels=M, n_frames=WINDOW, dtype=dtype, **kw)[0]

    def leg(shape, kind, dtype):
        pcm, flt = shapes[shape]

        def fn():
            at[0] += 1
            i = at[0] % args.ring
            if kind == "float":
                return call(shape, flt[i], dtype)
            if kind == "convert_float":
                return call(shape, pcm[i].to(torch.float32).mul_(scale), dtype)
            return call(shape, pcm[i], dtype, pcm_scale=scale)
        return fn

    legs = [(f"{shape}_{name}_{kind}", leg(shape, kind, dtype)) for shape in shapes for name, dtype in (("f32", torch.float32), ("bf16", torch.bfloat16))
            for kind in ("float", "convert_float", "pcm")]
    for shape, (pcm, flt) in shapes.items():  # what is compared computes the same bits
        for dtype in (torch.float32, torch.bfloat16):
            assert torch.equal(call(shape, pcm[0], dtype, pcm_scale=scale), call(shape, flt[0], dtype)), f"{shape}: the PCM call is not the float call"

    def timed(fn, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps * 1e3

    for _, fn in legs:
        for _ in range(args.ring):
            fn()
    torch.cuda.synchronize()
    us = {name: [] for name, _ in legs}
    for _ in range(rounds):
        for name, fn in legs:
            us[name].append(timed(fn, args.reps))
    for name, _ in legs:
        v = us[name]
        res[name] = {"us_min": min(v), "us_median": statistics.median(v), "us_max": max(v)}
    for shape in shapes:
        for name in ("f32", "bf16"):
            a, b, c = (res[f"{shape}_{name}_{kind}"] for kind in ("float", "convert_float", "pcm"))
            c["pcm_over_convert_float"] = c["us_median"] / b["us_median"]
            c["pcm_over_float"] = c["us_median"] / a["us_median"]
            c["slower_than_convert_float"] = c["us_median"] - b["us_median"] > b["us_max"] - b["us_min"]
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=256)
    ap.add_argument("--mels", type=int, default=80)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--ring", type=int, default=2)
    ap.add_argument("--pcm16", action="store_true", help="time the 16-bit PCM calls beside the float calls (see the module docstring)")
    args = ap.parse_args()
    if args.pcm16:
        return pcm16_report(args)

    import numpy as np
    import torch

    import speechsauce_amd as ss

    n, M = args.clips, args.mels
    rng = np.random.default_rng(0)
    at = [0]
    res = {"clips": n, "n_mels": M, "window_frames": WINDOW, "reps": args.reps, "rounds": args.rounds, "ring": args.ring,
           "device": torch.cuda.get_device_name()}
    legs, nbytes = [], {}

    def ring_of(make):
        return [make() for _ in range(args.ring)]

    # ---- dense: n clips x 30 s ----
    dense = ring_of(lambda: torch.randn((n, WINDOW * 160), device="cuda").mul_(0.1))

    def route_dense(dtype):
        def fn():
            at[0] += 1
            db = ss.log_mel_spectrogram(dense[at[0] % args.ring], 16000, num_filters=M, **ROUTE)  # [n, M, R], R >= WINDOW
            out = db[..., :WINDOW].mul(0.025).add_(1.0)
            return out if dtype == torch.float32 else out.to(dtype)
        return fn

    def new_dense(dtype):
        def fn():
            at[0] += 1
            return ss.whisper_log_mel(dense[at[0] % args.ring], n_mels=M, n_frames=WINDOW, dtype=dtype)
        return fn

    # ---- ragged: n clips of 1 .. 30 s, packed ----
    lens = rng.integers(16000, WINDOW * 160 + 1, n)
    total = int(lens.sum())
    packed = ring_of(lambda: torch.randn((total,), device="cuda").mul_(0.1))
    _, ro = ss.log_mel_spectrogram_packed(packed[0], lens, 16000, num_filters=M, **ROUTE)
    ro = np.asarray(ro.cpu() if hasattr(ro, "cpu") else ro, dtype=np.int64)
    rows = np.diff(ro)
    keep = np.minimum(rows, WINDOW)
    # element (b, m, t), t < keep[b], of the window block comes from element M * ro[b] + m * rows[b] + t of the route's flat result
    src = np.concatenate([(M * ro[b] + np.arange(M)[:, None] * rows[b] + np.arange(keep[b])[None, :]).ravel() for b in range(n)])
    dst = np.concatenate([((b * M + np.arange(M))[:, None] * WINDOW + np.arange(keep[b])[None, :]).ravel() for b in range(n)])
    d_src, d_dst = torch.from_numpy(src).cuda(), torch.from_numpy(dst).cuda()
    pad_rows = torch.from_numpy(np.repeat(np.arange(n), M)).cuda()
    seg_lens = torch.from_numpy(M * rows).cuda()

    def route_ragged(dtype):
        def fn():
            at[0] += 1
            flat, _ = ss.log_mel_spectrogram_packed(packed[at[0] % args.ring], lens, 16000, num_filters=M, **ROUTE)
            flat = flat.reshape(-1)
            # the padding is the clip's floor: its maximum - 80 dB, the smallest value of its block
            out = torch.segment_reduce(flat, "min", lengths=seg_lens)[pad_rows][:, None].expand(n * M, WINDOW).contiguous()
            out.view(-1)[d_dst] = flat[d_src]
            out = out.mul_(0.025).add_(1.0).view(n, M, WINDOW)
            return out if dtype == torch.float32 else out.to(dtype)
        return fn

    def new_ragged(dtype):
        def fn():
            at[0] += 1
            return ss.whisper_log_mel_packed(packed[at[0] % args.ring], lens, n_mels=M, n_frames=WINDOW, dtype=dtype)[0]
        return fn

    live_dense = n * M * WINDOW
    live_ragged = sum(M * first_silent(int(k), WINDOW) for k in lens)
    for shape, samples, live, new, route in (("dense30", n * WINDOW * 160, live_dense, new_dense, route_dense),
                                             ("ragged", total, live_ragged, new_ragged, route_ragged)):
        for name, dtype, es in (("f32", torch.float32, 4), ("bf16", torch.bfloat16, 2)):
            legs += [(f"{shape}_{name}_new", new(dtype), args.reps), (f"{shape}_{name}_route", route(dtype), args.reps)]
            nbytes[f"{shape}_{name}_new"] = samples * 4 + n * M * WINDOW * es + 2 * live * 4
    res["ragged_seconds_mean"] = float(lens.mean() / 16000)
    res["ragged_live_frame_fraction"] = live_ragged / live_dense

    # a look, not a test: the route divides by its window's norm and uses the Vorbis window, a constant offset in log10 that its add
    # would absorb at no cost
    a = new_ragged(torch.float32)().float()
    b = route_ragged(torch.float32)().float()
    res["ragged_new_vs_route_median_abs_diff"] = float((a - b).abs().median())
    del a, b

    def timed(fn, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps * 1e3

    for _, fn, _ in legs:
        for _ in range(args.ring):
            fn()
    torch.cuda.synchronize()
    us = {name: [] for name, _, _ in legs}
    for _ in range(args.rounds):
        for name, fn, reps in legs:
            us[name].append(timed(fn, reps))
    for name, _, _ in legs:
        v = us[name]
        leg = res[name] = {"us_per_call_median": statistics.median(v), "us_min": min(v), "us_max": max(v)}
        if name in nbytes:
            leg["bytes_per_call"] = nbytes[name]
            leg["hbm_fraction"] = nbytes[name] / (leg["us_per_call_median"] * 1e-6) / HBM_PEAK
    for shape in ("dense30", "ragged"):
        for name in ("f32", "bf16"):
            new, route = res[f"{shape}_{name}_new"], res[f"{shape}_{name}_route"]
            new["route_over_new"] = route["us_per_call_median"] / new["us_per_call_median"]
            new["ranges_overlap"] = not (new["us_max"] < route["us_min"] or route["us_max"] < new["us_min"])
    print(json.dumps(res))


if __name__ == "__main__":
    main()
