"""Rows/s and median µs per call of the Kaldi fbank / MFCC front end over a pool of stream states (ss_kstream_*_packed_device)
beside what a caller could do without it.

    python tools/kaldi_stream_rate.py [--pool 4096] [--active 1024] [--max-hops 4] [--reps 200] [--ring-mb 320] [--pcm16]

Workload: 16 kHz, 25 / 10 ms frames (400-sample frames, 160-sample hop, S = 320 carried samples per stream); a pool of `--pool`
stream states of which `--active` deliver audio in a call, in random slot order, each 1 .. `--max-hops` hops (uniform).  Every call
is timed on its own with HIP events on one stream after warm-up; the figure is the median over `--reps` calls.  Every call works on
the next element of a ring of pre-built ticks (chunks and tables) whose inputs together are larger than the 256 MB Infinity Cache
(`--ring-mb`), so that a call does not find its samples in the caches an earlier call left them in.
  fbank80       ss_kstream_fbank_packed_device, 80 mel bins, with the log energy (two launches per call)
  mfcc13        ss_kstream_mfcc_packed_device, 13 cepstra on 23 bins
  with --pcm16  the same two legs on the same ticks as signed 16-bit PCM (the _i16 entry points, scale 2^-15) next to the float legs
  frame_pool    baseline (a): ss_mfcc_stream_packed_device, the project's own MFCC (not Kaldi's arithmetic) at its default shape
                (320-sample frames, 160-sample hop, 40 filters) on the same ticks
  per_stream    baseline (b): what a caller does with the dense call alone -- per entry a concatenation of its state row and its
                chunk, one ss_kaldi_fbank_device call (80 bins), and the state row's update; `--loop-reps` ticks only
Prints one JSON line.  Measuring only: not collected by pytest, not part of bench.py.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mfcc-rust_amd"))

STEP = 160


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pool", type=int, default=4096)
    ap.add_argument("--active", type=int, default=1024)
    ap.add_argument("--max-hops", type=int, default=4)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--loop-reps", type=int, default=3)
    ap.add_argument("--ring-mb", type=int, default=320)
    ap.add_argument("--pcm16", action="store_true")
    args = ap.parse_args()

    import numpy as np
    import torch

    import speechsauce_amd as ss
    from speechsauce_amd import _lib

    lib = _lib.lib()
    P, N, H = args.pool, args.active, args.max_hops
    sp = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rng = np.random.default_rng(0)
    cap = N * H  # rows a tick can have
    n_ring = max(2, int(args.ring_mb * 2**20 / (N * (H + 1) / 2 * STEP * 4)) + 1)
    scale = 2.0 ** -15

    ticks = []
    for _ in range(n_ring):
        hops = rng.integers(1, H + 1, N)
        slots = rng.permutation(P)[:N].astype(np.int32)
        so = np.zeros(N + 1, np.int64)
        np.cumsum(hops * STEP, out=so[1:])
        pcm = torch.randint(-3000, 3000, (int(so[-1]),), device="cuda", dtype=torch.int32).to(torch.int16)
        ticks.append({"rows": int(hops.sum()), "pcm": pcm, "x": pcm.to(torch.float32).mul_(scale), "so": torch.from_numpy(so).cuda(),
                      "ro": torch.from_numpy(so // STEP).cuda(), "slots": torch.from_numpy(slots).cuda(), "so_host": so, "slots_host": slots})
    at = [0]

    def nxt():
        at[0] += 1
        return ticks[at[0] % n_ring]

    def timed(fn, reps):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        kernel = lib.ss_last_kernel_name().decode()
        start = at[0]
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
        for a, b in ev:
            a.record()
            fn()
            b.record()
        torch.cuda.synchronize()
        us = statistics.median(a.elapsed_time(b) * 1e3 for a, b in ev)
        rows = sum(ticks[(start + 1 + k) % n_ring]["rows"] for k in range(reps)) / reps
        return {"rows_per_call": rows, "median_us_per_call": us, "rows_per_s": rows / (us * 1e-6), "kernel": kernel}

    res = {"pool": P, "active": N, "max_hops": H, "ring": n_ring, "reps": args.reps, "device": torch.cuda.get_device_name()}

    def kaldi_leg(mfcc, pcm):
        p = _lib.SsKaldiParams()
        _lib.check(lib.ss_kaldi_params_default(C.byref(p), 16000))
        p.num_mel_bins, p.num_ceps = (23, 13) if mfcc else (80, 0)
        cfg = ss.KaldiConfig(p)
        S, D = C.c_size_t(), C.c_size_t()
        _lib.check(lib.ss_kstream_state_len(C.byref(p), C.byref(S), C.byref(D)))
        pool = torch.randn((P, S.value), device="cuda").mul_(0.1)
        out = torch.empty((cap, 13 if mfcc else 80), device="cuda")
        en = torch.empty((cap,), device="cuda")
        fn = getattr(lib, f"ss_kstream_{'mfcc' if mfcc else 'fbank'}_packed{'_i16' if pcm else ''}_device")

        def call():
            t = nxt()
            a = [cfg.handle, t["pcm" if pcm else "x"].data_ptr(), N, t["so"].data_ptr(), t["ro"].data_ptr(), t["rows"], t["slots"].data_ptr(), P]
            a += ([scale] if pcm else []) + [pool.data_ptr(), out.data_ptr()] + ([] if mfcc else [en.data_ptr()])
            _lib.check(fn(*a, sp))

        r = timed(call, args.reps)
        _lib.check(lib.ss_kaldi_config_device_status(cfg.handle))
        return r

    for pcm in ([False, True] if args.pcm16 else [False]):
        tag = "_pcm16" if pcm else ""
        res["fbank80" + tag] = kaldi_leg(False, pcm)
        res["mfcc13" + tag] = kaldi_leg(True, pcm)

    # baseline (a): the frame pool at its default shape on the same ticks
    cfg_a = ss.SpeechConfig(_lib.make_params())
    pool_a = torch.randn((P, 160), device="cuda").mul_(0.1)
    out_a = torch.empty((cap, 13), device="cuda")

    def frame_pool():
        t = nxt()
        _lib.check(lib.ss_mfcc_stream_packed_device(cfg_a.handle, t["x"].data_ptr(), N, t["so"].data_ptr(), t["ro"].data_ptr(), t["rows"],
                                                    t["slots"].data_ptr(), P, 100, pool_a.data_ptr(), out_a.data_ptr(), sp))

    res["frame_pool"] = timed(frame_pool, args.reps)

    # baseline (b): a per-stream loop of the dense call over state ++ chunk
    p = _lib.SsKaldiParams()
    _lib.check(lib.ss_kaldi_params_default(C.byref(p), 16000))
    p.num_mel_bins, p.num_ceps = 80, 0
    cfg_b = ss.KaldiConfig(p)
    pool_b = torch.randn((P, 320), device="cuda").mul_(0.1)
    out_b = torch.empty((cap, 80), device="cuda")

    def per_stream():
        t = nxt()
        so, slots = t["so_host"], t["slots_host"]
        row = 0
        for i in range(N):
            both = torch.cat([pool_b[int(slots[i])], t["x"][int(so[i]):int(so[i + 1])]])
            k = (int(so[i + 1]) - int(so[i])) // STEP
            _lib.check(lib.ss_kaldi_fbank_device(cfg_b.handle, both.data_ptr(), 1, both.numel(), both.numel(), out_b[row:].data_ptr(), None, sp))
            pool_b[int(slots[i])] = both[both.numel() - 320:]
            row += k

    res["per_stream"] = timed(per_stream, args.loop_reps)
    res["per_stream"]["reps"] = args.loop_reps
    res["fbank80_over_per_stream"] = res["fbank80"]["rows_per_s"] / res["per_stream"]["rows_per_s"]
    res["mfcc13_over_frame_pool"] = res["mfcc13"]["rows_per_s"] / res["frame_pool"]["rows_per_s"]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
