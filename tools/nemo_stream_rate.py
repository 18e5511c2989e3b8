"""Median µs per call (with [min, max]) and rows/s of the NeMo / Parakeet log-mel front end over a pool of stream states
(ss_nstream_log_mel_packed_device) beside the Kaldi pool on the same ticks and beside what a caller could do without it.

    python tools/nemo_stream_rate.py [--pool 4096] [--active 1024] [--max-hops 4] [--reps 200] [--ring-mb 320] [--pcm16]

Workload: 16 kHz, 400-sample window, 160-sample hop (S = 361 carried samples per stream, L = 1 row of delay); a pool of `--pool`
stream states of which `--active` deliver audio in a call, in random slot order, each 1 .. `--max-hops` hops (uniform).  Every call
is timed on its own with HIP events on one stream after warm-up; the figures are the median, the smallest and the largest over
`--reps` calls.  Every call works on the next element of a ring of pre-built ticks (chunks and tables) whose inputs together are
larger than the 256 MB Infinity Cache (`--ring-mb`), so that a call does not find its samples in the caches an earlier call left
them in.
  nemo80 / nemo128  ss_nstream_log_mel_packed_device, 80 and 128 bands (two launches per call: the rows, the state advance)
  with --pcm16      the same two legs on the same ticks as signed 16-bit PCM (the _i16 entry point, scale 2^-15)
  flush80           ss_nstream_flush_device over the tick's slots, 80 bands (the rows launch and the zeroing of the named rows)
  kaldi_fbank80     the yardstick: ss_kstream_fbank_packed_device at 80 bins with the log energy, on the same ticks in the same run
  per_stream        what a caller does with the dense call alone -- per entry a concatenation of its carried samples and its chunk,
                    one ss_nemo_log_mel_device call (80 bands), and the carried samples' update; `--loop-reps` ticks only
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

    def timed(fn, reps, rows_of=lambda t: t["rows"]):
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
        each = [a.elapsed_time(b) * 1e3 for a, b in ev]
        us = statistics.median(each)
        rows = sum(rows_of(ticks[(start + 1 + k) % n_ring]) for k in range(reps)) / reps
        return {"rows_per_call": rows, "median_us_per_call": us, "min_us": min(each), "max_us": max(each), "rows_per_s": rows / (us * 1e-6),
                "kernel": kernel}

    res = {"pool": P, "active": N, "max_hops": H, "ring": n_ring, "reps": args.reps, "device": torch.cuda.get_device_name()}

    def nemo_cfg(n_mels):
        p = _lib.SsNemoParams()
        _lib.check(lib.ss_nemo_params_default(C.byref(p), n_mels))
        p.normalize = 0
        S, L = C.c_size_t(), C.c_size_t()
        _lib.check(lib.ss_nstream_state_len(C.byref(p), C.byref(S), C.byref(L)))
        return ss.NemoConfig(p), S.value, L.value

    def nemo_leg(n_mels, pcm):
        cfg, S, _ = nemo_cfg(n_mels)
        pool = torch.randn((P, S), device="cuda").mul_(0.1)
        out = torch.empty((cap, n_mels), device="cuda")
        fn = getattr(lib, f"ss_nstream_log_mel_packed{'_i16' if pcm else ''}_device")

        def call():
            t = nxt()
            a = [cfg.handle, t["pcm" if pcm else "x"].data_ptr(), N, t["so"].data_ptr(), t["ro"].data_ptr(), t["rows"], t["slots"].data_ptr(), P]
            a += ([scale] if pcm else []) + [pool.data_ptr(), out.data_ptr()]
            _lib.check(fn(*a, sp))

        r = timed(call, args.reps)
        _lib.check(lib.ss_nemo_config_device_status(cfg.handle))
        return r

    for pcm in ([False, True] if args.pcm16 else [False]):
        tag = "_pcm16" if pcm else ""
        res["nemo80" + tag] = nemo_leg(80, pcm)
        res["nemo128" + tag] = nemo_leg(128, pcm)

    cfg_f, S_f, L_f = nemo_cfg(80)
    pool_f = torch.randn((P, S_f), device="cuda").mul_(0.1)
    out_f = torch.empty((N * L_f, 80), device="cuda")

    def flush():
        t = nxt()
        _lib.check(lib.ss_nstream_flush_device(cfg_f.handle, N, t["slots"].data_ptr(), P, pool_f.data_ptr(), out_f.data_ptr(), sp))

    res["flush80"] = timed(flush, args.reps, lambda t: N * L_f)

    # the yardstick: the Kaldi pool at 80 bins on the same ticks
    kp = _lib.SsKaldiParams()
    _lib.check(lib.ss_kaldi_params_default(C.byref(kp), 16000))
    kp.num_mel_bins, kp.num_ceps = 80, 0
    cfg_k = ss.KaldiConfig(kp)
    pool_k = torch.randn((P, 320), device="cuda").mul_(0.1)
    out_k, en_k = torch.empty((cap, 80), device="cuda"), torch.empty((cap,), device="cuda")

    def kaldi():
        t = nxt()
        _lib.check(lib.ss_kstream_fbank_packed_device(cfg_k.handle, t["x"].data_ptr(), N, t["so"].data_ptr(), t["ro"].data_ptr(), t["rows"],
                                                      t["slots"].data_ptr(), P, pool_k.data_ptr(), out_k.data_ptr(), en_k.data_ptr(), sp))

    res["kaldi_fbank80"] = timed(kaldi, args.reps)

    # what a caller does without the pool: a per-stream loop of the dense call over carried samples ++ chunk
    cfg_b, S_b, _ = nemo_cfg(80)
    pool_b = torch.randn((P, S_b), device="cuda").mul_(0.1)
    out_b = torch.empty((cap + N * (S_b // STEP + 1), 80), device="cuda")

    def per_stream():
        t = nxt()
        so, slots = t["so_host"], t["slots_host"]
        row = 0
        for i in range(N):
            both = torch.cat([pool_b[int(slots[i])], t["x"][int(so[i]):int(so[i + 1])]])
            _lib.check(lib.ss_nemo_log_mel_device(cfg_b.handle, both.data_ptr(), 1, both.numel(), both.numel(), out_b[row:].data_ptr(), sp))
            pool_b[int(slots[i])] = both[both.numel() - S_b:]
            row += both.numel() // STEP

    res["per_stream"] = timed(per_stream, args.loop_reps)
    res["per_stream"]["reps"] = args.loop_reps
    res["nemo80_over_kaldi_fbank80_us"] = res["nemo80"]["median_us_per_call"] / res["kaldi_fbank80"]["median_us_per_call"]
    res["nemo80_over_per_stream"] = res["nemo80"]["rows_per_s"] / res["per_stream"]["rows_per_s"]
    print(json.dumps(res))
    for k, v in res.items():
        if isinstance(v, dict):
            print(f"{k}: {v['median_us_per_call']:.1f} us [{v['min_us']:.1f}, {v['max_us']:.1f}] per call, {v['rows_per_call']:.0f} rows, {v['kernel']}",
                  file=sys.stderr)


if __name__ == "__main__":
    main()
