"""µs per call of the causal CMVN over a pool of stream states (ss_cmvn_stream_packed_device) beside the ragged streaming MFCC call
whose rows it normalises (ss_mfcc_stream_packed_device), both from one process.

    python tools/cmvn_stream_rate.py [--pool 4096] [--active 1024] [--max-hops 4] [--win 301] [--reps 200] [--rounds 7] [--ring 16]

Workload: a pool of `--pool` streams of which `--active` deliver 1 .. `--max-hops` rows in a tick (uniform), in random slot order,
every stream in steady state (a full window of history in its pool row).  cols = 13 and 40, variance normalisation off and on.
Protocol: every leg is warmed up, then `--rounds` rounds alternate the legs -- the MFCC call, then the four CMVN shapes -- each
timed with HIP events around `--reps` back-to-back calls on one stream; every call takes the next tick of a ring of `--ring`
pre-built ticks (rows, tables, slots), so no call repeats the inputs of the one before it.  Reported per leg: the median over the
rounds, the fastest and the slowest round.  bytes_pool_per_call is what the call must move for the advance of the named pool rows
(each read once and written once), the floor its time is to be read against.
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

STEP, S, NCEP = 160, 160, 13


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pool", type=int, default=4096)
    ap.add_argument("--active", type=int, default=1024)
    ap.add_argument("--max-hops", type=int, default=4)
    ap.add_argument("--win", type=int, default=301)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--ring", type=int, default=16)
    args = ap.parse_args()

    import numpy as np
    import torch

    import speechsauce_amd as ss
    from speechsauce_amd import _lib

    lib = _lib.lib()
    P, N, H, W = args.pool, args.active, args.max_hops, args.win
    sp = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    cfg = ss.SpeechConfig(_lib.make_params())
    rng = np.random.default_rng(0)
    cap = N * H
    shapes = [(13, 0), (13, 1), (40, 0), (40, 1)]

    ticks = []
    for _ in range(args.ring):
        hops = rng.integers(1, H + 1, N)
        slots = rng.permutation(P)[:N].astype(np.int32)
        so = np.zeros(N + 1, np.int64)
        np.cumsum(hops * STEP, out=so[1:])
        rows = int(hops.sum())
        ticks.append({"rows": rows, "x": torch.randn(int(so[-1]), device="cuda").mul_(0.1), "so": torch.from_numpy(so).cuda(),
                      "ro": torch.from_numpy(so // STEP).cuda(), "slots": torch.from_numpy(slots).cuda(),
                      "feat": {c: torch.randn((rows, c), device="cuda").mul_(3).add_(1) for c in (13, 40)}})
    at = [0]

    def nxt():
        at[0] += 1
        return ticks[at[0] % args.ring]

    fpool = torch.randn((P, S), device="cuda").mul_(0.1)
    fout = torch.empty((cap, NCEP), device="cuda")
    cpool, cout = {}, {}
    for c in (13, 40):
        L = C.c_size_t()
        _lib.check(lib.ss_cmvn_stream_state_len(c, W, C.byref(L)))
        cpool[c] = torch.randn((P, L.value), device="cuda").mul_(3).add_(1)
        cpool[c][:, -1] = W - 1  # steady state: every stream has a full window of history
        cout[c] = torch.empty((cap, c), device="cuda")

    def mfcc():
        t = nxt()
        _lib.check(lib.ss_mfcc_stream_packed_device(cfg.handle, t["x"].data_ptr(), N, t["so"].data_ptr(), t["ro"].data_ptr(), t["rows"],
                                                    t["slots"].data_ptr(), P, 100, fpool.data_ptr(), fout.data_ptr(), sp))

    def cmvn(c, var):
        def call():
            t = nxt()
            _lib.check(lib.ss_cmvn_stream_packed_device(t["feat"][c].data_ptr(), N, t["ro"].data_ptr(), t["rows"], t["slots"].data_ptr(), P, c, W,
                                                        var, cpool[c].data_ptr(), cout[c].data_ptr(), sp))
        return call

    legs = [("mfcc_pool", mfcc)] + [(f"cmvn_cols{c}_var{v}", cmvn(c, v)) for c, v in shapes]

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / args.reps * 1e3

    for _, fn in legs:  # warm-up: code objects, every tick of the ring once
        for _ in range(args.ring):
            fn()
    torch.cuda.synchronize()
    us = {name: [] for name, _ in legs}
    for _ in range(args.rounds):
        for name, fn in legs:
            us[name].append(timed(fn))
    mean_rows = sum(t["rows"] for t in ticks) / len(ticks)
    res = {"pool": P, "active": N, "max_hops": H, "win": W, "reps": args.reps, "rounds": args.rounds, "ring": args.ring,
           "rows_per_call": mean_rows, "device": torch.cuda.get_device_name(), "mfcc_kernel": lib.ss_last_kernel_name().decode()}
    for name, _ in legs:
        v = us[name]
        res[name] = {"us_per_call_median": statistics.median(v), "us_min": min(v), "us_max": max(v)}
    for c, v in shapes:
        leg = res[f"cmvn_cols{c}_var{v}"]
        leg["bytes_pool_per_call"] = 2 * N * ((W - 1) * c + 1) * 4
        leg["pool_gb_per_s"] = leg["bytes_pool_per_call"] / leg["us_per_call_median"] * 1e-3
        leg["over_mfcc_pool"] = leg["us_per_call_median"] / res["mfcc_pool"]["us_per_call_median"]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
