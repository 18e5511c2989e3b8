"""µs per call of the time-axis delta features: ss_add_deltas_packed_device on a packed block, and ss_add_deltas_stream_packed_device
over a pool of stream states beside the MFCC pool call and the causal CMVN pool call it chains behind, all from one process.

    python tools/add_deltas_rate.py [--clips 1024] [--pool 4096] [--active 1024] [--max-hops 4] [--order 2] [--window 2]
                                    [--reps 100] [--rounds 7] [--ring 8] [--loop-streams 64]

Packed workload: `--clips` clips of 1 .. 16 s (98 .. 1598 rows at 100 rows/s, uniform), cols = 13 and 40 -- the packed-post shape.
bytes_per_call is vec once plus out once ((order + 2) * rows * cols * 4); hbm_fraction reads it against 8.0 TB/s (the spec peak; a
float4 copy reaches about 79 % of it).
Pool workload: a pool of `--pool` streams of which `--active` deliver 1 .. `--max-hops` rows in a tick (uniform), in random slot
order, every stream in steady state (a full history in its pool row); cols = 13 and 40.  per_stream_loop is the same tick served
by the packed call once per stream on that stream's 2L history rows plus its new rows -- what a caller without the pool call would
launch; it is timed on `--loop-streams` streams and scaled to `--active` (over_pool_call = loop / pool call).
Protocol: every leg is warmed up, then `--rounds` rounds alternate the legs, each timed with HIP events around `--reps` back-to-back
calls on one stream; every call takes the next tick of a ring of `--ring` pre-built inputs, so no call repeats the inputs of the one
before it.  Reported per leg: the median over the rounds, the fastest and the slowest round.
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

STEP, S, NCEP, CMVN_WIN = 160, 160, 13, 301
HBM_PEAK = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=1024)
    ap.add_argument("--pool", type=int, default=4096)
    ap.add_argument("--active", type=int, default=1024)
    ap.add_argument("--max-hops", type=int, default=4)
    ap.add_argument("--order", type=int, default=2)
    ap.add_argument("--window", type=int, default=2)
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--ring", type=int, default=8)
    ap.add_argument("--loop-streams", type=int, default=64)
    args = ap.parse_args()

    import numpy as np
    import torch

    import speechsauce_amd as ss
    from speechsauce_amd import _lib

    lib = _lib.lib()
    P, N, H, O, W = args.pool, args.active, args.max_hops, args.order, args.window
    L = O * W
    sp = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    cfg = ss.SpeechConfig(_lib.make_params())
    rng = np.random.default_rng(0)
    cols_set = (13, 40)

    # ---- packed: two blocks per column count, alternated ----
    lens = rng.integers(98, 1599, args.clips)
    off = np.zeros(args.clips + 1, np.int64)
    np.cumsum(lens, out=off[1:])
    rows_packed = int(off[-1])
    d_off = torch.from_numpy(off).cuda()
    pk_in = {c: [torch.randn((rows_packed, c), device="cuda").mul_(3).add_(1) for _ in range(2)] for c in cols_set}
    pk_out = {c: torch.empty((rows_packed, (O + 1) * c), device="cuda") for c in cols_set}
    flip = [0]

    def packed(c):
        def call():
            flip[0] ^= 1
            _lib.check(lib.ss_add_deltas_packed_device(pk_in[c][flip[0]].data_ptr(), args.clips, d_off.data_ptr(), rows_packed, c, O, W,
                                                       pk_out[c].data_ptr(), sp))
        return call

    # ---- pool: a ring of ticks ----
    cap = N * H
    ticks = []
    for _ in range(args.ring):
        hops = rng.integers(1, H + 1, N)
        slots = rng.permutation(P)[:N].astype(np.int32)
        so = np.zeros(N + 1, np.int64)
        np.cumsum(hops * STEP, out=so[1:])
        rows = int(hops.sum())
        ticks.append({"rows": rows, "x": torch.randn(int(so[-1]), device="cuda").mul_(0.1), "so": torch.from_numpy(so).cuda(),
                      "ro": torch.from_numpy(so // STEP).cuda(), "slots": torch.from_numpy(slots).cuda(),
                      "feat": {c: torch.randn((rows, c), device="cuda").mul_(3).add_(1) for c in cols_set}})
    at = [0]

    def nxt():
        at[0] += 1
        return ticks[at[0] % args.ring]

    fpool = torch.randn((P, S), device="cuda").mul_(0.1)
    fout = torch.empty((cap, NCEP), device="cuda")
    cpool, cout, dpool, dout = {}, {}, {}, {}
    for c in cols_set:
        n = C.c_size_t()
        _lib.check(lib.ss_cmvn_stream_state_len(c, CMVN_WIN, C.byref(n)))
        cpool[c] = torch.randn((P, n.value), device="cuda").mul_(3).add_(1)
        cpool[c][:, -1] = CMVN_WIN - 1  # steady state: every stream has a full window of history
        cout[c] = torch.empty((cap, c), device="cuda")
        _lib.check(lib.ss_add_deltas_stream_state_len(c, O, W, C.byref(n)))
        dpool[c] = torch.randn((P, n.value), device="cuda").mul_(3).add_(1)
        dpool[c][:, -1] = 2 * L  # steady state: 2L rows of history
        dout[c] = torch.empty((cap, (O + 1) * c), device="cuda")

    def mfcc():
        t = nxt()
        _lib.check(lib.ss_mfcc_stream_packed_device(cfg.handle, t["x"].data_ptr(), N, t["so"].data_ptr(), t["ro"].data_ptr(), t["rows"],
                                                    t["slots"].data_ptr(), P, 100, fpool.data_ptr(), fout.data_ptr(), sp))

    def cmvn(c):
        def call():
            t = nxt()
            _lib.check(lib.ss_cmvn_stream_packed_device(t["feat"][c].data_ptr(), N, t["ro"].data_ptr(), t["rows"], t["slots"].data_ptr(), P, c,
                                                        CMVN_WIN, 0, cpool[c].data_ptr(), cout[c].data_ptr(), sp))
        return call

    def deltas(c):
        def call():
            t = nxt()
            _lib.check(lib.ss_add_deltas_stream_packed_device(t["feat"][c].data_ptr(), N, t["ro"].data_ptr(), t["rows"], t["slots"].data_ptr(), P, c,
                                                              O, W, dpool[c].data_ptr(), dout[c].data_ptr(), sp))
        return call

    # the per-stream loop: one packed call per stream on [2L history rows | new rows] (the copy that assembles it is not timed)
    M = min(args.loop_streams, N)
    loop_in = {c: torch.randn((M, 2 * L + H, c), device="cuda") for c in cols_set}
    loop_out = {c: torch.empty((M, 2 * L + H, (O + 1) * c), device="cuda") for c in cols_set}
    loop_off = torch.tensor([0, 2 * L + H], dtype=torch.int64, device="cuda")

    def loop(c):
        def call():
            for i in range(M):
                _lib.check(lib.ss_add_deltas_packed_device(loop_in[c][i].data_ptr(), 1, loop_off.data_ptr(), 2 * L + H, c, O, W,
                                                           loop_out[c][i].data_ptr(), sp))
        return call

    legs = ([(f"packed_cols{c}", packed(c), args.reps) for c in cols_set] + [("mfcc_pool", mfcc, args.reps)]
            + [(f"cmvn_pool_cols{c}", cmvn(c), args.reps) for c in cols_set] + [(f"deltas_pool_cols{c}", deltas(c), args.reps) for c in cols_set]
            + [(f"per_stream_loop_cols{c}", loop(c), max(args.reps // 20, 2)) for c in cols_set])

    def timed(fn, reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / reps * 1e3

    for _, fn, _ in legs:  # warm-up: code objects, every tick of the ring once
        for _ in range(args.ring):
            fn()
    torch.cuda.synchronize()
    us = {name: [] for name, _, _ in legs}
    for _ in range(args.rounds):
        for name, fn, reps in legs:
            us[name].append(timed(fn, reps))
    mean_rows = sum(t["rows"] for t in ticks) / len(ticks)
    res = {"clips": args.clips, "rows_packed": rows_packed, "pool": P, "active": N, "max_hops": H, "order": O, "window": W, "reps": args.reps,
           "rounds": args.rounds, "ring": args.ring, "rows_per_pool_call": mean_rows, "loop_streams": M, "device": torch.cuda.get_device_name(),
           "mfcc_kernel": lib.ss_last_kernel_name().decode()}
    for name, _, _ in legs:
        v = us[name]
        res[name] = {"us_per_call_median": statistics.median(v), "us_min": min(v), "us_max": max(v)}
    for c in cols_set:
        leg = res[f"packed_cols{c}"]
        leg["bytes_per_call"] = (O + 2) * rows_packed * c * 4
        leg["gb_per_s"] = leg["bytes_per_call"] / leg["us_per_call_median"] * 1e-3
        leg["hbm_fraction"] = leg["gb_per_s"] * 1e9 / HBM_PEAK
        leg = res[f"deltas_pool_cols{c}"]
        leg["bytes_per_call"] = int((O + 2) * mean_rows * c * 4 + 2 * N * (2 * L * c + 1) * 4)  # vec + out, and the named pool rows read and written
        leg["over_mfcc_pool"] = leg["us_per_call_median"] / res["mfcc_pool"]["us_per_call_median"]
        leg["over_cmvn_pool"] = leg["us_per_call_median"] / res[f"cmvn_pool_cols{c}"]["us_per_call_median"]
        lp = res[f"per_stream_loop_cols{c}"]
        lp["us_scaled_to_active"] = lp["us_per_call_median"] * N / M
        lp["over_pool_call"] = lp["us_scaled_to_active"] / leg["us_per_call_median"]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
