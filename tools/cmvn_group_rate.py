"""µs per call of grouped CMVN (ss_cmvn_stats_packed_device, ss_cmvn_apply_packed_device, ss_cmvn_grouped_packed_device) beside
ss_cmvn_packed_device with variance normalisation -- the nearest existing kernel -- and a torch restatement, all from one process.

    python tools/cmvn_group_rate.py [--clips 1024] [--cols 13 40 80] [--groups 1 64 1024] [--reps 50] [--rounds 10]

Workload: `--clips` clips of 1 .. 16 s (98 .. 1598 rows at 100 rows/s, uniform: about 891 k rows for 1024 clips), clip b in group
b % n_groups.  Legs per (cols, n_groups): stats (into a block that is zeroed outside the timed window every round), apply, and the
combined call; per cols: cmvn_packed with variance on, the torch restatement (f64 index_add_ of x and x^2 over repeat_interleave'd
group ids, then the broadcast apply: what a caller without these calls would write) at the middle n_groups, and fold_probe -- the
statistics call on `--clips` one-row clips in ONE group, where the per-clip pass has next to nothing to do, so that the call is its
launches plus the serial fold of `--clips` merges per column: the floor under the global case.
bytes: stats reads the block once, apply and cmvn_packed read it once and write it once (cmvn_packed really reads it twice; the
second read is served by the caches), the combined call reads it twice and writes it once but is charged the algorithmic
read-once-write-once too; hbm_fraction reads them against 8.0 TB/s (the spec peak; a float4 copy reaches about 79 % of it).
Protocol: every leg is warmed up, then `--rounds` windows alternate the legs, each timed with HIP events around `--reps` back-to-back
calls on one stream; consecutive calls take alternating input blocks.  Reported per leg: the median over the windows, the fastest
and the slowest.  Prints one JSON line.  Measuring only: not collected by pytest, not part of bench.py.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mfcc-rust_amd"))

HBM_PEAK = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=1024)
    ap.add_argument("--cols", type=int, nargs="+", default=[13, 40, 80])
    ap.add_argument("--groups", type=int, nargs="+", default=[1, 64, 1024])
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=10)
    args = ap.parse_args()

    import ctypes as C

    import numpy as np
    import torch

    from speechsauce_amd import _lib

    lib = _lib.lib()
    sp = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rng = np.random.default_rng(0)
    n = args.clips
    lens = rng.integers(98, 1599, n)
    off = np.zeros(n + 1, np.int64)
    np.cumsum(lens, out=off[1:])
    rows = int(off[-1])
    d_off = torch.from_numpy(off).cuda()
    d_off1 = torch.arange(n + 1, dtype=torch.int64, device="cuda")  # fold_probe: one row per clip
    grp = {g: torch.from_numpy((np.arange(n) % g).astype(np.int32)).cuda() for g in args.groups}
    row_grp = {g: torch.repeat_interleave(grp[g].long(), torch.from_numpy(lens).cuda()) for g in args.groups}
    flip = [0]
    legs, zero = [], []

    def block(c):
        return [torch.randn((rows, c), device="cuda").mul_(3).add_(1) for _ in range(2)]

    def nxt(x):
        flip[0] ^= 1
        return x[flip[0]]

    for c in args.cols:
        x, out, L = block(c), torch.empty((rows, c), device="cuda"), 2 * c + 1

        def packed(x=x, out=out, c=c):
            _lib.check(lib.ss_cmvn_packed_device(nxt(x).data_ptr(), n, d_off.data_ptr(), rows, c, 1, out.data_ptr(), sp))

        legs.append((f"cmvn_packed_cols{c}", packed, c, 2))
        probe = torch.zeros((1, L), dtype=torch.float64, device="cuda")
        zero.append(probe)

        def fold_probe(x=x, probe=probe, c=c):
            _lib.check(lib.ss_cmvn_stats_packed_device(nxt(x).data_ptr(), n, d_off1.data_ptr(), n, c, None, 1, probe.data_ptr(), sp))

        legs.append((f"fold_probe_cols{c}", fold_probe, c, 0))
        for g in args.groups:
            st = torch.zeros((g, L), dtype=torch.float64, device="cuda")
            zero.append(st)
            full = torch.zeros((g, L), dtype=torch.float64, device="cuda")
            _lib.check(lib.ss_cmvn_stats_packed_device(x[0].data_ptr(), n, d_off.data_ptr(), rows, c, grp[g].data_ptr(), g, full.data_ptr(), sp))

            def stats(x=x, st=st, c=c, g=g):
                _lib.check(lib.ss_cmvn_stats_packed_device(nxt(x).data_ptr(), n, d_off.data_ptr(), rows, c, grp[g].data_ptr(), g, st.data_ptr(), sp))

            def apply(x=x, full=full, out=out, c=c, g=g):
                _lib.check(lib.ss_cmvn_apply_packed_device(nxt(x).data_ptr(), n, d_off.data_ptr(), rows, c, grp[g].data_ptr(), g, full.data_ptr(), 1,
                                                           out.data_ptr(), sp))

            def grouped(x=x, out=out, c=c, g=g):
                _lib.check(lib.ss_cmvn_grouped_packed_device(nxt(x).data_ptr(), n, d_off.data_ptr(), rows, c, grp[g].data_ptr(), g, 1, out.data_ptr(), sp))

            legs += [(f"stats_cols{c}_g{g}", stats, c, 1), (f"apply_cols{c}_g{g}", apply, c, 2), (f"grouped_cols{c}_g{g}", grouped, c, 2)]
        g = args.groups[len(args.groups) // 2]

        def restated(x=x, c=c, g=g):
            v = nxt(x).double()
            s1 = torch.zeros((g, c), dtype=torch.float64, device="cuda").index_add_(0, row_grp[g], v)
            s2 = torch.zeros((g, c), dtype=torch.float64, device="cuda").index_add_(0, row_grp[g], v * v)
            cnt = torch.zeros(g, dtype=torch.float64, device="cuda").index_add_(0, grp[g].long(), d_off.diff().double())
            mean = s1 / cnt[:, None]
            inv = 1.0 / ((s2 / cnt[:, None] - mean * mean).clamp_min(0).sqrt() + 2.0 ** -30)
            return ((v - mean[row_grp[g]]) * inv[row_grp[g]]).float()

        legs.append((f"torch_index_add_cols{c}_g{g}", restated, c, 2))

    def timed(fn, reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / reps * 1e3

    for _, fn, _, _ in legs:
        for _ in range(4):
            fn()
    torch.cuda.synchronize()
    us = {name: [] for name, _, _, _ in legs}
    for _ in range(args.rounds):
        for name, fn, _, _ in legs:
            for z in zero:  # statistics accumulate: every window starts from fresh blocks (outside the timed region)
                z.zero_()
            reps = max(args.reps // 10, 2) if name.startswith("torch") else args.reps
            us[name].append(timed(fn, reps))
    res = {"clips": n, "rows": rows, "reps": args.reps, "rounds": args.rounds, "device": torch.cuda.get_device_name()}
    for name, _, c, passes in legs:
        v = us[name]
        leg = {"us_per_call_median": statistics.median(v), "us_min": min(v), "us_max": max(v)}
        if passes:
            leg["bytes_per_call"] = passes * rows * c * 4
            leg["hbm_fraction"] = leg["bytes_per_call"] / (leg["us_per_call_median"] * 1e-6) / HBM_PEAK
        res[name] = leg
    print(json.dumps(res))


if __name__ == "__main__":
    main()
