"""µs per call of frame splicing and subsampling: ss_splice_packed_device on a packed block beside the torch gather a user writes
without it, and ss_splice_stream_packed_device over a pool of stream states beside the MFCC pool call and the add-deltas pool call on
the same tables, all from one process.

    python tools/splice_rate.py [--clips 1024] [--pool 4096] [--active 1024] [--max-periods 4] [--reps 50] [--rounds 7] [--ring 8]

Packed workload: `--clips` clips of 1 .. 16 s (98 .. 1598 rows at 100 rows/s, uniform; about 891 k rows), cols = 40 and 80, the
parameter sets (left, right, stride) = (5, 5, 1) -- splice-feats +-5 -- and (3, 3, 6) -- low frame rate 7 / 6.  bytes_per_call is vec
once plus out once; hbm_fraction reads it against 8.0 TB/s (the spec peak; a float4 copy reaches about 79 % of it).  torch_gather is
`rows[idx].reshape(T_out, W * cols)` with the clamped index tensor [T_out, W] built outside the timed region.
Pool workload: a pool of `--pool` streams of which `--active` deliver 1 .. `--max-periods` periods in a tick (uniform), in random
slot order, every stream in steady state (a full history in its pool row); cols = 40, both parameter sets; the MFCC pool call and the
add-deltas pool call (order 2, window 2) run on the tables of the stride-1 ticks.
Protocol: every leg is warmed up, then `--rounds` rounds alternate the legs, each timed with HIP events around `--reps` back-to-back
calls on one stream; every call takes the next of a ring of `--ring` pre-built inputs, so no call repeats the inputs of the one before
it.  Reported per leg: the median over the rounds, the fastest and the slowest round.
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
HBM_PEAK = 8.0e12
SETS = ((5, 5, 1), (3, 3, 6))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=1024)
    ap.add_argument("--pool", type=int, default=4096)
    ap.add_argument("--active", type=int, default=1024)
    ap.add_argument("--max-periods", type=int, default=4)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--ring", type=int, default=8)
    args = ap.parse_args()

    import numpy as np
    import torch

    import speechsauce_amd as ss
    from speechsauce_amd import _lib

    lib = _lib.lib()
    P, N, H = args.pool, args.active, args.max_periods
    sp = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    cfg = ss.SpeechConfig(_lib.make_params())
    rng = np.random.default_rng(0)

    # ---- packed: two input blocks per column count, alternated ----
    lens = rng.integers(98, 1599, args.clips)
    ro = np.zeros(args.clips + 1, np.int64)
    np.cumsum(lens, out=ro[1:])
    rows_packed = int(ro[-1])
    d_ro = torch.from_numpy(ro).cuda()
    cols_set = (40, 80)
    pk_in = {c: [torch.randn((rows_packed, c), device="cuda").mul_(3).add_(1) for _ in range(2)] for c in cols_set}
    flip = [0]
    legs, packed_bytes = [], {}
    for left, right, stride in SETS:
        W = left + 1 + right
        oo = np.zeros_like(ro)
        _lib.check(lib.ss_splice_packed_offsets(args.clips, ro.ctypes.data, stride, oo.ctypes.data))
        out_rows = int(oo[-1])
        d_oo = torch.from_numpy(oo).cuda()
        # the gather a user writes today: per output row the W clamped source rows
        idx = np.concatenate([ro[b] + np.clip(np.arange(0, n, stride)[:, None] + np.arange(-left, right + 1)[None, :], 0, n - 1)
                              for b, n in enumerate(lens)])
        d_idx = torch.from_numpy(idx).cuda()
        for c in cols_set:
            out = torch.empty((out_rows, W * c), device="cuda")
            tag = f"l{left}r{right}s{stride}_cols{c}"
            packed_bytes[tag] = (rows_packed * c + out_rows * W * c) * 4

            def ours(c=c, d_oo=d_oo, out=out, left=left, right=right, stride=stride, out_rows=out_rows):
                flip[0] ^= 1
                _lib.check(lib.ss_splice_packed_device(pk_in[c][flip[0]].data_ptr(), args.clips, d_ro.data_ptr(), rows_packed, d_oo.data_ptr(), out_rows,
                                                       c, left, right, stride, out.data_ptr(), sp))

            def gather(c=c, d_idx=d_idx, out_rows=out_rows, W=W):
                flip[0] ^= 1
                return pk_in[c][flip[0]][d_idx].reshape(out_rows, W * c)

            legs += [(f"packed_{tag}", ours, args.reps), (f"torch_gather_{tag}", gather, args.reps)]

    # ---- pool: a ring of ticks per stride ----
    c = 40
    ticks = {}
    for stride in sorted({s for _, _, s in SETS}):
        ticks[stride] = []
        for _ in range(args.ring):
            periods = rng.integers(1, H + 1, N)
            slots = rng.permutation(P)[:N].astype(np.int32)
            rows = periods * stride
            r = np.zeros(N + 1, np.int64)
            np.cumsum(rows, out=r[1:])
            total = int(r[-1])
            ticks[stride].append({"rows": total, "ro": torch.from_numpy(r).cuda(), "so": torch.from_numpy(r * STEP).cuda(),
                                  "slots": torch.from_numpy(slots).cuda(), "feat": torch.randn((total, c), device="cuda").mul_(3).add_(1),
                                  "x": torch.randn(total * STEP, device="cuda").mul_(0.1) if stride == 1 else None})
    at = [0]

    def nxt(stride):
        at[0] += 1
        return ticks[stride][at[0] % args.ring]

    cap = N * H * max(s for _, _, s in SETS)
    fpool = torch.randn((P, S), device="cuda").mul_(0.1)
    fout = torch.empty((cap, NCEP), device="cuda")
    n = C.c_size_t()
    _lib.check(lib.ss_add_deltas_stream_state_len(c, 2, 2, C.byref(n)))
    dpool = torch.randn((P, n.value), device="cuda").mul_(3).add_(1)
    dpool[:, -1] = 8  # steady state: 2L rows of history
    dout = torch.empty((cap, 3 * c), device="cuda")

    def mfcc():
        t = nxt(1)
        _lib.check(lib.ss_mfcc_stream_packed_device(cfg.handle, t["x"].data_ptr(), N, t["so"].data_ptr(), t["ro"].data_ptr(), t["rows"],
                                                    t["slots"].data_ptr(), P, 100, fpool.data_ptr(), fout.data_ptr(), sp))

    def deltas():
        t = nxt(1)
        _lib.check(lib.ss_add_deltas_stream_packed_device(t["feat"].data_ptr(), N, t["ro"].data_ptr(), t["rows"], t["slots"].data_ptr(), P, c, 2, 2,
                                                          dpool.data_ptr(), dout.data_ptr(), sp))

    legs += [("mfcc_pool", mfcc, args.reps), ("deltas_pool_cols40", deltas, args.reps)]
    pool_bytes = {}
    for left, right, stride in SETS:
        W = left + 1 + right
        d = C.c_size_t()
        _lib.check(lib.ss_splice_stream_state_len(c, left, right, stride, C.byref(n), C.byref(d)))
        spool = torch.randn((P, n.value), device="cuda").mul_(3).add_(1)
        spool[:, -1] = (n.value - 1) // c  # steady state: H rows of history
        sout = torch.empty((N * H, W * c), device="cuda")
        tag = f"splice_pool_l{left}r{right}s{stride}_cols{c}"
        mean_rows = sum(t["rows"] for t in ticks[stride]) / args.ring
        pool_bytes[tag] = int((mean_rows * c + mean_rows / stride * W * c + 2 * N * n.value) * 4)  # vec + out, the named pool rows read and written

        def splice(left=left, right=right, stride=stride, spool=spool, sout=sout):
            t = nxt(stride)
            _lib.check(lib.ss_splice_stream_packed_device(t["feat"].data_ptr(), N, t["ro"].data_ptr(), t["rows"], t["slots"].data_ptr(), P, c, left,
                                                          right, stride, spool.data_ptr(), sout.data_ptr(), sp))

        legs.append((tag, splice, args.reps))

    def timed(fn, reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / reps * 1e3

    for _, fn, _ in legs:  # warm-up: code objects, every input of the ring once
        for _ in range(args.ring):
            fn()
    torch.cuda.synchronize()
    us = {name: [] for name, _, _ in legs}
    for _ in range(args.rounds):
        for name, fn, reps in legs:
            us[name].append(timed(fn, reps))
    res = {"clips": args.clips, "rows_packed": rows_packed, "pool": P, "active": N, "max_periods": H, "reps": args.reps, "rounds": args.rounds,
           "ring": args.ring, "device": torch.cuda.get_device_name()}
    for name, _, _ in legs:
        v = us[name]
        res[name] = {"us_per_call_median": statistics.median(v), "us_min": min(v), "us_max": max(v)}
    for tag, nbytes in packed_bytes.items():
        for leg in (res[f"packed_{tag}"], res[f"torch_gather_{tag}"]):
            leg["bytes_per_call"] = nbytes
            leg["gb_per_s"] = nbytes / leg["us_per_call_median"] * 1e-3
            leg["hbm_fraction"] = leg["gb_per_s"] * 1e9 / HBM_PEAK
        res[f"torch_gather_{tag}"]["over_packed"] = res[f"torch_gather_{tag}"]["us_per_call_median"] / res[f"packed_{tag}"]["us_per_call_median"]
    for tag, nbytes in pool_bytes.items():
        res[tag]["bytes_per_call"] = nbytes
        res[tag]["over_mfcc_pool"] = res[tag]["us_per_call_median"] / res["mfcc_pool"]["us_per_call_median"]
        res[tag]["over_deltas_pool"] = res[tag]["us_per_call_median"] / res["deltas_pool_cols40"]["us_per_call_median"]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
