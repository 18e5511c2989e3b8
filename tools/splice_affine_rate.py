"""µs per call of the fused splice + affine transform: ss_affine_splice_packed_device on a packed block beside what a user runs
without it -- ss_splice_packed_device followed by torch.addmm in float32 on the spliced block -- and beside that product alone on a
spliced block built beforehand, all from one process.

    python tools/splice_affine_rate.py [--clips 1024] [--reps 20] [--rounds 7] [--ring 4]

Workload: the block of tools/splice_rate.py, `--clips` clips of 1 .. 16 s (98 .. 1598 rows at 100 rows/s, uniform; about 891 k rows).
Shapes (cols, left, right, stride, out_dim): (40, 5, 5, 1, 40) -- splice-feats +-5 then a 40 x 440 LDA -- and (80, 3, 3, 6, 256) -- low
frame rate 7 / 6 then a 256 x 560 input projection.  flop_per_call is 2 * out_rows * K4 * (out_dim padded to tiles of 16), what the
kernel issues; mfma_fraction reads it against 155 TF (the f32 matrix rate: 256 CUs x 4 SIMDs x 64 FLOP/clk x 2.4 GHz).
Legs: fused (ours); splice_addmm (a): the splice call, then torch.addmm(bias, spliced, M^T); addmm (b): (a)'s product alone.
Protocol: every leg is warmed up, then `--rounds` rounds alternate the legs, each timed with HIP events around `--reps` back-to-back
calls on one stream; every call takes the next of a ring of `--ring` pre-built input blocks.  Reported per leg: the median over the
rounds, the fastest and the slowest round.
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

MFMA_F32_PEAK = 155e12
SHAPES = ((40, 5, 5, 1, 40), (80, 3, 3, 6, 256))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--ring", type=int, default=4)
    args = ap.parse_args()

    import numpy as np
    import torch

    import speechsauce_amd as ss
    from speechsauce_amd import _lib

    lib = _lib.lib()
    sp = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rng = np.random.default_rng(0)
    lens = rng.integers(98, 1599, args.clips)
    ro = np.zeros(args.clips + 1, np.int64)
    np.cumsum(lens, out=ro[1:])
    rows = int(ro[-1])
    d_ro = torch.from_numpy(ro).cuda()
    at = [0]
    legs, meta, keep = [], {}, []
    for cols, left, right, stride, out_dim in SHAPES:
        K = (left + 1 + right) * cols
        oo = np.zeros_like(ro)
        _lib.check(lib.ss_splice_packed_offsets(args.clips, ro.ctypes.data, stride, oo.ctypes.data))
        out_rows = int(oo[-1])
        d_oo = torch.from_numpy(oo).cuda()
        M = (rng.standard_normal((out_dim, K)) / np.sqrt(K)).astype(np.float32)
        bias = rng.standard_normal(out_dim).astype(np.float32)
        t = ss.Affine(M, bias)
        keep.append(t)
        d_mt, d_bias = torch.from_numpy(M).cuda().t().contiguous(), torch.from_numpy(bias).cuda()
        ring = [torch.randn((rows, cols), device="cuda").mul_(3).add_(1) for _ in range(args.ring)]
        spliced = torch.empty((out_rows, K), device="cuda")
        out = torch.empty((out_rows, out_dim), device="cuda")
        tag = f"cols{cols}_l{left}r{right}s{stride}_out{out_dim}"
        meta[tag] = {"out_rows": out_rows, "K4": t.chain_len, "flop_per_call": 2 * out_rows * t.chain_len * (-(-out_dim // 16) * 16),
                     "spliced_bytes": out_rows * K * 4}

        def nxt(ring=ring):
            at[0] += 1
            return ring[at[0] % args.ring]

        def splice(x, d_oo=d_oo, out_rows=out_rows, cols=cols, left=left, right=right, stride=stride, spliced=spliced):
            _lib.check(lib.ss_splice_packed_device(x.data_ptr(), args.clips, d_ro.data_ptr(), rows, d_oo.data_ptr(), out_rows, cols, left, right, stride,
                                                   spliced.data_ptr(), sp))

        def fused(nxt=nxt, t=t, d_oo=d_oo, out_rows=out_rows, cols=cols, left=left, right=right, stride=stride, out=out):
            _lib.check(lib.ss_affine_splice_packed_device(t.handle, nxt().data_ptr(), args.clips, d_ro.data_ptr(), rows, d_oo.data_ptr(), out_rows, cols,
                                                          left, right, stride, out.data_ptr(), sp))

        def addmm(spliced=spliced, d_mt=d_mt, d_bias=d_bias, out=out):
            torch.addmm(d_bias, spliced, d_mt, out=out)

        def splice_addmm(nxt=nxt, splice=splice, addmm=addmm):
            splice(nxt())
            addmm()

        splice(ring[0])  # (b)'s block
        legs += [(f"fused_{tag}", fused), (f"splice_addmm_{tag}", splice_addmm), (f"addmm_{tag}", addmm)]

    def timed(fn, reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / reps * 1e3

    for _, fn in legs:  # warm-up: code objects, the handle's table, every input of the ring once
        for _ in range(args.ring):
            fn()
    torch.cuda.synchronize()
    us = {name: [] for name, _ in legs}
    for _ in range(args.rounds):
        for name, fn in legs:
            us[name].append(timed(fn, args.reps))
    res = {"clips": args.clips, "rows": rows, "reps": args.reps, "rounds": args.rounds, "ring": args.ring, "device": torch.cuda.get_device_name()}
    for name, _ in legs:
        v = us[name]
        res[name] = {"us_per_call_median": statistics.median(v), "us_min": min(v), "us_max": max(v)}
    for tag, m in meta.items():
        f = res[f"fused_{tag}"]
        f.update(m)
        f["mfma_fraction"] = m["flop_per_call"] / (f["us_per_call_median"] * 1e-6) / MFMA_F32_PEAK
        f["over_splice_addmm"] = f["us_per_call_median"] / res[f"splice_addmm_{tag}"]["us_per_call_median"]
        f["over_addmm"] = f["us_per_call_median"] / res[f"addmm_{tag}"]["us_per_call_median"]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
