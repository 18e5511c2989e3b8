"""µs per call of the padded-batch collation: ss_pad_packed_device on a packed block beside what a user writes without it, with the
lengths already known on the host -- `pad_sequence(torch.split(x, lens), batch_first=True)`, `.transpose(1, 2)` for channels first,
`.to(dtype).contiguous()` -- from one process.

    python tools/pad_rate.py [--clips 1024] [--reps 20] [--torch-reps 5] [--rounds 5] [--ring 2]

Workload: `--clips` clips of 1 .. 16 s (98 .. 1598 rows at 100 rows/s, uniform; about 868 k rows), cols = 80 (fbank) and 240 (spliced),
max_rows = the longest clip (what pad_sequence pads to), pad_value 0; the configurations btc float32, btc bfloat16 and bct bfloat16.
bytes_per_call is the kept rows of vec once plus out once; hbm_fraction reads it against 8.0 TB/s (the spec peak; a float4 copy reaches
about 79 % of it).  Before anything is timed every configuration's result is compared with the baseline's (torch.equal: the rows are
finite).
Protocol: every leg is warmed up, then `--rounds` rounds alternate the legs, each timed with HIP events around back-to-back calls on
one stream; every call takes the next of a ring of `--ring` input blocks and output buffers.  At the default size one call's input and
output together are 0.5 GiB and more, twice the 256 MiB Infinity Cache, so no call finds its rows in a cache.  Reported per leg: the
median over the rounds, the fastest and the slowest round.
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

HBM_PEAK = 8.0e12
CONFIGS = (("btc", "float32"), ("btc", "bfloat16"), ("bct", "bfloat16"))
LAYOUT_CODE = {"btc": 0, "bct": 1}
DTYPE_CODE = {"float32": 0, "float16": 1, "bfloat16": 2}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--torch-reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--ring", type=int, default=2)
    args = ap.parse_args()

    import numpy as np
    import torch
    from torch.nn.utils.rnn import pad_sequence

    from speechsauce_amd import _lib

    lib = _lib.lib()
    sp = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rng = np.random.default_rng(0)
    n = args.clips
    lens = rng.integers(98, 1599, n)
    ro = np.zeros(n + 1, np.int64)
    np.cumsum(lens, out=ro[1:])
    rows, max_rows, lens_list = int(ro[-1]), int(lens.max()), [int(v) for v in lens]
    d_ro = torch.from_numpy(ro).cuda()
    d_len = torch.empty(n, dtype=torch.int32, device="cuda")
    at = [0]
    legs, nbytes = [], {}
    res = {"clips": n, "rows_packed": rows, "max_rows": max_rows, "reps": args.reps, "torch_reps": args.torch_reps, "rounds": args.rounds,
           "ring": args.ring, "device": torch.cuda.get_device_name()}
    for cols in (80, 240):
        ins = [torch.randn((rows, cols), device="cuda").mul_(3).add_(1) for _ in range(args.ring)]
        for layout, dtype in CONFIGS:
            tdt = getattr(torch, dtype)
            shape = (n, max_rows, cols) if layout == "btc" else (n, cols, max_rows)
            outs = [torch.empty(shape, dtype=tdt, device="cuda") for _ in range(args.ring)]
            tag = f"{layout}_{dtype}_cols{cols}"
            nbytes[tag] = rows * cols * 4 + n * max_rows * cols * outs[0].element_size()

            def ours(cols=cols, layout=layout, dtype=dtype, ins=ins, outs=outs):
                at[0] += 1
                k = at[0] % args.ring
                _lib.check(lib.ss_pad_packed_device(ins[k].data_ptr(), n, d_ro.data_ptr(), rows, cols, max_rows, LAYOUT_CODE[layout], DTYPE_CODE[dtype], 0.0,
                                                    outs[k].data_ptr(), d_len.data_ptr(), sp))
                return outs[k]

            def baseline(layout=layout, tdt=tdt, ins=ins):
                at[0] += 1
                p = pad_sequence(torch.split(ins[at[0] % args.ring], lens_list), batch_first=True)
                if layout == "bct":
                    p = p.transpose(1, 2)
                return p.to(tdt).contiguous()

            at[0] = 0
            got = ours()
            at[0] = 0
            want = baseline()
            torch.cuda.synchronize()
            assert torch.equal(got, want) and d_len.cpu().tolist() == lens_list, tag
            del want
            legs += [(f"pad_{tag}", ours, args.reps), (f"torch_{tag}", baseline, args.torch_reps)]

    def timed(fn, reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / reps * 1e3

    for _, fn, _ in legs:  # warm-up: code objects, the allocator's blocks, every buffer of the ring once
        for _ in range(args.ring):
            fn()
    torch.cuda.synchronize()
    us = {name: [] for name, _, _ in legs}
    for _ in range(args.rounds):
        for name, fn, reps in legs:
            us[name].append(timed(fn, reps))
    for name, _, _ in legs:
        v = us[name]
        res[name] = {"us_per_call_median": statistics.median(v), "us_min": min(v), "us_max": max(v)}
    for tag, b in nbytes.items():
        for leg in (res[f"pad_{tag}"], res[f"torch_{tag}"]):
            leg["bytes_per_call"] = b
            leg["gb_per_s"] = b / leg["us_per_call_median"] * 1e-3
            leg["hbm_fraction"] = leg["gb_per_s"] * 1e9 / HBM_PEAK
        res[f"torch_{tag}"]["over_pad"] = res[f"torch_{tag}"]["us_per_call_median"] / res[f"pad_{tag}"]["us_per_call_median"]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
