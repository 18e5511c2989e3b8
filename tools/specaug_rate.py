"""µs per call of SpecAugment on packed rows: ss_specaug_packed_device in place and out of place beside the copy that is the floor of
the out-of-place form and beside what a user writes in torch with the lengths already known on the host, from one process.

    python tools/specaug_rate.py [--clips 1024] [--reps 20] [--torch-reps 5] [--rounds 5] [--ring 2]

Workload: `--clips` clips of 1 .. 16 s (98 .. 1598 rows at 100 rows/s, uniform; about 868 k rows), cols = 80 (fbank) and 240 (spliced),
the LibriSpeech policy: 2 time masks of at most 100 rows, 2 frequency masks of at most 27 columns, mask value 0.  Legs, per cols:
  specaug_inplace   the combined call with out == vec: plan launch, apply launch, epoch bump; only the masked elements are written
  specaug_copy      the combined call into a second block: every element read once and written once
  copy_floor        out.copy_(vec) of the same block: what moving the block costs without any masking
  torch_masks       the same policy in torch on the packed rows: widths and starts from torch.rand, the clip id and local row of every
                    packed row from repeat_interleave / arange on the host-known lengths, `arange` compares for the two kinds of span,
                    masked_fill_ in place
bytes_per_call is vec once plus out once for the two copying legs and the masked elements once (counted from the spans of one call)
for the in-place leg; hbm_fraction reads it against 8.0 TB/s.  Before anything is timed the out-of-place result is compared with
torch.where on a mask built from the call's own spans, and the in-place result with it (torch.equal: the rows are finite).
Protocol: every leg is warmed up, then `--rounds` rounds alternate the legs, each timed with HIP events around back-to-back calls on
one stream; every call takes the next of a ring of `--ring` blocks.  Reported per leg: the median over the rounds, the fastest and the
slowest round.
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
POLICY = (2, 100, 1.0, 2, 27)  # n_time, max_time_width, time_ratio, n_freq, max_freq_width


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

    from speechsauce_amd import _lib

    lib = _lib.lib()
    sp = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rng = np.random.default_rng(0)
    n = args.clips
    lens = rng.integers(98, 1599, n)
    ro = np.zeros(n + 1, np.int64)
    np.cumsum(lens, out=ro[1:])
    rows = int(ro[-1])
    d_ro, d_lens = torch.from_numpy(ro).cuda(), torch.from_numpy(lens).cuda()
    block = torch.from_numpy(np.array([2026, 0], np.uint64).view(np.int64)).cuda()
    spans = torch.zeros((n, 4, 2), dtype=torch.int32, device="cuda")
    nt, tw, ratio, nf, fw = POLICY
    at = [0]
    legs, nbytes = [], {}
    res = {"clips": n, "rows_packed": rows, "policy": list(POLICY), "reps": args.reps, "torch_reps": args.torch_reps, "rounds": args.rounds,
           "ring": args.ring, "device": torch.cuda.get_device_name()}

    def call(src, dst):
        """the combined call on one block; the column count is the block's own, so no leg can hand in another's"""
        assert src.shape == dst.shape == (rows, src.shape[1]) and src.is_contiguous() and dst.is_contiguous()
        _lib.check(lib.ss_specaug_packed_device(src.data_ptr(), n, d_ro.data_ptr(), rows, src.shape[1], block.data_ptr(), 0, nt, tw, ratio, nf, fw, 0.0,
                                                dst.data_ptr(), spans.data_ptr(), sp))

    def row_index():
        """the clip id and the local row of every packed row, from the host-known lengths (no read-back: output_size is given)"""
        cid = torch.repeat_interleave(torch.arange(n, device="cuda"), d_lens, output_size=rows)
        return cid, torch.arange(rows, device="cuda") - d_ro[cid]

    def mask_of(sp_table, cols):
        """the boolean mask [rows, cols] of a spans table, by arange compares"""
        cid, local = row_index()
        s = sp_table.long()
        tm = torch.zeros(rows, dtype=torch.bool, device="cuda")
        for k in range(nt):
            tm |= (local >= s[cid, k, 0]) & (local < s[cid, k, 0] + s[cid, k, 1])
        c = torch.arange(cols, device="cuda")
        fm = torch.zeros((n, cols), dtype=torch.bool, device="cuda")
        for k in range(nt, nt + nf):
            fm |= (c >= s[:, k, :1]) & (c < s[:, k, :1] + s[:, k, 1:])
        return tm[:, None] | fm[cid]

    for cols in (80, 240):
        ins = [torch.randn((rows, cols), device="cuda").mul_(3).add_(1) for _ in range(args.ring)]
        outs = [torch.empty((rows, cols), device="cuda") for _ in range(args.ring)]

        def inplace(ins=ins):
            at[0] += 1
            call(ins[at[0] % args.ring], ins[at[0] % args.ring])

        def copy(ins=ins, outs=outs):
            at[0] += 1
            call(ins[at[0] % args.ring], outs[at[0] % args.ring])

        def floor(ins=ins, outs=outs):
            at[0] += 1
            outs[at[0] % args.ring].copy_(ins[at[0] % args.ring])

        def torch_masks(ins=ins, cols=cols):
            at[0] += 1
            x = ins[at[0] % args.ring]
            u = torch.rand((n, nt + nf, 2), device="cuda")
            T = d_lens.double()
            cid, local = row_index()
            tm = torch.zeros(rows, dtype=torch.bool, device="cuda")
            for k in range(nt):
                width = (u[:, k, 0] * (torch.clamp(T * ratio, max=tw) + 1)).long()
                start = (u[:, k, 1] * (T - width + 1)).long()
                tm |= (local >= start[cid]) & (local < (start + width)[cid])
            c = torch.arange(cols, device="cuda")
            fm = torch.zeros((n, cols), dtype=torch.bool, device="cuda")
            for k in range(nt, nt + nf):
                width = (u[:, k, 0] * (min(fw, cols) + 1)).long()
                start = (u[:, k, 1] * (cols - width + 1)).long()
                fm |= (c >= start[:, None]) & (c < (start + width)[:, None])
            x.masked_fill_(tm[:, None] | fm[cid], 0.0)
            return x

        # the check: one out-of-place call against torch.where on the mask of its own spans, then the same epoch in place
        epoch = int(block.cpu().numpy().view(np.uint64)[1])
        call(ins[0], outs[0])
        torch.cuda.synchronize()
        m = mask_of(spans, cols)
        assert torch.equal(outs[0], torch.where(m, torch.zeros((), device="cuda"), ins[0])), cols
        masked = int(m.sum())
        assert 0 < masked < rows * cols
        block[1:].copy_(torch.from_numpy(np.array([epoch], np.uint64).view(np.int64)))
        work = ins[0].clone()
        call(work, work)
        torch.cuda.synchronize()
        assert torch.equal(work, outs[0]), cols
        del work, m
        nbytes[f"specaug_inplace_cols{cols}"] = masked * 4
        for name in ("specaug_copy", "copy_floor", "torch_masks"):
            nbytes[f"{name}_cols{cols}"] = 2 * rows * cols * 4
        res[f"masked_fraction_cols{cols}"] = masked / (rows * cols)
        legs += [(f"specaug_inplace_cols{cols}", inplace, args.reps), (f"specaug_copy_cols{cols}", copy, args.reps), (f"copy_floor_cols{cols}", floor, args.reps),
                 (f"torch_masks_cols{cols}", torch_masks, args.torch_reps)]

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
        leg = res[name] = {"us_per_call_median": statistics.median(v), "us_min": min(v), "us_max": max(v), "bytes_per_call": nbytes[name]}
        leg["gb_per_s"] = nbytes[name] / leg["us_per_call_median"] * 1e-3
        leg["hbm_fraction"] = leg["gb_per_s"] * 1e9 / HBM_PEAK
    for cols in (80, 240):
        res[f"specaug_copy_cols{cols}"]["over_copy_floor"] = res[f"specaug_copy_cols{cols}"]["us_per_call_median"] / res[f"copy_floor_cols{cols}"]["us_per_call_median"]
        for name in ("specaug_inplace", "specaug_copy"):
            res[f"torch_masks_cols{cols}"][f"over_{name}"] = res[f"torch_masks_cols{cols}"]["us_per_call_median"] / res[f"{name}_cols{cols}"]["us_per_call_median"]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
