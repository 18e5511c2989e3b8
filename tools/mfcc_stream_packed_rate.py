"""Rows/s and µs per call of the ragged streaming MFCC over a pool of stream states (ss_mfcc_stream_packed_device) beside what a
caller could do without it.

    python tools/mfcc_stream_packed_rate.py [--pool 4096] [--active 1024] [--max-hops 4] [--reps 200] [--ring-mb 320] [--pcm16]

Workload: 16 kHz MFCC at the default shape (512 points, 320-sample frames, 160-sample hop, 40 filters); a pool of `--pool` stream
states of which `--active` deliver audio in a call, in random slot order, each 1 .. `--max-hops` hops (uniform).  Measured with HIP
events around back-to-back calls on one stream after warm-up.  Every call works on the next element of a ring of pre-built ticks
(chunks, tables, bucket index lists) whose inputs together are larger than the 256 MB Infinity Cache (`--ring-mb`), so that a call
does not find its samples in the caches an earlier call left them in.
  ragged        one ss_mfcc_stream_packed_device call per tick (two launches), eager
  ragged_graph  the same call captured once on static buffers of full capacity and replayed; the tick's chunks and tables are
                copied into the captured buffers first, as a live loop does (us_copies: those copies alone)
  dense2/dense3 baseline (a): the dense ss_mfcc_stream_device on `--active` streams x 2 and x 3 hops -- equal-length work that
                brackets the ragged tick's row count (mean 2.5 hops per entry)
  bucketed      baseline (b): what a caller does with the dense call alone -- per hop count R an index_select of the chunks and of
                the state rows into dense blocks, one dense call, an index_copy_ of the state rows back.  The bucket index lists are
                built outside the timed loop (the host-side bucketing is not charged to the baseline).
With --pcm16 the same ticks are fed as signed 16-bit PCM instead (ss_mfcc_stream_packed_i16_device, scale 2^-15), three legs,
each measured twice (the spread between the two runs is the resolution of the comparison):
  pcm           the PCM ragged call on the int16 chunks
  float         the float ragged call on the same ticks, converted outside the timed loop
  convert_float what a caller does without the PCM call: pcm.to(torch.float32).mul_(scale) in front of the float call
The float ring alone is sized to --ring-mb (the PCM ring is half of it in bytes: still the same ticks).
Prints one JSON line.  Measuring only: not collected by pytest, not part of bench.py.
"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mfcc-rust_amd"))

FLEN, STEP, S, NCEP = 320, 160, 160, 13


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pool", type=int, default=4096)
    ap.add_argument("--active", type=int, default=1024)
    ap.add_argument("--max-hops", type=int, default=4)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--ring-mb", type=int, default=320)
    ap.add_argument("--pcm16", action="store_true")
    args = ap.parse_args()

    import numpy as np
    import torch

    import speechsauce_amd as ss
    from speechsauce_amd import _lib

    lib = _lib.lib()
    P, N, H = args.pool, args.active, args.max_hops
    st = torch.cuda.current_stream()
    sp = C.c_void_p(st.cuda_stream)
    cfg = ss.SpeechConfig(_lib.make_params())
    rng = np.random.default_rng(0)
    cap = N * H  # rows a tick can have
    n_ring = max(2, int(args.ring_mb * 2**20 / (N * (H + 1) / 2 * STEP * 4)) + 1)
    pool = torch.randn((P, S), device="cuda").mul_(0.1)

    ticks = []
    for _ in range(n_ring):
        hops = rng.integers(1, H + 1, N)
        slots = rng.permutation(P)[:N].astype(np.int32)
        so = np.zeros(N + 1, np.int64)
        np.cumsum(hops * STEP, out=so[1:])
        t = {"rows": int(hops.sum()), "x": torch.randn(int(so[-1]), device="cuda").mul_(0.1), "so": torch.from_numpy(so).cuda(),
             "ro": torch.from_numpy(so // STEP).cuda(), "slots": torch.from_numpy(slots).cuda()}
        # baseline (b): the same chunks as rows of a dense [N, H * STEP] block (row i holds its hops[i] hops), bucketed by hop count
        dense = torch.zeros((N, H * STEP), device="cuda")
        for r in range(1, H + 1):
            idx = np.flatnonzero(hops == r)
            cols = (so[idx][:, None] + np.arange(r * STEP)[None, :]).reshape(-1)
            dense[torch.from_numpy(idx).cuda(), :r * STEP] = t["x"][torch.from_numpy(cols).cuda()].reshape(len(idx), r * STEP)
        t["dense"] = dense
        t["buckets"] = [(r, torch.from_numpy(np.flatnonzero(hops == r)).cuda(),
                         torch.from_numpy(slots[hops == r].astype(np.int64)).cuda()) for r in range(1, H + 1) if (hops == r).any()]
        ticks.append(t)
    at = [0]

    def nxt():
        at[0] += 1
        return ticks[at[0] % n_ring]

    def timed(fn, reps):
        fn()
        torch.cuda.synchronize()
        kernel = lib.ss_last_kernel_name().decode()
        start = at[0]
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        rows = sum(ticks[(start + 1 + k) % n_ring]["rows"] for k in range(reps))
        return a.elapsed_time(b) / reps * 1e-3, rows / reps, kernel

    res = {"pool": P, "active": N, "max_hops": H, "ring": n_ring, "device": torch.cuda.get_device_name()}
    out = torch.empty((cap, NCEP), device="cuda")

    if args.pcm16:
        scale = 2.0 ** -15
        for t in ticks:
            t["pcm"] = torch.randint(-32768, 32768, (t["x"].numel(),), device="cuda", dtype=torch.int32).to(torch.int16)
            t["x"] = t["pcm"].to(torch.float32).mul_(scale)
            del t["dense"], t["buckets"]
        cur = torch.cuda.current_stream().cuda_stream

        def pcm():
            t = nxt()
            _lib.check(lib.ss_mfcc_stream_packed_i16_device(cfg.handle, t["pcm"].data_ptr(), N, t["so"].data_ptr(), t["ro"].data_ptr(), t["rows"],
                                                            t["slots"].data_ptr(), P, scale, 100, pool.data_ptr(), out.data_ptr(), C.c_void_p(cur)))

        def flt_on(x, t):
            _lib.check(lib.ss_mfcc_stream_packed_device(cfg.handle, x.data_ptr(), N, t["so"].data_ptr(), t["ro"].data_ptr(), t["rows"],
                                                        t["slots"].data_ptr(), P, 100, pool.data_ptr(), out.data_ptr(), C.c_void_p(cur)))

        def flt():
            t = nxt()
            flt_on(t["x"], t)

        def convert_float():
            t = nxt()
            flt_on(t["pcm"].to(torch.float32).mul_(scale), t)

        for leg, fn in (("pcm", pcm), ("float", flt), ("convert_float", convert_float)):
            res[leg] = {"us_per_call": [], "rows_per_s": []}
        for _ in range(2):
            for leg, fn in (("pcm", pcm), ("float", flt), ("convert_float", convert_float)):
                sec, rows, k = timed(fn, args.reps)
                res[leg]["us_per_call"].append(sec * 1e6)
                res[leg]["rows_per_s"].append(rows / sec)
                res[leg]["rows_per_call"] = rows
                res[leg]["kernel"] = k
        best = {leg: min(res[leg]["us_per_call"]) for leg in ("pcm", "float", "convert_float")}
        res["pcm_over_convert_float_time"] = best["pcm"] / best["convert_float"]
        res["pcm_over_float_time"] = best["pcm"] / best["float"]
        print(json.dumps(res))
        return

    def ragged_on(x, so, ro, slots, total_rows):
        _lib.check(lib.ss_mfcc_stream_packed_device(cfg.handle, x.data_ptr(), N, so.data_ptr(), ro.data_ptr(), total_rows, slots.data_ptr(),
                                                    P, 100, pool.data_ptr(), out.data_ptr(),
                                                    C.c_void_p(torch.cuda.current_stream().cuda_stream)))

    def ragged():
        t = nxt()
        ragged_on(t["x"], t["so"], t["ro"], t["slots"], t["rows"])

    sec, rows, k = timed(ragged, args.reps)
    res["ragged"] = {"rows_per_call": rows, "us_per_call": sec * 1e6, "rows_per_s": rows / sec, "kernel": k}

    # the same call captured on static buffers of full capacity
    gx = torch.zeros(cap * STEP, device="cuda")
    gso, gro = torch.zeros(N + 1, dtype=torch.int64, device="cuda"), torch.zeros(N + 1, dtype=torch.int64, device="cuda")
    gsl = torch.arange(N, dtype=torch.int32, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(st)
    with torch.cuda.stream(side):
        ragged_on(gx, gso, gro, gsl, cap)
    st.wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ragged_on(gx, gso, gro, gsl, cap)

    def copies():
        t = nxt()
        gx[:t["x"].numel()].copy_(t["x"])
        gso.copy_(t["so"])
        gro.copy_(t["ro"])
        gsl.copy_(t["slots"])

    def replay():
        copies()
        g.replay()

    sec, rows, _ = timed(replay, args.reps)
    sec_c, _, _ = timed(copies, args.reps)
    res["ragged_graph"] = {"rows_per_call": rows, "us_per_call": sec * 1e6, "us_copies": sec_c * 1e6, "rows_per_s": rows / sec, "kernel": k}

    # baseline (a): equal-length dense calls that bracket the row count
    state = torch.zeros((N, S), device="cuda")
    for r in (2, 3):
        n_d = max(2, int(args.ring_mb * 2**20 / (N * r * STEP * 4)) + 1)
        ring = [torch.randn((N, r * STEP), device="cuda").mul_(0.1) for _ in range(n_d)]
        out_d = torch.empty((N, r, NCEP), device="cuda")
        i = [0]

        def dense():
            i[0] += 1
            x = ring[i[0] % n_d]
            _lib.check(lib.ss_mfcc_stream_device(cfg.handle, x.data_ptr(), N, r * STEP, r * STEP, 100, state.data_ptr(), out_d.data_ptr(), sp))

        sec, _, k = timed(dense, args.reps)
        res[f"dense{r}"] = {"rows_per_call": N * r, "us_per_call": sec * 1e6, "rows_per_s": N * r / sec, "kernel": k}
        del ring

    # baseline (b): bucket by hop count, gather, one dense call per bucket, scatter the state back
    outs_b = {r: torch.empty((N, r, NCEP), device="cuda") for r in range(1, H + 1)}

    def bucketed():
        t = nxt()
        for r, idx, slots in t["buckets"]:
            x = t["dense"].index_select(0, idx)[:, :r * STEP].contiguous()
            stt = pool.index_select(0, slots)
            n = idx.numel()
            _lib.check(lib.ss_mfcc_stream_device(cfg.handle, x.data_ptr(), n, r * STEP, r * STEP, 100, stt.data_ptr(), outs_b[r].data_ptr(), sp))
            pool.index_copy_(0, slots, stt)

    sec, rows, k = timed(bucketed, args.reps)
    res["bucketed"] = {"rows_per_call": rows, "us_per_call": sec * 1e6, "rows_per_s": rows / sec, "kernel": k,
                       "launches_per_call": "4 per bucket + the dense call's 2"}
    res["ragged_over_bucketed"] = res["ragged"]["rows_per_s"] / res["bucketed"]["rows_per_s"]
    res["ragged_over_dense"] = [res["ragged"]["rows_per_s"] / res[f"dense{r}"]["rows_per_s"] for r in (2, 3)]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
