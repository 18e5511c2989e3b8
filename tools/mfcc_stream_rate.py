"""Rows/s and µs per call of the streaming MFCC (ss_mfcc_stream_device) beside the one-shot call on the same real frames.

    python tools/mfcc_stream_rate.py [--streams 1024] [--hops 16] [--reps 50] [--ring 8]

Workloads, 16 kHz MFCC at the default shape (512 points, 320-sample frames, 160-sample hop, 40 filters), measured with HIP events
around synchronised work on one stream after warm-up.  Every call reads the next buffer of an input ring (`--ring` buffers), so
that a call does not find its samples in the caches the previous call left them in:
  (a) continuous   n streams x `hops` hops per call: the rows and the state advance (two launches per call)
      oneshot      ss_mfcc_batch_device on n clips of (hops + 1) frames: the same real frames, one launch
  (b) live_graph   n streams x 1 hop per call, captured once in a torch.cuda graph and replayed (µs per call); live_eager: the same
                   call launched eagerly
  (c) generic      as (a) on the generic kernel's streaming build (the lab library's ss_debug_force_generic), for the record
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
    ap.add_argument("--streams", type=int, default=1024)
    ap.add_argument("--hops", type=int, default=16)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--ring", type=int, default=8)
    args = ap.parse_args()

    import torch

    import speechsauce_amd as ss
    from speechsauce_amd import _lib

    lib = _lib.lib()
    B, K = args.streams, args.hops
    st = torch.cuda.current_stream()
    sp = C.c_void_p(st.cuda_stream)
    cfg = ss.SpeechConfig(_lib.make_params())
    at = [0]

    def timed(fn, reps, lib_=lib):
        fn()
        torch.cuda.synchronize()
        kernel = lib_.ss_last_kernel_name().decode()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / reps * 1e-3, kernel

    def nxt(ring):
        at[0] += 1
        return ring[at[0] % len(ring)]

    res = {"streams": B, "hops": K, "ring": args.ring, "device": torch.cuda.get_device_name()}
    rows = B * K

    # (a) K hops per call against the one-shot call on the same real frames
    ring = [torch.randn((B, K * STEP), device="cuda").mul_(0.1) for _ in range(args.ring)]
    state = torch.zeros((B, S), device="cuda")
    out = torch.empty((B, K, NCEP), device="cuda")

    def cont(lib_=lib, cfg_=cfg):
        x = nxt(ring)
        _lib.check(lib_.ss_mfcc_stream_device(cfg_.handle, x.data_ptr(), B, K * STEP, K * STEP, 100, state.data_ptr(), out.data_ptr(), sp))

    t, k = timed(cont, args.reps)
    res["continuous"] = {"rows": rows, "s_per_call": t, "rows_per_s": rows / t, "kernel": k}
    L = FLEN + K * STEP  # K + 1 frames per clip
    ring_o = [torch.randn((B, L), device="cuda").mul_(0.1) for _ in range(args.ring)]
    out_o = torch.empty((B, K + 1, NCEP), device="cuda")

    def oneshot():
        x = nxt(ring_o)
        _lib.check(lib.ss_mfcc_batch_device(cfg.handle, x.data_ptr(), B, L, L, out_o.data_ptr(), sp))

    t, k = timed(oneshot, args.reps)
    frames = B * (K + 1)
    res["oneshot"] = {"frames": frames, "s_per_call": t, "frames_per_s": frames / t, "kernel": k}
    res["continuous_over_oneshot"] = res["continuous"]["rows_per_s"] / res["oneshot"]["frames_per_s"]

    # (b) one hop per call: graph-replayed and eager
    ring1 = [torch.randn((B, STEP), device="cuda").mul_(0.1) for _ in range(args.ring)]
    x1 = torch.zeros((B, STEP), device="cuda")
    out1 = torch.empty((B, 1, NCEP), device="cuda")

    def live():
        _lib.check(lib.ss_mfcc_stream_device(cfg.handle, x1.data_ptr(), B, STEP, STEP, 100, state.data_ptr(), out1.data_ptr(),
                                             C.c_void_p(torch.cuda.current_stream().cuda_stream)))

    side = torch.cuda.Stream()
    side.wait_stream(st)
    with torch.cuda.stream(side):
        live()
    st.wait_stream(side)
    torch.cuda.synchronize()
    kernel = lib.ss_last_kernel_name().decode()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        live()

    def replay():
        x1.copy_(nxt(ring1))  # a new chunk into the captured input, as a live loop does
        g.replay()

    def eager():
        x1.copy_(nxt(ring1))
        live()

    def copy_only():
        x1.copy_(nxt(ring1))

    t, _ = timed(replay, args.reps * 4)
    tc, _ = timed(copy_only, args.reps * 4)
    res["live_graph"] = {"rows": B, "us_per_call": t * 1e6, "us_chunk_copy": tc * 1e6, "rows_per_s": B / t, "kernel": kernel}
    t, _ = timed(eager, args.reps * 4)
    res["live_eager"] = {"rows": B, "us_per_call": t * 1e6, "kernel": kernel}

    # (c) the generic streaming build at the shape of (a)
    lab = _lib.lab()
    with _lib.use_library(lab):
        cfg_g = ss.SpeechConfig(_lib.make_params())
        try:
            lab.ss_debug_force_generic(1)
            t, k = timed(lambda: cont(lab, cfg_g), max(1, args.reps // 5), lab)
        finally:
            lab.ss_debug_force_generic(0)
    res["generic"] = {"rows": rows, "s_per_call": t, "rows_per_s": rows / t, "kernel": k}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
