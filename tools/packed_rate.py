"""Frames/s of packed variable-length clips (ss_mfcc_packed_device) beside the equal-length batch rate and a per-clip loop.

    python tools/packed_rate.py [--clips 1024] [--min-s 1] [--max-s 16] [--reps 20]

Workloads, all 16 kHz MFCC in reference mode (cfg1 parameters), measured with HIP events on one stream after warm-up:
  packed      n clips, lengths uniform in [min-s, max-s] seconds, one ss_mfcc_packed_device call (one launch)
  equal       ss_mfcc_batch_device over n clips of the packed set's mean length (the same frame count to within a clip)
  per_clip    the packed set's clips, one ss_mfcc_batch_device(batch = 1) call each
Prints one JSON line.  Measuring only: not collected by pytest, not part of bench.py.
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mfcc-rust_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=1024)
    ap.add_argument("--min-s", type=float, default=1.0)
    ap.add_argument("--max-s", type=float, default=16.0)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()

    import torch

    import speechsauce_amd as ss
    from speechsauce_amd import _lib

    lib = _lib.lib()
    sr = 16000
    rng = np.random.default_rng(args.seed)
    lens = rng.integers(int(args.min_s * sr), int(args.max_s * sr) + 1, args.clips).astype(np.int64)
    cfg = ss.SpeechConfig(_lib.make_params(sample_rate=sr))
    so, fo = ss._packed_offsets(cfg, lens, int(lens.sum()), "packed_rate")
    rows = int(fo[-1])
    x = torch.randn(int(so[-1]), device="cuda").mul_(0.05)
    dso, dfo = torch.from_numpy(so).cuda(), torch.from_numpy(fo).cuda()
    out = torch.empty((rows, 13), device="cuda")
    L = int(lens.mean())
    T = cfg.num_frames(L)
    xe = torch.randn((args.clips, L), device="cuda").mul_(0.05)
    oute = torch.empty((args.clips, T, 13), device="cuda")
    st = torch.cuda.current_stream()
    sp = C.c_void_p(st.cuda_stream)

    def packed():
        _lib.check(lib.ss_mfcc_packed_device(cfg.handle, x.data_ptr(), args.clips, dso.data_ptr(), dfo.data_ptr(), rows,
                                             out.data_ptr(), sp))

    def equal():
        _lib.check(lib.ss_mfcc_batch_device(cfg.handle, xe.data_ptr(), args.clips, L, L, oute.data_ptr(), sp))

    def per_clip():
        for b in range(args.clips):
            n = int(lens[b])
            _lib.check(lib.ss_mfcc_batch_device(cfg.handle, x.data_ptr() + 4 * int(so[b]), 1, n, n,
                                                out.data_ptr() + 4 * 13 * int(fo[b]), sp))

    def timed(fn, reps):
        fn()
        torch.cuda.synchronize()
        kernel = lib.ss_last_kernel_name().decode()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        cfg.device_status()
        return a.elapsed_time(b) / reps * 1e-3, kernel

    res = {"clips": args.clips, "min_s": args.min_s, "max_s": args.max_s, "device": torch.cuda.get_device_name()}
    t, k = timed(packed, args.reps)
    res["packed"] = {"frames": rows, "s_per_call": t, "frames_per_s": rows / t, "kernel": k}
    t, k = timed(equal, args.reps)
    res["equal"] = {"frames": args.clips * T, "clip_samples": L, "s_per_call": t, "frames_per_s": args.clips * T / t, "kernel": k}
    t, k = timed(per_clip, max(1, args.reps // 10))
    res["per_clip"] = {"frames": rows, "s_per_loop": t, "frames_per_s": rows / t, "kernel": k}
    res["packed_over_equal"] = res["packed"]["frames_per_s"] / res["equal"]["frames_per_s"]
    res["packed_over_per_clip"] = res["packed"]["frames_per_s"] / res["per_clip"]["frames_per_s"]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
