"""Rows/s of the packed variable-length mel spectrogram (ss_mel_spectrogram_packed_device) beside the equal-length rate and a
per-clip loop.

    python tools/mel_packed_rate.py [--clips 1024] [--min-s 1] [--max-s 16] [--reps 20]

Workloads, all 16 kHz, the cfg3 shape (2048 points, hop 512, 128 mels), measured with HIP events on one stream after warm-up:
  packed      n clips, lengths uniform in [min-s, max-s] seconds, one ss_mel_spectrogram_packed_device call (one launch)
  equal       ss_mel_spectrogram_device over n clips of the packed set's mean length (the same row count to within a clip)
  per_clip    the packed set's clips, one ss_mel_spectrogram_device(channels = 1) call each
Also the packed call on the generic kernel's packed build (--no-generic skips it; it needs the lab library).  Prints one JSON
line.  Measuring only: not collected by pytest, not part of bench.py.
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mfcc-rust_amd"))

CFG3 = dict(sample_rate=16000, fft_points=2048, frame_length=0.032, frame_stride=0.032, num_filters=128, high_frequency=8000.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=1024)
    ap.add_argument("--min-s", type=float, default=1.0)
    ap.add_argument("--max-s", type=float, default=16.0)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--no-generic", action="store_true")
    args = ap.parse_args()

    import torch

    import speechsauce_amd as ss
    from speechsauce_amd import _lib

    lib = _lib.lib()
    sr = 16000
    M = CFG3["num_filters"]
    rng = np.random.default_rng(args.seed)
    lens = rng.integers(int(args.min_s * sr), int(args.max_s * sr) + 1, args.clips).astype(np.int64)
    cfg = ss.SpeechConfig(_lib.make_params(**CFG3))
    so = ss._sample_offsets(lens, int(lens.sum()), "mel_packed_rate")
    ro = ss._row_offsets(cfg, so)
    rows = int(ro[-1])
    x = torch.randn(int(so[-1]), device="cuda").mul_(0.05)
    dso, dro = torch.from_numpy(so).cuda(), torch.from_numpy(ro).cuda()
    out = torch.empty((M * rows,), device="cuda")
    L = int(lens.mean())
    R, _ = cfg.stft_rows(L)
    xe = torch.randn((args.clips, L), device="cuda").mul_(0.05)
    oute = torch.empty((args.clips, M, R), device="cuda")
    st = torch.cuda.current_stream()
    sp = C.c_void_p(st.cuda_stream)

    def packed(lb=lib, c=cfg):
        _lib.check(lb.ss_mel_spectrogram_packed_device(c.handle, x.data_ptr(), args.clips, dso.data_ptr(), dro.data_ptr(), rows,
                                                       out.data_ptr(), sp))

    def equal():
        _lib.check(lib.ss_mel_spectrogram_device(cfg.handle, xe.data_ptr(), args.clips, L, L, oute.data_ptr(), sp))

    def per_clip():
        for b in range(args.clips):
            n = int(lens[b])
            _lib.check(lib.ss_mel_spectrogram_device(cfg.handle, x.data_ptr() + 4 * int(so[b]), 1, n, n,
                                                     out.data_ptr() + 4 * M * int(ro[b]), sp))

    def timed(fn, reps, lb=lib, c=cfg):
        fn()
        torch.cuda.synchronize()
        kernel = lb.ss_last_kernel_name().decode()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        c.device_status()
        return a.elapsed_time(b) / reps * 1e-3, kernel

    res = {"clips": args.clips, "min_s": args.min_s, "max_s": args.max_s, "device": torch.cuda.get_device_name()}
    t, k = timed(packed, args.reps)
    res["packed"] = {"rows": rows, "s_per_call": t, "rows_per_s": rows / t, "kernel": k}
    t, k = timed(equal, args.reps)
    res["equal"] = {"rows": args.clips * R, "clip_samples": L, "s_per_call": t, "rows_per_s": args.clips * R / t, "kernel": k}
    t, k = timed(per_clip, max(1, args.reps // 10))
    res["per_clip"] = {"rows": rows, "s_per_loop": t, "rows_per_s": rows / t, "kernel": k}
    res["packed_over_equal"] = res["packed"]["rows_per_s"] / res["equal"]["rows_per_s"]
    res["packed_over_per_clip"] = res["packed"]["rows_per_s"] / res["per_clip"]["rows_per_s"]
    if not args.no_generic:
        lab = _lib.lab()
        with _lib.use_library(lab):
            lab.ss_debug_force_generic(1)
            try:
                lcfg = ss.SpeechConfig(_lib.make_params(**CFG3))
                t, k = timed(lambda: packed(lab, lcfg), args.reps, lab, lcfg)
            finally:
                lab.ss_debug_force_generic(0)
        res["packed_generic"] = {"rows": rows, "s_per_call": t, "rows_per_s": rows / t, "kernel": k}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
