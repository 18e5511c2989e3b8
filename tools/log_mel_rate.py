"""Microseconds per call of the fused log-mel calls beside the two-step pair they replace: what converting in the epilogue buys.

    python tools/log_mel_rate.py [--clips 1024] [--samples 16000] [--min-s 1] [--max-s 16] [--reps 20] [--rounds 9] [--seed 0]

The mel spectrogram of the cfg3 shape (16 kHz, 2048 / 512, 128 mels), two layouts, top_db 80 and None:
  dense   --clips x --samples equal-length clips
    fused     ss_log_mel_spectrogram_device
    two_step  ss_mel_spectrogram_device, then ss_power_to_db_packed_device over the block with every clip as its own segment
  packed  --clips clips, lengths uniform in [min-s, max-s] seconds
    fused     ss_log_mel_spectrogram_packed_device
    two_step  ss_mel_spectrogram_packed_device, then ss_power_to_db_packed_device over the row offsets
Both legs run in the same process on the same buffers and write the same output block (checked bit for bit before anything is
timed).  HIP events on one stream after warm-up; every call takes the next of a ring of input buffers that together hold more than
256 MiB, so no call finds its samples in the Infinity Cache.  A round times --reps calls of one leg, the legs alternate round by
round; reported per leg: the median over --rounds rounds and their spread (max - min), in microseconds per call, and the kernel
names ss_last_kernel_name() gave (the two-step leg: the mel kernel's; the dB pass has no name of its own).
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

ROTATE_BYTES = 256 << 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=1024)
    ap.add_argument("--samples", type=int, default=16000)
    ap.add_argument("--min-s", type=float, default=1.0)
    ap.add_argument("--max-s", type=float, default=16.0)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()

    import torch

    import speechsauce_amd as ss
    from speechsauce_amd import _lib

    lib = _lib.lib()
    sr, M = 16000, 128
    cfg = ss.SpeechConfig(_lib.make_params(sample_rate=sr, fft_points=2048, frame_length=0.032, frame_stride=0.032, num_filters=M,
                                           high_frequency=8000.0))
    sp = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    res = {"clips": args.clips, "device": torch.cuda.get_device_name(), "reps": args.reps, "rounds": args.rounds}

    def ring(n_samples):
        """Enough float buffers of n_samples that together they exceed ROTATE_BYTES, at least 2: 0.1-amplitude noise."""
        k = max(2, ROTATE_BYTES // (4 * n_samples) + 1)
        g = torch.Generator(device="cuda")
        g.manual_seed(args.seed)
        return [torch.randn(n_samples, generator=g, device="cuda").mul_(0.1) for _ in range(k)]

    def one_round(fn, k, first):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for i in range(args.reps):
            fn((first + i) % k)
        b.record()
        torch.cuda.synchronize()
        cfg.device_status()
        return a.elapsed_time(b) / args.reps * 1e3  # us per call

    def compare(fused, two_step, k, out):
        """Both legs give the same bits; then alternating rounds."""
        legs = {}
        for name, fn in (("fused", fused), ("two_step", two_step)):
            for i in range(k):  # warm-up: every buffer once
                fn(i)
            torch.cuda.synchronize()
            legs[name] = {"kernel": lib.ss_last_kernel_name().decode(), "us": []}
        fused(0)
        got = out.clone()
        two_step(0)
        torch.cuda.synchronize()
        if not torch.equal(got, out):
            raise SystemExit("log_mel_rate: the fused call and the two-step pair disagree")
        for r in range(args.rounds):
            for name, fn in (("fused", fused), ("two_step", two_step)):
                legs[name]["us"].append(one_round(fn, k, r * args.reps))
        for leg in legs.values():
            us = leg.pop("us")
            leg.update(us_per_call=float(np.median(us)), spread_us=float(max(us) - min(us)), rounds_us=[round(u, 2) for u in us])
        legs["fused_over_two_step"] = legs["fused"]["us_per_call"] / legs["two_step"]["us_per_call"]
        return legs

    for top_db in (80.0, None):
        td = -1.0 if top_db is None else top_db
        tag = "top80" if top_db is not None else "nofloor"
        # dense
        B, L = args.clips, args.samples
        R = cfg.stft_rows(L)[0]
        xs = ring(B * L)
        out, tmp = torch.empty((B, M, R), device="cuda"), torch.empty((B, M, R), device="cuda")
        table = (torch.arange(B + 1, dtype=torch.int64) * R).cuda()

        def dense_fused(i):
            _lib.check(lib.ss_log_mel_spectrogram_device(cfg.handle, xs[i].data_ptr(), B, L, L, 1.0, 1e-10, td, out.data_ptr(), sp))

        def dense_two_step(i):
            _lib.check(lib.ss_mel_spectrogram_device(cfg.handle, xs[i].data_ptr(), B, L, L, tmp.data_ptr(), sp))
            _lib.check(lib.ss_power_to_db_packed_device(tmp.data_ptr(), B, table.data_ptr(), B * R, M, 1.0, 1e-10, td, out.data_ptr(), sp))

        res[f"dense_{tag}"] = dict(compare(dense_fused, dense_two_step, len(xs), out), rows=B * R, clip_samples=L, buffers=len(xs))
        del xs, out, tmp
        # packed
        rng = np.random.default_rng(args.seed)
        lens = rng.integers(int(args.min_s * sr), int(args.max_s * sr) + 1, args.clips).astype(np.int64)
        so = ss._sample_offsets(lens, int(lens.sum()), "log_mel_rate")
        ro = ss._row_offsets(cfg, so)
        rows, n = int(ro[-1]), int(so[-1])
        dso, dro = torch.from_numpy(so).cuda(), torch.from_numpy(ro).cuda()
        xs = ring(n)
        out, tmp = torch.empty(M * rows, device="cuda"), torch.empty(M * rows, device="cuda")

        def packed_fused(i):
            _lib.check(lib.ss_log_mel_spectrogram_packed_device(cfg.handle, xs[i].data_ptr(), args.clips, dso.data_ptr(), dro.data_ptr(), rows,
                                                                1.0, 1e-10, td, out.data_ptr(), sp))

        def packed_two_step(i):
            _lib.check(lib.ss_mel_spectrogram_packed_device(cfg.handle, xs[i].data_ptr(), args.clips, dso.data_ptr(), dro.data_ptr(), rows,
                                                            tmp.data_ptr(), sp))
            _lib.check(lib.ss_power_to_db_packed_device(tmp.data_ptr(), args.clips, dro.data_ptr(), rows, M, 1.0, 1e-10, td, out.data_ptr(), sp))

        res[f"packed_{tag}"] = dict(compare(packed_fused, packed_two_step, len(xs), out), rows=rows, samples=n, buffers=len(xs),
                                    min_s=args.min_s, max_s=args.max_s)
        del xs, out, tmp
    print(json.dumps(res))


if __name__ == "__main__":
    main()
