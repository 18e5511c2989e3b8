"""Frames/s of the one-shot MFCC calls fed 16-bit PCM beside the float calls: what converting on load buys.

    python tools/pcm16_rate.py [--clips 1024] [--samples 16000] [--min-s 1] [--max-s 16] [--reps 20] [--host-reps 5]
    python tools/pcm16_rate.py --mel [--clips 1024] [--samples 16000] [--min-s 1] [--max-s 16] [--pool 4096] [--max-hops 4] [--reps 20]

16 kHz MFCC in reference mode (cfg1 parameters).  Device legs, HIP events on one stream after warm-up, every call on the next of
a set of input buffers that together hold more than 256 MiB (no call finds its samples in the Infinity Cache):
  batch   --clips x --samples equal-length clips
    pcm          ss_mfcc_batch_i16_device
    float        ss_mfcc_batch_device on the pre-converted buffers (the float path itself: compare it with the parent commit's)
    convert      one conversion launch (int16 * scale -> float32 into a temporary) + ss_mfcc_batch_device: what a caller did before
  packed  --clips clips, lengths uniform in [min-s, max-s] seconds: the same three on ss_mfcc_packed[_i16]_device
Host leg, pinned buffers, wall clock: ss_mfcc_batch_i16 against ss_mfcc_batch on the same clips (PCIe included).
The decision rule of DESIGN section 4: a PCM build stays where pcm is not slower than 1.02 x convert on its shape.
--mel: the mel spectrogram of the cfg3 shape (2048 / 512, 128 mels) instead, rows/s, the same three legs on three layouts: dense
(ss_mel_spectrogram[_i16]_device), packed (ss_mel_spectrogram_packed[_i16]_device) and the pool workload of
tools/mel_stream_packed_rate.py (--clips entries of 1 .. --max-hops hops on a --pool row pool, ss_mel_spectrogram_stream_packed[_i16]_device).
Prints one JSON line.  Measuring only: not collected by pytest, not part of bench.py.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

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
    ap.add_argument("--host-reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--legs", default="batch,packed,host")
    ap.add_argument("--mel", action="store_true")
    ap.add_argument("--pool", type=int, default=4096)
    ap.add_argument("--max-hops", type=int, default=4)
    args = ap.parse_args()

    import torch

    import speechsauce_amd as ss
    from speechsauce_amd import _lib

    lib = _lib.lib()
    sr, scale = 16000, 2.0 ** -15
    cfg = ss.SpeechConfig(_lib.make_params(sample_rate=sr))
    sp = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    res = {"clips": args.clips, "device": torch.cuda.get_device_name(), "scale": scale}

    def pcm_sets(n_samples):
        """Enough int16 buffers of n_samples that the PCM set alone exceeds ROTATE_BYTES (the float set is twice that), at least 2."""
        k = max(2, ROTATE_BYTES // (2 * n_samples) + 1)
        g = torch.Generator(device="cuda")
        g.manual_seed(args.seed)
        ps = [torch.randint(-3000, 3000, (n_samples,), generator=g, device="cuda", dtype=torch.int32).to(torch.int16) for _ in range(k)]
        return ps, [p.to(torch.float32) * scale for p in ps]

    def timed(fn, reps, k):
        for i in range(k):  # warm-up: every buffer once
            fn(i)
        torch.cuda.synchronize()
        kernel = lib.ss_last_kernel_name().decode()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for i in range(reps):
            fn(i % k)
        b.record()
        torch.cuda.synchronize()
        cfg.device_status()
        return a.elapsed_time(b) / reps * 1e-3, kernel

    def three(frames, k, pcm_call, float_call, convert):
        out = {}
        for name, fn in (("pcm", pcm_call), ("float", float_call), ("convert", lambda i: (convert(i), float_call(-1)))):
            t, kern = timed(fn, args.reps, k)
            out[name] = {"s_per_call": t, "frames_per_s": frames / t, "kernel": kern}
        out["frames"] = frames
        out["pcm_over_convert"] = out["pcm"]["frames_per_s"] / out["convert"]["frames_per_s"]
        out["pcm_over_float"] = out["pcm"]["frames_per_s"] / out["float"]["frames_per_s"]
        return out

    if args.mel:
        cfg = ss.SpeechConfig(_lib.make_params(sample_rate=sr, fft_points=2048, frame_length=0.032, frame_stride=0.032, num_filters=128,
                                               high_frequency=8000.0))
        H, M, rng = 512, 128, np.random.default_rng(args.seed)
        # dense
        B, L = args.clips, args.samples
        R = cfg.stft_rows(L)[0]
        ps, fs = pcm_sets(B * L)
        tmp, out = torch.empty(B * L, device="cuda"), torch.empty((B, M, R), device="cuda")
        res["dense"] = three(B * R, len(ps),
                             lambda i: _lib.check(lib.ss_mel_spectrogram_i16_device(cfg.handle, ps[i].data_ptr(), B, L, L, scale, out.data_ptr(), sp)),
                             lambda i: _lib.check(lib.ss_mel_spectrogram_device(cfg.handle, (tmp if i < 0 else fs[i]).data_ptr(), B, L, L,
                                                                                out.data_ptr(), sp)),
                             lambda i: torch.mul(ps[i], scale, out=tmp))
        del ps, fs, tmp, out
        # packed
        lens = rng.integers(int(args.min_s * sr), int(args.max_s * sr) + 1, args.clips).astype(np.int64)
        so = ss._sample_offsets(lens, int(lens.sum()), "pcm16_rate")
        ro = ss._row_offsets(cfg, so)
        rows, n = int(ro[-1]), int(so[-1])
        dso, dro = torch.from_numpy(so).cuda(), torch.from_numpy(ro).cuda()
        ps, fs = pcm_sets(n)
        tmp, out = torch.empty(n, device="cuda"), torch.empty(M * rows, device="cuda")
        res["packed"] = three(rows, len(ps),
                              lambda i: _lib.check(lib.ss_mel_spectrogram_packed_i16_device(cfg.handle, ps[i].data_ptr(), args.clips, dso.data_ptr(),
                                                                                            scale, dro.data_ptr(), rows, out.data_ptr(), sp)),
                              lambda i: _lib.check(lib.ss_mel_spectrogram_packed_device(cfg.handle, (tmp if i < 0 else fs[i]).data_ptr(), args.clips,
                                                                                        dso.data_ptr(), dro.data_ptr(), rows, out.data_ptr(), sp)),
                              lambda i: torch.mul(ps[i], scale, out=tmp))
        del ps, fs, tmp, out
        # pool
        hops = rng.integers(1, args.max_hops + 1, args.clips).astype(np.int64)
        so = np.zeros(args.clips + 1, np.int64)
        np.cumsum(hops * H, out=so[1:])
        ro = so // H
        rows, n = int(ro[-1]), int(so[-1])
        dso, dro = torch.from_numpy(so).cuda(), torch.from_numpy(ro).cuda()
        dsl = torch.from_numpy(rng.permutation(args.pool)[:args.clips].astype(np.int32)).cuda()
        pool = torch.zeros((args.pool, 2048 - H), device="cuda")
        ps, fs = pcm_sets(n)
        tmp, out = torch.empty(n, device="cuda"), torch.empty(M * rows, device="cuda")
        res["pool"] = three(rows, len(ps),
                            lambda i: _lib.check(lib.ss_mel_spectrogram_stream_packed_i16_device(
                                cfg.handle, ps[i].data_ptr(), args.clips, dso.data_ptr(), dro.data_ptr(), rows, dsl.data_ptr(), args.pool, scale,
                                pool.data_ptr(), out.data_ptr(), sp)),
                            lambda i: _lib.check(lib.ss_mel_spectrogram_stream_packed_device(
                                cfg.handle, (tmp if i < 0 else fs[i]).data_ptr(), args.clips, dso.data_ptr(), dro.data_ptr(), rows, dsl.data_ptr(),
                                args.pool, pool.data_ptr(), out.data_ptr(), sp)),
                            lambda i: torch.mul(ps[i], scale, out=tmp))
        res["pool"].update(pool=args.pool, max_hops=args.max_hops, samples=n)
        print(json.dumps(res))
        return

    if "batch" in args.legs:
        B, L = args.clips, args.samples
        T = cfg.num_frames(L)
        ps, fs = pcm_sets(B * L)
        tmp = torch.empty(B * L, device="cuda")
        out = torch.empty((B, T, 13), device="cuda")

        def float_call(i):
            x = tmp if i < 0 else fs[i]
            _lib.check(lib.ss_mfcc_batch_device(cfg.handle, x.data_ptr(), B, L, L, out.data_ptr(), sp))

        res["batch"] = three(B * T, len(ps),
                             lambda i: _lib.check(lib.ss_mfcc_batch_i16_device(cfg.handle, ps[i].data_ptr(), B, L, L, scale, out.data_ptr(), sp)),
                             float_call, lambda i: torch.mul(ps[i], scale, out=tmp))
        res["batch"]["clip_samples"] = L
        res["batch"]["buffers"] = len(ps)
        del ps, fs, tmp

    if "packed" in args.legs:
        rng = np.random.default_rng(args.seed)
        lens = rng.integers(int(args.min_s * sr), int(args.max_s * sr) + 1, args.clips).astype(np.int64)
        so, fo = ss._packed_offsets(cfg, lens, int(lens.sum()), "pcm16_rate")
        rows, n = int(fo[-1]), int(so[-1])
        dso, dfo = torch.from_numpy(so).cuda(), torch.from_numpy(fo).cuda()
        ps, fs = pcm_sets(n)
        tmp = torch.empty(n, device="cuda")
        out = torch.empty((rows, 13), device="cuda")

        def float_call(i):
            x = tmp if i < 0 else fs[i]
            _lib.check(lib.ss_mfcc_packed_device(cfg.handle, x.data_ptr(), args.clips, dso.data_ptr(), dfo.data_ptr(), rows, out.data_ptr(), sp))

        res["packed"] = three(rows, len(ps),
                              lambda i: _lib.check(lib.ss_mfcc_packed_i16_device(cfg.handle, ps[i].data_ptr(), args.clips, dso.data_ptr(), scale,
                                                                                 dfo.data_ptr(), rows, out.data_ptr(), sp)),
                              float_call, lambda i: torch.mul(ps[i], scale, out=tmp))
        res["packed"].update(min_s=args.min_s, max_s=args.max_s, samples=n, buffers=len(ps))
        del ps, fs, tmp

    if "host" in args.legs:
        B, L = args.clips, args.samples
        T = cfg.num_frames(L)
        hp = torch.randint(-3000, 3000, (B, L), dtype=torch.int16).pin_memory()
        hf = (hp.to(torch.float32) * scale).pin_memory()
        ho = torch.empty((B, T, 13)).pin_memory()
        host = {}
        for name, call in (("pcm", lambda: lib.ss_mfcc_batch_i16(cfg.handle, hp.data_ptr(), B, L, L, scale, ho.data_ptr())),
                           ("float", lambda: lib.ss_mfcc_batch(cfg.handle, hf.data_ptr(), B, L, L, ho.data_ptr()))):
            _lib.check(call())
            t0 = time.perf_counter()
            for _ in range(args.host_reps):
                _lib.check(call())
            t = (time.perf_counter() - t0) / args.host_reps
            host[name] = {"s_per_call": t, "frames_per_s": B * T / t}
        host["pcm_over_float"] = host["pcm"]["frames_per_s"] / host["float"]["frames_per_s"]
        host["bytes_ratio"] = (2 * L + 4 * 13 * T) / (4 * L + 4 * 13 * T)
        res["host"] = host
    print(json.dumps(res))


if __name__ == "__main__":
    main()
