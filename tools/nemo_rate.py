"""µs per call of the NeMo / Parakeet log-mel front end (ss_nemo_log_mel_device and ss_nemo_log_mel_packed_device) beside the nearest
existing kernel and beside what a user runs without it, all from one process.

    python tools/nemo_rate.py [--clips 1024] [--seconds 1] [--reps 50] [--windows 10] [--ring-mib 300]

Workload: `--clips` clips of `--seconds` s at 16 kHz (100 rows each) and the same number of clips of 1 .. 16 s (uniform) packed end
to end, at 80 and at 128 bands.  Legs, alternated inside every window:
  nemo_dense_M         ss_nemo_log_mel_device, per-feature normalisation: ss_nemo_c256<13> and ss_nemo_norm_kernel
  nemo_dense_M_none    the same handle with SS_NEMO_NORM_NONE: the first launch alone
  nemo_packed_M        ss_nemo_log_mel_packed_device on the clips of 1 .. 16 s, normalised
  kaldi_fbank80 (a)    ss_kaldi_fbank_device at 80 bins, 25 / 10 ms, on the dense samples: the nearest existing kernel (per-frame
                       conditioning, snip_edges framing, five filter slots per lane, no normalisation)
  torch_dense_M (b)    the extractor's lines in plain torch on the device (pre-emphasis, torch.stft, power, bank matmul, log, mean and
                       deviation over time): what a user runs today
Protocol: every leg is warmed up; then `--windows` windows alternate the legs, each timed with device events around `--reps`
back-to-back calls on one stream (the torch legs: reps / 5); the inputs of a leg rotate over blocks that add up to at least
`--ring-mib` MiB (more than the 256 MiB Infinity Cache), so no call finds its samples on the die.  Reported per leg: the median window
(µs per call), the fastest and the slowest, rows per second, and the share of the 8 TB/s HBM peak on the bytes the call must move
(samples once, rows once; the normalised legs read and write the rows twice more: three passes in place).  Prints one JSON line.
Measuring only: not collected by pytest, not part of bench.py."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mfcc-rust_amd"))

HBM_PEAK = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=1024)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--windows", type=int, default=10)
    ap.add_argument("--ring-mib", type=int, default=300)
    args = ap.parse_args()

    import numpy as np
    import torch

    import speechsauce_amd as ss
    from speechsauce_amd import _lib

    lib = _lib.lib()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    B, L = args.clips, int(round(args.seconds * 16000))
    T = L // 160
    gen = torch.Generator(device="cuda").manual_seed(0)

    def ring(numel):
        n = max(2, -(-args.ring_mib * (1 << 20) // (4 * numel)))
        return [torch.randn(numel, device="cuda", generator=gen) * 0.1 for _ in range(n)]

    dense = [b.view(B, L) for b in ring(B * L)]
    rng = np.random.default_rng(0)
    lens = rng.integers(16000, 16 * 16000 + 1, B).astype(np.int64)
    so = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    fo = np.concatenate([[0], np.cumsum(lens // 160)]).astype(np.int64)
    total_in, rows_p = int(so[-1]), int(fo[-1])
    packed = ring(total_in)
    dso, dfo = torch.from_numpy(so).cuda(), torch.from_numpy(fo).cuda()
    legs = {}  # name -> (call(i), reps, rows, bytes)
    handles = []

    for M in (80, 128):
        cfg = ss._get_nemo_config((M, "per_feature", 400, 0.97, 2.0 ** -24, 1e-5), 0)
        raw = ss._get_nemo_config((M, None, 400, 0.97, 2.0 ** -24, 1e-5), 0)
        handles += [cfg, raw]
        out = torch.empty((B, T, M), device="cuda")
        out_p = torch.empty((rows_p, M), device="cuda")

        def nemo_dense(i, h=cfg.handle, out=out):
            _lib.check(lib.ss_nemo_log_mel_device(h, dense[i % len(dense)].data_ptr(), B, L, L, out.data_ptr(), stream))

        def nemo_none(i, h=raw.handle, out=out):
            _lib.check(lib.ss_nemo_log_mel_device(h, dense[i % len(dense)].data_ptr(), B, L, L, out.data_ptr(), stream))

        def nemo_packed(i, h=cfg.handle, out=out_p):
            _lib.check(lib.ss_nemo_log_mel_packed_device(h, packed[i % len(packed)].data_ptr(), B, dso.data_ptr(), dfo.data_ptr(), rows_p,
                                                         out.data_ptr(), stream))

        legs[f"nemo_dense_{M}"] = (nemo_dense, args.reps, B * T, 4 * (B * L + 5 * B * T * M))
        legs[f"nemo_dense_{M}_none"] = (nemo_none, args.reps, B * T, 4 * (B * L + B * T * M))
        legs[f"nemo_packed_{M}"] = (nemo_packed, max(1, args.reps // 5), rows_p, 4 * (total_in + 5 * rows_p * M))

        p = _lib.SsNemoParams()
        _lib.check(lib.ss_nemo_params_default(C.byref(p), M))
        bank_h = np.zeros((M, 257), np.float32)
        _lib.check(lib.ss_nemo_mel_bank(C.byref(p), bank_h.ctypes.data))
        bank_d = torch.from_numpy(bank_h).cuda()
        win = torch.hann_window(400, periodic=False, device="cuda")

        def torch_rows(x, bank_d=bank_d):
            x = torch.cat([x[:, :1], x[:, 1:] - 0.97 * x[:, :-1]], dim=1)
            spec = torch.stft(x, 512, hop_length=160, win_length=400, window=win, return_complex=True, pad_mode="constant")
            mel = torch.log(bank_d @ (spec.real ** 2 + spec.imag ** 2) + 2.0 ** -24).permute(0, 2, 1)[:, :T]
            mean = mel.mean(dim=1, keepdim=True)
            return (mel - mean) / (mel.std(dim=1, keepdim=True) + 1e-5)

        def torch_leg(i, f=torch_rows):
            f(dense[i % len(dense)])

        legs[f"torch_dense_{M}"] = (torch_leg, max(1, args.reps // 5), B * T, 4 * (B * L + B * T * M))
        nemo_dense(0)
        ref = torch_rows(dense[0])
        torch.cuda.synchronize()
        legs[f"nemo_dense_{M}"] += (float((out - ref).abs().max() / ref.abs().max()),)

    key80 = (16000, 25.0, 10.0, 80, 0, 20.0, 0.0, 0.97, 0.0, "povey", 0.42, True, True, False, True, 1.0, 1.0)
    k80 = ss._get_kaldi_config(key80, 0)
    Tk = 1 + (L - 400) // 160
    out_k, en_k = torch.empty((B, Tk, 80), device="cuda"), torch.empty((B, Tk), device="cuda")

    def kaldi_fbank(i):
        _lib.check(lib.ss_kaldi_fbank_device(k80.handle, dense[i % len(dense)].data_ptr(), B, L, L, out_k.data_ptr(), en_k.data_ptr(), stream))

    legs["kaldi_fbank80"] = (kaldi_fbank, args.reps, B * Tk, 4 * (B * L + B * Tk * 81))

    names = {}
    for name, leg in legs.items():
        leg[0](0)
        leg[0](1)
        torch.cuda.synchronize()
        names[name] = "torch" if name.startswith("torch") else lib.ss_last_kernel_name().decode()

    times = {name: [] for name in legs}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    it = 2
    for _ in range(args.windows):
        for name, leg in legs.items():
            call, reps = leg[0], leg[1]
            e0.record()
            for r in range(reps):
                call(it + r)
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e3 / reps)
            it += reps
    for h in handles:
        h.device_status()

    report = {"clips": B, "seconds": args.seconds, "rows_per_clip": T, "reps": args.reps, "windows": args.windows,
              "ring_blocks_dense": len(dense), "ring_blocks_packed": len(packed), "packed_rows": rows_p, "packed_samples": total_in,
              "device": torch.cuda.get_device_name(), "legs": {}}
    for name, leg in legs.items():
        rows, nbytes = leg[2], leg[3]
        med = statistics.median(times[name])
        report["legs"][name] = {"kernel": names[name], "us_per_call": round(med, 2), "us_min": round(min(times[name]), 2),
                                "us_max": round(max(times[name]), 2), "rows_per_s": round(rows / (med * 1e-6)), "bytes_per_call": nbytes,
                                "hbm_fraction": round(nbytes / (med * 1e-6) / HBM_PEAK, 4)}
        if len(leg) > 4:
            report["legs"][name]["vs_torch_block_metric"] = leg[4]
    us = {name: report["legs"][name]["us_per_call"] for name in legs}
    for M in (80, 128):
        report[f"torch_over_nemo_dense_{M}"] = round(us[f"torch_dense_{M}"] / us[f"nemo_dense_{M}"], 2)
    report["nemo_dense_80_none_over_kaldi_fbank80"] = round(us["nemo_dense_80_none"] / us["kaldi_fbank80"], 3)
    print(json.dumps(report))


if __name__ == "__main__":
    main()
