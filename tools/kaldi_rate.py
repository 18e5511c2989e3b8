"""µs per call of the Kaldi-compatible front end (ss_kaldi_fbank_device and friends) beside the nearest existing kernel and beside
what a user runs without it, all from one process.

    python tools/kaldi_rate.py [--clips 1024] [--seconds 1] [--reps 100] [--windows 10] [--ring-mib 300] [--pcm16]

Workload: `--clips` clips of `--seconds` s at 16 kHz (98 frames each at 25 / 10 ms), fbank-80.  Legs, alternated inside every window:
  kaldi_fbank80      ss_kaldi_fbank_device, 80 bins, 25 / 10 ms, the log energy written too
  mfe80_c256w (a)    ss_mfe_batch_device at 80 filters, frame length 400, Hann window, power spectrum: the nearest existing kernel
                     (it must report ss_mfcc_c256w<13,pow2,mfe,win>), so the difference is the conditioning stage and the ln
  torch_fbank80 (b)  the same definition in plain torch on the device: unfold, mean, pre-emphasis, window, torch.fft.rfft, matmul,
                     log -- what a user runs today (torchaudio is not needed)
  kaldi_mfcc13       ss_kaldi_mfcc_device, 23 bins, 13 cepstra
  kaldi_fbank80_packed   ss_kaldi_fbank_packed_device on `--clips` clips of 1 .. 16 s (uniform)
Protocol: every leg is warmed up; then `--windows` windows alternate the legs, each timed with device events around `--reps`
back-to-back launches on one stream (the torch leg: reps / 5); the inputs of a leg rotate over blocks that add up to at least
`--ring-mib` MiB (more than the 256 MiB Infinity Cache), so no call finds its samples on the die.  Reported per leg: the median
window (µs per call), the fastest and the slowest, rows per second, and the share of the 8 TB/s HBM peak on input-once plus
output-once bytes; then the ratios of the fbank leg to (a) and (b).  Prints one JSON line.  Measuring only: not collected by pytest, not
part of bench.py.

--pcm16: the same two shapes (dense fbank-80 and packed fbank-80) fed signed 16-bit PCM, three legs each under the same protocol (at
least five windows):
  *_float (a)          ss_kaldi_fbank[_packed]_device on a ready float buffer
  *_convert_float (b)  pcm.to(float32).mul_(scale) and then that float call: what a caller with an int16 corpus ran before
  *_pcm (c)            ss_kpcm_fbank[_packed]_device on the int16 buffer (scale 2^-15)
Every leg reports min / median / max over the windows, so the run's own spread is visible; then (c) over (b), (c) over (a), and whether
(c)'s median lies above (b)'s by more than the spread (max - min) of (b)'s windows -- the PCM build being slower than what it replaces.
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


def pcm16_report(args):
    """the --pcm16 run: see the module docstring"""
    import numpy as np
    import torch

    import speechsauce_amd as ss
    from speechsauce_amd import _lib

    lib = _lib.lib()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    B, L = args.clips, int(round(args.seconds * 16000))
    T = 1 + (L - 400) // 160
    scale = 2.0 ** -15
    windows = max(5, args.windows)
    gen = torch.Generator(device="cuda").manual_seed(0)

    def rings(numel):
        """(int16 blocks, the float blocks of the same samples): each ring adds up to at least --ring-mib MiB"""
        n = max(2, -(-args.ring_mib * (1 << 20) // (2 * numel)))
        pcm = [torch.randint(-32768, 32768, (numel,), device="cuda", generator=gen, dtype=torch.int32).to(torch.int16) for _ in range(n)]
        n_f = max(2, -(-args.ring_mib * (1 << 20) // (4 * numel)))
        return pcm, [pcm[i].to(torch.float32).mul_(scale) for i in range(n_f)]

    key80 = (16000, 25.0, 10.0, 80, 0, 20.0, 0.0, 0.97, 0.0, "povey", 0.42, True, True, False, True, 1.0, 1.0)
    k80 = ss._get_kaldi_config(key80, 0)
    h = k80.handle
    legs = {}  # name -> (call(i), rows, bytes)

    pcm_d, flt_d = rings(B * L)
    out, en = torch.empty((B, T, 80), device="cuda"), torch.empty((B, T), device="cuda")
    outs = (out.data_ptr(), en.data_ptr(), stream)

    def dense_float(i, x=None):
        x = flt_d[i % len(flt_d)] if x is None else x
        _lib.check(lib.ss_kaldi_fbank_device(h, x.data_ptr(), B, L, L, *outs))
        return x  # (kept by the caller until the launch is queued)

    def dense_convert(i):
        dense_float(i, pcm_d[i % len(pcm_d)].to(torch.float32).mul_(scale))

    def dense_pcm(i):
        _lib.check(lib.ss_kpcm_fbank_device(h, pcm_d[i % len(pcm_d)].data_ptr(), B, L, L, scale, *outs))

    out_b = 4 * B * T * 81
    legs["dense_float"] = (dense_float, B * T, 4 * B * L + out_b)
    legs["dense_convert_float"] = (dense_convert, B * T, 10 * B * L + out_b)
    legs["dense_pcm"] = (dense_pcm, B * T, 2 * B * L + out_b)

    rng = np.random.default_rng(0)
    lens = rng.integers(16000, 16 * 16000 + 1, B).astype(np.int64)
    so = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    fo = np.empty_like(so)
    _lib.check(lib.ss_kaldi_packed_frame_offsets(C.byref(k80.params), B, so.ctypes.data, fo.ctypes.data))
    total_in, rows_p = int(so[-1]), int(fo[-1])
    pcm_p, flt_p = rings(total_in)
    dso, dfo = torch.from_numpy(so).cuda(), torch.from_numpy(fo).cuda()
    out_p, en_p = torch.empty((rows_p, 80), device="cuda"), torch.empty((rows_p,), device="cuda")
    outs_p = (out_p.data_ptr(), en_p.data_ptr(), stream)

    def packed_float(i, x=None):
        x = flt_p[i % len(flt_p)] if x is None else x
        _lib.check(lib.ss_kaldi_fbank_packed_device(h, x.data_ptr(), B, dso.data_ptr(), dfo.data_ptr(), rows_p, *outs_p))
        return x

    def packed_convert(i):
        packed_float(i, pcm_p[i % len(pcm_p)].to(torch.float32).mul_(scale))

    def packed_pcm(i):
        _lib.check(lib.ss_kpcm_fbank_packed_device(h, pcm_p[i % len(pcm_p)].data_ptr(), B, dso.data_ptr(), scale, dfo.data_ptr(), rows_p, *outs_p))

    out_b = 4 * rows_p * 81
    legs["packed_float"] = (packed_float, rows_p, 4 * total_in + out_b)
    legs["packed_convert_float"] = (packed_convert, rows_p, 10 * total_in + out_b)
    legs["packed_pcm"] = (packed_pcm, rows_p, 2 * total_in + out_b)

    # what is compared computes the same bits; the kernels that ran
    names = {}
    for name, (call, _, _) in legs.items():
        call(0)
        call(1)
        torch.cuda.synchronize()
        names[name] = lib.ss_last_kernel_name().decode()
    for shape, o in (("dense", out), ("packed", out_p)):
        legs[f"{shape}_float"][0](0)
        want = o.clone()
        legs[f"{shape}_pcm"][0](0)
        torch.cuda.synchronize()
        assert torch.equal(o, want), f"{shape}: the PCM call is not the float call bit for bit"

    times = {name: [] for name in legs}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    it = 2
    for _ in range(windows):
        for name, (call, _, _) in legs.items():
            e0.record()
            for r in range(args.reps):
                call(it + r)
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e3 / args.reps)
            it += args.reps
    k80.device_status()

    report = {"pcm16": True, "scale": scale, "clips": B, "seconds": args.seconds, "frames_per_clip": T, "reps": args.reps, "windows": windows,
              "ring_blocks": {"dense_pcm": len(pcm_d), "dense_float": len(flt_d), "packed_pcm": len(pcm_p), "packed_float": len(flt_p)},
              "packed_rows": rows_p, "device": torch.cuda.get_device_name(), "legs": {}}
    for name, (_, rows, nbytes) in legs.items():
        med = statistics.median(times[name])
        report["legs"][name] = {"kernel": names[name], "us_min": round(min(times[name]), 2), "us_median": round(med, 2),
                                "us_max": round(max(times[name]), 2), "rows_per_s": round(rows / (med * 1e-6)), "bytes_per_call": nbytes,
                                "hbm_fraction": round(nbytes / (med * 1e-6) / HBM_PEAK, 4)}
    for shape in ("dense", "packed"):
        a, b, c = (report["legs"][f"{shape}_{k}"] for k in ("float", "convert_float", "pcm"))
        report[f"{shape}_pcm_over_convert_float"] = round(c["us_median"] / b["us_median"], 3)
        report[f"{shape}_pcm_over_float"] = round(c["us_median"] / a["us_median"], 3)
        report[f"{shape}_pcm_slower_than_convert_float"] = c["us_median"] - b["us_median"] > b["us_max"] - b["us_min"]
    print(json.dumps(report))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=1024)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--windows", type=int, default=10)
    ap.add_argument("--ring-mib", type=int, default=300)
    ap.add_argument("--pcm16", action="store_true", help="time the 16-bit PCM calls beside the float calls (see the module docstring)")
    args = ap.parse_args()
    if args.pcm16:
        return pcm16_report(args)

    import numpy as np
    import torch

    import speechsauce_amd as ss
    from speechsauce_amd import _lib

    lib = _lib.lib()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    B, L = args.clips, int(round(args.seconds * 16000))
    flen, shift, N = 400, 160, 512
    T = 1 + (L - flen) // shift
    gen = torch.Generator(device="cuda").manual_seed(0)

    def ring(numel):
        n = max(2, -(-args.ring_mib * (1 << 20) // (4 * numel)))
        return [torch.randn(numel, device="cuda", generator=gen) * 0.1 for _ in range(n)]

    dense = [b.view(B, L) for b in ring(B * L)]
    legs = {}  # name -> (call(i), reps, rows, bytes, kernel name or None)

    # ---- the Kaldi legs ----
    key80 = (16000, 25.0, 10.0, 80, 0, 20.0, 0.0, 0.97, 0.0, "povey", 0.42, True, True, False, True, 1.0, 1.0)
    k80 = ss._get_kaldi_config(key80, 0)
    out80 = torch.empty((B, T, 80), device="cuda")
    en80 = torch.empty((B, T), device="cuda")

    def kaldi_fbank(i):
        _lib.check(lib.ss_kaldi_fbank_device(k80.handle, dense[i % len(dense)].data_ptr(), B, L, L, out80.data_ptr(), en80.data_ptr(), stream))

    legs["kaldi_fbank80"] = (kaldi_fbank, args.reps, B * T, 4 * (B * L + B * T * 81))
    key13 = (16000, 25.0, 10.0, 23, 13, 20.0, 0.0, 0.97, 22.0, "povey", 0.42, True, True, False, True, 1.0, 1.0)
    k13 = ss._get_kaldi_config(key13, 0)
    out13 = torch.empty((B, T, 13), device="cuda")

    def kaldi_mfcc(i):
        _lib.check(lib.ss_kaldi_mfcc_device(k13.handle, dense[i % len(dense)].data_ptr(), B, L, L, out13.data_ptr(), stream))

    legs["kaldi_mfcc13"] = (kaldi_mfcc, args.reps, B * T, 4 * (B * L + B * T * 13))

    # ---- (a) the nearest existing kernel ----
    cfg_a = ss.SpeechConfig(ss.make_params(sample_rate=16000, frame_length=0.025, frame_stride=0.01, num_filters=80, num_cepstral=13,
                                           spectrum_exponent=2, mfcc_window="hann"))
    Ta = cfg_a.num_frames(L)
    feat_a = torch.empty((B, Ta, 80), device="cuda")
    en_a = torch.empty((B, Ta), device="cuda")

    def mfe_a(i):
        _lib.check(lib.ss_mfe_batch_device(cfg_a.handle, dense[i % len(dense)].data_ptr(), B, L, L, feat_a.data_ptr(), en_a.data_ptr(), stream))

    legs["mfe80_c256w"] = (mfe_a, args.reps, B * Ta, 4 * (B * L + B * Ta * 81))

    # ---- (b) plain torch ----
    p = _lib.SsKaldiParams()
    _lib.check(lib.ss_kaldi_params_default(C.byref(p), 16000))
    p.num_mel_bins = 80
    w_h = np.zeros(flen, np.float32)
    bank_h = np.zeros((80, N // 2), np.float32)
    _lib.check(lib.ss_kaldi_window(C.byref(p), w_h.ctypes.data))
    _lib.check(lib.ss_kaldi_mel_bank(C.byref(p), bank_h.ctypes.data))
    w_d, bank_d = torch.from_numpy(w_h).cuda(), torch.from_numpy(bank_h).cuda().t().contiguous()
    eps = torch.tensor(1.1920929e-7, device="cuda")

    def torch_fbank(x):
        s = x.unfold(1, flen, shift)
        s = s - s.mean(dim=2, keepdim=True)
        prev = torch.cat([s[..., :1], s[..., :-1]], dim=2)
        y = (s - 0.97 * prev) * w_d
        spec = torch.fft.rfft(y, n=N, dim=2)[..., : N // 2]
        return torch.log(torch.maximum((spec.real ** 2 + spec.imag ** 2) @ bank_d, eps))

    def torch_leg(i):
        torch_fbank(dense[i % len(dense)])

    legs["torch_fbank80"] = (torch_leg, max(1, args.reps // 5), B * T, 4 * (B * L + B * T * 80))

    # ---- packed ----
    rng = np.random.default_rng(0)
    lens = rng.integers(16000, 16 * 16000 + 1, B).astype(np.int64)
    so = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    fo = np.empty_like(so)
    _lib.check(lib.ss_kaldi_packed_frame_offsets(C.byref(k80.params), B, so.ctypes.data, fo.ctypes.data))
    total_in, rows_p = int(so[-1]), int(fo[-1])
    packed = ring(total_in)
    dso, dfo = torch.from_numpy(so).cuda(), torch.from_numpy(fo).cuda()
    out_p = torch.empty((rows_p, 80), device="cuda")
    en_p = torch.empty((rows_p,), device="cuda")

    def kaldi_packed(i):
        _lib.check(lib.ss_kaldi_fbank_packed_device(k80.handle, packed[i % len(packed)].data_ptr(), B, dso.data_ptr(), dfo.data_ptr(), rows_p,
                                                    out_p.data_ptr(), en_p.data_ptr(), stream))

    legs["kaldi_fbank80_packed"] = (kaldi_packed, args.reps, rows_p, 4 * (total_in + rows_p * 81))

    # ---- correctness of what is compared, and the kernels that ran ----
    names = {}
    for name, (call, _, _, _) in legs.items():
        call(0)
        call(1)
        torch.cuda.synchronize()
        names[name] = "torch" if name.startswith("torch") else lib.ss_last_kernel_name().decode()
    assert names["mfe80_c256w"] == "ss_mfcc_c256w<13,pow2,mfe,win>", names["mfe80_c256w"]
    kaldi_fbank(0)
    ref = torch_fbank(dense[0])
    torch.cuda.synchronize()
    parity = float((out80 - ref).abs().max() / ref.abs().max())

    times = {name: [] for name in legs}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    it = 2
    for _ in range(args.windows):
        for name, (call, reps, _, _) in legs.items():
            e0.record()
            for r in range(reps):
                call(it + r)
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e3 / reps)
            it += reps
    k80.device_status()

    report = {"clips": B, "seconds": args.seconds, "frames_per_clip": T, "reps": args.reps, "windows": args.windows,
              "ring_blocks_dense": len(dense), "ring_blocks_packed": len(packed), "packed_rows": rows_p,
              "fbank_vs_torch_block_metric": parity, "legs": {}}
    for name, (_, reps, rows, nbytes) in legs.items():
        med = statistics.median(times[name])
        report["legs"][name] = {"kernel": names[name], "us_per_call": round(med, 2), "us_min": round(min(times[name]), 2),
                                "us_max": round(max(times[name]), 2), "rows_per_s": round(rows / (med * 1e-6)), "bytes_per_call": nbytes,
                                "hbm_fraction": round(nbytes / (med * 1e-6) / HBM_PEAK, 4)}
    us = {name: report["legs"][name]["us_per_call"] for name in legs}
    report["fbank_over_mfe_a"] = round(us["kaldi_fbank80"] / us["mfe80_c256w"], 3)
    report["torch_b_over_fbank"] = round(us["torch_fbank80"] / us["kaldi_fbank80"], 2)
    print(json.dumps(report))


if __name__ == "__main__":
    main()
