"""µs per call of reverberation on packed clips: ss_reverb_packed[_i16]_device beside the copy that is the floor of any out-of-place
pass over the block and beside what a user writes in torch with the lengths already known on the host, from one process.

    python tools/reverb_rate.py [--clips 1024] [--reps 5] [--torch-reps 2] [--rounds 5] [--ring 2]

Workloads at 16 kHz: `--clips` clips of 1 .. 16 s (uniform; about 139 M samples) and 16 clips of 60 s; a bank of 64 synthetic responses
of 4000 .. 16000 taps (decaying noise; 8 .. 32 partitions of 512 taps), unit energy, not peak-aligned (so that the torch leg needs no
per-clip shift).  prob 1.  Legs:
  reverb_f32          the combined call into a second block: plan launch, apply launch, epoch bump
  reverb_i16          the signal as 16-bit PCM, out float
  reverb_f32_16x60s   sixteen one-minute clips: 64 workgroups per clip
  copy_floor          out.copy_(x) of the 1024-clip block
  torch_fft           the same stage in torch: pad every clip to the longest (a boolean mask from the host-known lengths), one batched rfft
                      at the next power of two past longest clip + longest response, times the drawn responses' spectra (computed once,
                      gathered per call), irfft, trim, repack through the mask
Before anything is timed the product call's output is held to the torch leg's by the block metric (1e-4 of the block's largest value).
Protocol: every leg is warmed up, then `--rounds` rounds alternate the legs, each timed with HIP events around back-to-back calls on
one stream; every call takes the next of a ring of `--ring` blocks.  Reported per leg: the median over the rounds, the fastest and the
slowest round.
Prints one JSON line.  Measuring only: not collected by pytest, not part of bench.py.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mfcc-rust_amd"))

RATE = 16000
PCM = 2.0 ** -15
N_RIR = 64


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--torch-reps", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--ring", type=int, default=2)
    args = ap.parse_args()

    import numpy as np
    import torch

    import speechsauce_amd as ss

    rng = np.random.default_rng(0)
    rir_lens = rng.integers(4000, 16001, N_RIR)
    rirs = np.concatenate([(rng.standard_normal(k) * np.exp(-np.arange(k) / (k / 5.0))).astype(np.float32) for k in rir_lens])
    bank = ss.ReverbBank(rirs, rir_lens, normalize="energy", align_peak=False)
    taps = [torch.from_numpy(bank.rir(c)[0]).cuda() for c in range(N_RIR)]
    aug = ss.SpecAugment(2026, 0)
    at = [0]
    res = {"responses": N_RIR, "taps_total": int(rir_lens.sum()), "partitions": bank.n_partitions, "block": bank.block, "reps": args.reps,
           "torch_reps": args.torch_reps, "rounds": args.rounds, "ring": args.ring, "device": torch.cuda.get_device_name()}

    class Load:
        def __init__(self, lens):
            self.n, self.lens = len(lens), np.asarray(lens, np.int64)
            self.so = np.concatenate([[0], np.cumsum(self.lens)]).astype(np.int64)
            self.total, self.longest = int(self.so[-1]), int(self.lens.max())
            self.d_so, self.d_lens = torch.from_numpy(self.so).cuda(), torch.from_numpy(self.lens).cuda()
            self.ins = [torch.randn(self.total, device="cuda").mul_(0.1) for _ in range(args.ring)]
            self.ins_i16 = [(x / PCM).round().clamp(-32768, 32767).to(torch.int16) for x in self.ins]
            self.outs = [torch.empty(self.total, device="cuda") for _ in range(args.ring)]
            self.plan = None

        def reverb(self, src, dst):
            _, self.plan = ss.reverb_packed(src, None, bank, aug, 1.0, pcm_scale=PCM if src.dtype == torch.int16 else None, out=dst, device_tables=self.d_so)

        def torch_setup(self):
            self.nfft = 1 << int(self.longest + int(rir_lens.max()) - 1).bit_length()
            self.mask = torch.arange(self.longest, device="cuda")[None, :] < self.d_lens[:, None]
            self.spectra = torch.stack([torch.fft.rfft(h, n=self.nfft) for h in taps])

        def torch_fft(self, x, which):
            padded = torch.zeros((self.n, self.longest), device="cuda")
            padded[self.mask] = x
            y = torch.fft.irfft(torch.fft.rfft(padded, n=self.nfft) * self.spectra[which], n=self.nfft)
            return y[:, :self.longest][self.mask]

    big = Load(rng.integers(1 * RATE, 16 * RATE + 1, args.clips))
    long16 = Load(np.full(16, 60 * RATE))
    res.update(clips=big.n, samples_packed=big.total, samples_16x60s=long16.total)
    big.torch_setup()
    res["torch_fft_points"] = big.nfft

    # the check: one product call against the torch leg on the plan it drew
    big.reverb(big.ins[0], big.outs[0])
    torch.cuda.synchronize()
    rows = ss.reverb_plan_rows(big.plan)
    assert (rows["rir"] >= 0).all() and (rows["shift"] == 0).all()
    which = torch.from_numpy(rows["rir"].astype(np.int64)).cuda()
    want = big.torch_fft(big.ins[0], which)
    err = float((big.outs[0] - want).abs().max() / want.abs().max())
    assert err <= 1e-4, err
    res["block_error_against_torch"] = err
    del want
    draw = torch.randint(0, N_RIR, (big.n,), device="cuda")

    def ring(fn):
        def leg():
            at[0] += 1
            fn(at[0] % args.ring)
        return leg

    legs = [("reverb_f32", ring(lambda i: big.reverb(big.ins[i], big.outs[i])), args.reps),
            ("reverb_i16", ring(lambda i: big.reverb(big.ins_i16[i], big.outs[i])), args.reps),
            ("reverb_f32_16x60s", ring(lambda i: long16.reverb(long16.ins[i], long16.outs[i])), args.reps),
            ("copy_floor", ring(lambda i: big.outs[i].copy_(big.ins[i])), args.reps),
            ("torch_fft", ring(lambda i: big.torch_fft(big.ins[i], draw)), args.torch_reps)]

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
    res["reverb_f32"]["over_copy_floor"] = res["reverb_f32"]["us_per_call_median"] / res["copy_floor"]["us_per_call_median"]
    res["torch_fft"]["over_reverb_f32"] = res["torch_fft"]["us_per_call_median"] / res["reverb_f32"]["us_per_call_median"]
    res["reverb_f32"]["samples_per_us"] = big.total / res["reverb_f32"]["us_per_call_median"]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
