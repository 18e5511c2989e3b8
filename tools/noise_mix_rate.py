"""µs per call of noise mixing on packed clips: ss_noise_mix_packed[_i16]_device beside the copy that is the floor of any out-of-place
pass over the block and beside what a user writes in torch with the lengths already known on the host, from one process.

    python tools/noise_mix_rate.py [--clips 1024] [--reps 10] [--torch-reps 3] [--rounds 5] [--ring 2]

Workloads at 16 kHz: `--clips` clips of 1 .. 16 s (uniform; about 139 M samples) and 16 clips of 60 s; a bank of 64 noise clips of
5 .. 30 s (about 18 M samples, 72 MB as floats: it fits the Infinity Cache, so the noise reads may be served there).  prob 1, SNR
10 .. 30 dB, gain -6 .. 6 dB.  Legs:
  mix_f32           the combined call into a second block: energy launch, fold launch, apply launch, epoch bump
  mix_inplace_f32   the same with out == x
  mix_i16           signal and bank as 16-bit PCM, out float
  mix_f32_16x60s    sixteen one-minute clips: the energy launch still fills the device (64 workgroups per clip)
  copy_floor        out.copy_(x) of the 1024-clip block
  torch_mix         the same stage in torch on the packed samples: clip id and local index of every sample from repeat_interleave /
                    arange on the host-known lengths, the noise operand by an index gather with modulo, per-clip f64 energies by
                    segment_reduce, gains, addcmul
bytes_per_call is speech once + noise once + out once (12 bytes per sample, 8 for the PCM leg; the call itself reads speech and noise
twice, once per pass); hbm_fraction reads it against 8.0 TB/s.  Before anything is timed the SNR each clip of one call reached, from
torch's own f64 sums, is held to the plan's snr_db within 0.01 dB.
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
RATE = 16000
SCALARS = (1.0, 10.0, 30.0, -6.0, 6.0)  # prob, SNR range, gain range
PCM = 2.0 ** -15


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--torch-reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--ring", type=int, default=2)
    args = ap.parse_args()

    import numpy as np
    import torch

    import speechsauce_amd as ss
    from speechsauce_amd import _lib

    lib = _lib.lib()
    sp = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rng = np.random.default_rng(0)
    noise_lens = rng.integers(5 * RATE, 30 * RATE + 1, 64)
    no = np.zeros(65, np.int64)
    np.cumsum(noise_lens, out=no[1:])
    total_noise = int(no[-1])
    d_no, d_nlens = torch.from_numpy(no).cuda(), torch.from_numpy(noise_lens).cuda()
    bank = torch.randn(total_noise, device="cuda").mul_(0.03)
    bank_i16 = (bank / (PCM / 4)).round().clamp(-32768, 32767).to(torch.int16)
    block = torch.from_numpy(np.array([2026, 0], np.uint64).view(np.int64)).cuda()
    at = [0]
    res = {"noise_clips": 64, "noise_samples": total_noise, "reps": args.reps, "torch_reps": args.torch_reps, "rounds": args.rounds, "ring": args.ring,
           "device": torch.cuda.get_device_name()}

    class Load:
        def __init__(self, lens):
            self.n, self.lens = len(lens), lens
            self.so = np.zeros(self.n + 1, np.int64)
            np.cumsum(lens, out=self.so[1:])
            self.total = int(self.so[-1])
            self.d_so, self.d_lens = torch.from_numpy(self.so).cuda(), torch.from_numpy(np.asarray(lens, np.int64)).cuda()
            self.ins = [torch.randn(self.total, device="cuda").mul_(0.1) for _ in range(args.ring)]
            self.ins_i16 = [(x / PCM).round().clamp(-32768, 32767).to(torch.int16) for x in self.ins]
            self.outs = [torch.empty(self.total, device="cuda") for _ in range(args.ring)]
            self.plan = torch.zeros((self.n, 5), dtype=torch.int64, device="cuda")
            need = C.c_size_t()
            _lib.check(lib.ss_noise_mix_work_bytes(self.n, self.total, C.byref(need)))
            self.work = torch.empty(need.value // 8, dtype=torch.float64, device="cuda")

        def mix(self, src, dst):
            assert src.shape == dst.shape == (self.total,)
            if src.dtype == torch.int16:
                _lib.check(lib.ss_noise_mix_packed_i16_device(src.data_ptr(), PCM, self.n, self.d_so.data_ptr(), self.total, bank_i16.data_ptr(), PCM / 4, 64,
                                                              d_no.data_ptr(), total_noise, block.data_ptr(), 0, *SCALARS, dst.data_ptr(),
                                                              self.plan.data_ptr(), self.work.data_ptr(), self.work.numel() * 8, sp))
            else:
                _lib.check(lib.ss_noise_mix_packed_device(src.data_ptr(), self.n, self.d_so.data_ptr(), self.total, bank.data_ptr(), 64, d_no.data_ptr(),
                                                          total_noise, block.data_ptr(), 0, *SCALARS, dst.data_ptr(), self.plan.data_ptr(),
                                                          self.work.data_ptr(), self.work.numel() * 8, sp))

        def sample_index(self):
            """the clip id and the local index of every packed sample, from the host-known lengths (no read-back)"""
            cid = torch.repeat_interleave(torch.arange(self.n, device="cuda"), self.d_lens, output_size=self.total)
            return cid, torch.arange(self.total, device="cuda") - self.d_so[cid]

        def torch_mix(self, x):
            u = torch.rand((self.n, 4), device="cuda", dtype=torch.float64)
            c = (u[:, 0] * 64).long()
            period = d_nlens[c]
            start = (u[:, 1] * period).long()
            snr = SCALARS[1] + (SCALARS[2] - SCALARS[1]) * u[:, 2]
            gain = 10.0 ** ((SCALARS[3] + (SCALARS[4] - SCALARS[3]) * u[:, 3]) / 20.0)
            cid, local = self.sample_index()
            seg = bank[d_no[c][cid] + (start[cid] + local) % period[cid]]
            es = torch.segment_reduce(x.double().square_(), "sum", lengths=self.d_lens)
            en = torch.segment_reduce(seg.double().square_(), "sum", lengths=self.d_lens)
            ng = (gain * torch.sqrt(es / en) * 10.0 ** (-snr / 20.0)).float()
            return torch.addcmul(x * gain.float()[cid], seg, ng[cid])

    big = Load(rng.integers(1 * RATE, 16 * RATE + 1, args.clips))
    long16 = Load(np.full(16, 60 * RATE))
    res.update(clips=big.n, samples_packed=big.total, samples_16x60s=long16.total)

    # the check: the SNR every clip of one call reached, from torch's own f64 sums, against the plan
    for load in (big, long16):
        load.mix(load.ins[0], load.outs[0])
        torch.cuda.synchronize()
        rows = ss.noise_plan_rows(load.plan)
        assert (rows["noise_clip"] >= 0).all() and (rows["noise_gain"] > 0).all()
        cid, _ = load.sample_index()
        s = load.ins[0].double() * torch.from_numpy(rows["speech_gain"].astype(np.float64)).cuda()[cid]
        num = torch.segment_reduce(s.square(), "sum", lengths=load.d_lens)
        den = torch.segment_reduce((load.outs[0].double() - s).square_(), "sum", lengths=load.d_lens)
        reached = (10.0 * torch.log10(num / den)).cpu().numpy()
        assert np.abs(reached - rows["snr_db"]).max() < 0.01, np.abs(reached - rows["snr_db"]).max()
        del s, num, den, cid
    assert torch.isfinite(big.torch_mix(big.ins[0])).all()

    def ring(fn):
        def leg():
            at[0] += 1
            fn(at[0] % args.ring)
        return leg

    legs = [("mix_f32", ring(lambda i: big.mix(big.ins[i], big.outs[i])), args.reps, 12 * big.total),
            ("mix_inplace_f32", ring(lambda i: big.mix(big.ins[i], big.ins[i])), args.reps, 12 * big.total),
            ("mix_i16", ring(lambda i: big.mix(big.ins_i16[i], big.outs[i])), args.reps, 8 * big.total),
            ("mix_f32_16x60s", ring(lambda i: long16.mix(long16.ins[i], long16.outs[i])), args.reps, 12 * long16.total),
            ("copy_floor", ring(lambda i: big.outs[i].copy_(big.ins[i])), args.reps, 8 * big.total),
            ("torch_mix", ring(lambda i: big.torch_mix(big.ins[i])), args.torch_reps, 12 * big.total)]

    def timed(fn, reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / reps * 1e3

    for _, fn, _, _ in legs:  # warm-up: code objects, the allocator's blocks, every buffer of the ring once
        for _ in range(args.ring):
            fn()
    torch.cuda.synchronize()
    us = {name: [] for name, _, _, _ in legs}
    for _ in range(args.rounds):
        for name, fn, reps, _ in legs:
            us[name].append(timed(fn, reps))
    for name, _, _, nbytes in legs:
        v = us[name]
        leg = res[name] = {"us_per_call_median": statistics.median(v), "us_min": min(v), "us_max": max(v), "bytes_per_call": nbytes}
        leg["gb_per_s"] = nbytes / leg["us_per_call_median"] * 1e-3
        leg["hbm_fraction"] = leg["gb_per_s"] * 1e9 / HBM_PEAK
    res["mix_f32"]["over_copy_floor"] = res["mix_f32"]["us_per_call_median"] / res["copy_floor"]["us_per_call_median"]
    res["torch_mix"]["over_mix_f32"] = res["torch_mix"]["us_per_call_median"] / res["mix_f32"]["us_per_call_median"]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
