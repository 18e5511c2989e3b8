"""Time of the packed post-processing calls (ss_cmvn_packed_device, ss_cmvnw_packed_device, ss_power_to_db_packed_device) beside
the per-clip loop over the one-matrix calls on views of the same block.

    python tools/post_packed_rate.py [--clips 1024] [--min-s 1] [--max-s 16] [--reps 50] [--loop-reps 3]

Blocks, 16 kHz:
  uniform   the MFCC block tools/packed_rate.py builds: n clips uniform in [min-s, max-s] seconds, default MFCC shape, [sum T_b x 13]
  skewed    one 10-minute clip among n - 1 one-second clips, same shape
  mel       the cfg3 mel block of tools/mel_packed_rate.py ([128 x R_b] pieces) of the uniform clips, for power_to_db
For cmvn(var), cmvnw(301), cmvnw(301, var), cmvnw(31, var) on the MFCC blocks and power_to_db on the mel block, from one process and
alternating the two:
  packed    the packed call (HIP events around --reps calls after warm-up)
  loop      ss.cmvn / ss.cmvnw / ss.power_to_db once per clip on views of the same block: the only correct way without the packed
            calls, and the baseline (HIP events around --loop-reps passes)
  rate      bytes the call must move (block read + block written; cmvnw with variance twice) over the packed time, as a fraction
            of 8 TB/s HBM: an end-to-end rate over peak, not a kernel's share.  The blocks are far smaller than the 256 MiB
            Infinity Cache, so the rates are cache-assisted.
Prints one JSON line.  Measuring only: not collected by pytest, not part of bench.py.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mfcc-rust_amd"))

CFG3 = dict(frame_length=0.032, frame_stride=0.032, num_filters=128, fft_length=2048, high_frequency=8000.0)
HBM_BYTES_PER_S = 8e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=1024)
    ap.add_argument("--min-s", type=float, default=1.0)
    ap.add_argument("--max-s", type=float, default=16.0)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--loop-reps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()

    import torch

    import speechsauce_amd as ss

    sr = 16000
    rng = np.random.default_rng(args.seed)

    def events(fn, reps):
        fn()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / reps * 1e-3

    def compare(packed, loop, nbytes):
        # alternate the two: packed, loop, packed, loop; keep the better of each
        tp, tl = [], []
        for _ in range(2):
            tp.append(events(packed, args.reps))
            tl.append(events(loop, args.loop_reps))
        tp, tl = min(tp), min(tl)
        return {"packed_s": tp, "loop_s": tl, "loop_over_packed": tl / tp, "bytes": nbytes,
                "end_to_end_over_hbm_peak": nbytes / tp / HBM_BYTES_PER_S}

    def mfcc_block(lens):
        x = torch.randn(int(lens.sum()), device="cuda").mul_(0.05)
        feats, fo = ss.mfcc_packed(x, lens, sr)
        return feats, fo, fo.cpu().tolist()

    def post_cases(feats, fo, fol):
        n = len(fol) - 1
        views = [feats[fol[b]:fol[b + 1]] for b in range(n)]
        nbytes = 2 * feats.numel() * 4
        res = {"rows": fol[-1], "cols": feats.shape[1], "clips": n, "longest_clip_rows": max(b - a for a, b in zip(fol, fol[1:]))}
        res["cmvn_var"] = compare(lambda: ss.cmvn_packed(feats, fo, True), lambda: [ss.cmvn(v, True) for v in views], nbytes)
        for win, var in ((301, False), (301, True), (31, True)):
            res[f"cmvnw_{win}{'_var' if var else ''}"] = compare(
                lambda: ss.cmvnw_packed(feats, fo, win, var), lambda: [ss.cmvnw(v, win, var) for v in views], nbytes * (2 if var else 1))
        return res

    res = {"device": torch.cuda.get_device_name(), "reps": args.reps, "loop_reps": args.loop_reps}
    lens = rng.integers(int(args.min_s * sr), int(args.max_s * sr) + 1, args.clips).astype(np.int64)
    res["uniform"] = post_cases(*mfcc_block(lens))
    skew = np.full(args.clips, sr, dtype=np.int64)
    skew[args.clips // 2] = 600 * sr
    res["skewed"] = post_cases(*mfcc_block(skew))

    x = torch.randn(int(lens.sum()), device="cuda").mul_(0.05)
    mel, ro = ss.mel_spectrogram_packed(x, lens, sr, **CFG3)
    rol, M = ro.cpu().tolist(), CFG3["num_filters"]
    views = [mel[M * rol[b]:M * rol[b + 1]] for b in range(args.clips)]
    res["mel"] = {"rows": rol[-1], "cols": M, "clips": args.clips,
                  "power_to_db": compare(lambda: ss.power_to_db_packed(mel, ro, cols=M), lambda: [ss.power_to_db(v) for v in views],
                                         2 * mel.numel() * 4)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
