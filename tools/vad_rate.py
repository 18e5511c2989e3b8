"""µs per call of the energy VAD and the voiced-row selection: ss_vad_energy_packed_device and ss_select_rows_packed_device on a packed
block, each beside the torch restatement a user writes without it, and ss_vad_energy_stream_packed_device over a pool of stream states
beside its torch restatement, the MFCC pool call and the add-deltas pool call on the same tables, all from one process.

    python tools/vad_rate.py [--clips 1024] [--pool 4096] [--active 1024] [--max-rows 4] [--reps 30] [--rounds 7] [--ring 8]

Packed workload: `--clips` clips of 1 .. 16 s (98 .. 1598 rows at 100 rows/s, uniform; about 891 k rows), cols = 13 and 40, the energy
in column 0, the x-vector recipes' scalars (5.5 / 0.5 / 2 / 0.12).  Every call takes the next of a ring of input blocks that together
exceed the 256 MiB Infinity Cache, so no call finds its input cached by the one before it.
  torch_vad: the padded VAD -- the energies gathered into [clips, T_max] through a prebuilt index, the masked mean, the comparison, the
  window counts by conv1d, the bytes gathered back through a prebuilt index (no host sync).
  torch_select: `x[mask]` (which synchronises: the output size is data dependent) plus the recount of the offsets, a cumsum of the mask
  gathered at the prebuilt clip ends.
  The selection's bytes_per_call is vec once, the mask twice, the kept rows once; hbm_fraction reads it against 8.0 TB/s.
Pool workload: a pool of `--pool` streams of which `--active` deliver 1 .. `--max-rows` rows in a tick (uniform), in random slot order,
every stream in steady state; cols = 13.  torch_vad_pool keeps (sum, rows seen, last 2 L energies) per stream in three tensors and
decides a tick padded to [active, max_rows] through prebuilt indices.
Protocol: every leg is warmed up, then `--rounds` rounds alternate the legs, each timed with HIP events around `--reps` back-to-back
calls on one stream.  Reported per leg: the median over the rounds, the fastest and the slowest round.
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

STEP, S, NCEP = 160, 160, 13
HBM_PEAK = 8.0e12
THR, SCALE, L, PROP = 5.5, 0.5, 2, 0.12
CACHE = 256 << 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=1024)
    ap.add_argument("--pool", type=int, default=4096)
    ap.add_argument("--active", type=int, default=1024)
    ap.add_argument("--max-rows", type=int, default=4)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--ring", type=int, default=8)
    args = ap.parse_args()

    import numpy as np
    import torch
    import torch.nn.functional as F

    import speechsauce_amd as ss
    from speechsauce_amd import _lib

    lib = _lib.lib()
    P, N, H = args.pool, args.active, args.max_rows
    sp = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    cfg = ss.SpeechConfig(_lib.make_params())
    rng = np.random.default_rng(0)
    W = 2 * L + 1
    box = torch.ones((1, 1, W), device="cuda")

    # ---- packed ----
    n_clips = args.clips
    lens = rng.integers(98, 1599, n_clips)
    ro = np.zeros(n_clips + 1, np.int64)
    np.cumsum(lens, out=ro[1:])
    R, Tmax = int(ro[-1]), int(lens.max())
    d_ro = torch.from_numpy(ro).cuda()
    d_len = torch.from_numpy(lens).cuda().to(torch.float32)
    pad_idx = np.minimum(ro[:-1, None] + np.arange(Tmax)[None, :], R - 1)       # [clips, Tmax] row of (clip, t)
    valid = np.arange(Tmax)[None, :] < lens[:, None]
    flat_idx = np.flatnonzero(valid.reshape(-1))                                   # the padded place of every packed row
    d_pad, d_valid, d_flat = torch.from_numpy(pad_idx).cuda(), torch.from_numpy(valid).cuda(), torch.from_numpy(flat_idx).cuda()
    d_validf = d_valid.to(torch.float32)
    den = F.conv1d(d_validf[:, None, :], box, padding=L)[:, 0, :] * PROP          # den * p: the same for every call
    d_ends = torch.from_numpy(ro[1:]).cuda()
    legs, kept_fraction, sel_bytes = [], {}, {}
    for c in (13, 40):
        n_in = int(min(8, max(2, -(-2 * CACHE // (R * c * 4)))))
        blocks = []
        for _ in range(n_in):
            b = torch.randn((R, c), device="cuda").mul_(3).add_(1)
            b[:, 0] = torch.randn(R, device="cuda").mul_(2).add_(8)
            blocks.append(b)
        mask = torch.empty(R, dtype=torch.uint8, device="cuda")
        counts = torch.empty(n_clips, dtype=torch.int64, device="cuda")
        oo = torch.empty(n_clips + 1, dtype=torch.int64, device="cuda")
        out = torch.empty((R, c), device="cuda")
        at = [0]

        def block(at=at, blocks=blocks):
            at[0] += 1
            return blocks[at[0] % len(blocks)]

        def vad(c=c, mask=mask, counts=counts, block=block):
            _lib.check(lib.ss_vad_energy_packed_device(block().data_ptr(), n_clips, d_ro.data_ptr(), R, c, 0, THR, SCALE, L, PROP, mask.data_ptr(),
                                                       counts.data_ptr(), sp))

        def torch_vad(block=block):
            e = block()[:, 0][d_pad] * d_validf
            thr = THR + SCALE * (e.sum(1) / d_len)
            raw = ((e > thr[:, None]) & d_valid).to(torch.float32)
            num = F.conv1d(raw[:, None, :], box, padding=L)[:, 0, :]
            return (num >= den).reshape(-1)[d_flat].to(torch.uint8)

        _lib.check(lib.ss_vad_energy_packed_device(blocks[0].data_ptr(), n_clips, d_ro.data_ptr(), R, c, 0, THR, SCALE, L, PROP, mask.data_ptr(),
                                                   counts.data_ptr(), sp))
        torch.cuda.synchronize()
        kept = int(mask.sum())
        kept_fraction[c] = kept / R
        sel_bytes[c] = R * c * 4 + 2 * R + kept * c * 4
        sel_mask = mask.clone()  # the selection legs: the mask of block 0 on every block (the bytes moved do not depend on the rows)
        sel_bool = sel_mask.bool()

        def select(c=c, oo=oo, out=out, block=block, sel_mask=sel_mask):
            _lib.check(lib.ss_select_rows_packed_device(block().data_ptr(), n_clips, d_ro.data_ptr(), R, c, sel_mask.data_ptr(), oo.data_ptr(),
                                                        out.data_ptr(), sp))

        def torch_select(block=block, sel_bool=sel_bool, sel_mask=sel_mask):
            rows = block()[sel_bool]
            cs = F.pad(torch.cumsum(sel_mask, 0, dtype=torch.int64), (1, 0))
            return rows, F.pad(cs[d_ends], (1, 0))

        legs += [(f"vad_packed_cols{c}", vad), (f"torch_vad_cols{c}", torch_vad), (f"select_packed_cols{c}", select), (f"torch_select_cols{c}", torch_select)]

    # ---- pool: a ring of ticks ----
    c = 13
    ticks = []
    for _ in range(args.ring):
        rows = rng.integers(1, H + 1, N)
        slots = rng.permutation(P)[:N].astype(np.int32)
        r = np.zeros(N + 1, np.int64)
        np.cumsum(rows, out=r[1:])
        total = int(r[-1])
        pidx = np.minimum(r[:-1, None] + np.arange(H)[None, :], total - 1)
        pvalid = np.arange(H)[None, :] < rows[:, None]
        hidx = rows[:, None] + np.arange(2 * L)[None, :]  # the last 2 L of (history ++ entry): columns rows .. rows + 2 L - 1 of seq
        ticks.append({"rows": total, "ro": torch.from_numpy(r).cuda(), "so": torch.from_numpy(r * STEP).cuda(), "slots": torch.from_numpy(slots).cuda(),
                      "lslots": torch.from_numpy(slots.astype(np.int64)).cuda(), "feat": torch.randn((total, c), device="cuda").mul_(2).add_(8),
                      "x": torch.randn(total * STEP, device="cuda").mul_(0.1), "pidx": torch.from_numpy(pidx).cuda(),
                      "pvalid": torch.from_numpy(pvalid).cuda(), "pflat": torch.from_numpy(np.flatnonzero(pvalid.reshape(-1))).cuda(),
                      "hidx": torch.from_numpy(hidx).cuda(), "last": torch.from_numpy(rows - 1).cuda()[:, None],
                      "lens": torch.from_numpy(rows).cuda()})
    tk = [0]

    def nxt():
        tk[0] += 1
        return ticks[tk[0] % args.ring]

    cap = N * H
    fpool = torch.randn((P, S), device="cuda").mul_(0.1)
    fout = torch.empty((cap, NCEP), device="cuda")
    n = C.c_size_t()
    _lib.check(lib.ss_add_deltas_stream_state_len(c, 2, 2, C.byref(n)))
    dpool = torch.randn((P, n.value), device="cuda").mul_(3).add_(1)
    dpool[:, -1] = 8  # steady state: 2 * lag rows of history
    dout = torch.empty((cap, 3 * c), device="cuda")
    _lib.check(lib.ss_vad_energy_stream_state_len(L, C.byref(n)))
    vrows = np.zeros((P, n.value), np.float32)  # steady state: the sum 8000.0 of 1000 rows seen, a full history
    vrows.view(np.uint32)[:, 0:2] = np.array([8000.0]).view(np.uint32)
    vrows.view(np.uint32)[:, 2] = 1000
    vrows[:, 3:3 + 2 * L] = rng.standard_normal((P, 2 * L)) * 2 + 8
    vrows[:, -1] = 2 * L
    vpool = torch.from_numpy(vrows).cuda()
    vmask = torch.empty(cap, dtype=torch.uint8, device="cuda")
    t_sum = torch.full((P,), 8000.0, dtype=torch.float64, device="cuda")
    t_seen = torch.full((P,), 1000, dtype=torch.int64, device="cuda")
    t_hist = torch.randn((P, 2 * L), device="cuda").mul_(2).add_(8)
    ar = torch.arange(1, H + 1, device="cuda")[None, :]

    def mfcc():
        t = nxt()
        _lib.check(lib.ss_mfcc_stream_packed_device(cfg.handle, t["x"].data_ptr(), N, t["so"].data_ptr(), t["ro"].data_ptr(), t["rows"],
                                                    t["slots"].data_ptr(), P, 100, fpool.data_ptr(), fout.data_ptr(), sp))

    def deltas():
        t = nxt()
        _lib.check(lib.ss_add_deltas_stream_packed_device(t["feat"].data_ptr(), N, t["ro"].data_ptr(), t["rows"], t["slots"].data_ptr(), P, c, 2, 2,
                                                          dpool.data_ptr(), dout.data_ptr(), sp))

    def vad_pool():
        t = nxt()
        _lib.check(lib.ss_vad_energy_stream_packed_device(t["feat"].data_ptr(), N, t["ro"].data_ptr(), t["rows"], t["slots"].data_ptr(), P, c, 0, THR,
                                                          SCALE, L, PROP, vpool.data_ptr(), vmask.data_ptr(), sp))

    def torch_vad_pool():
        t = nxt()
        sl = t["lslots"]
        e = t["feat"][:, 0][t["pidx"]] * t["pvalid"]                      # [N, H], zeros past an entry's rows
        cums = t_sum[sl][:, None] + torch.cumsum(e.to(torch.float64), 1)
        thr = (THR + SCALE * (cums / (t_seen[sl][:, None] + ar))).to(torch.float32)
        seq = torch.cat([t_hist[sl], e], 1)                               # [N, 2 L + H]
        num = (seq.unfold(1, W, 1) > thr[:, :, None]).sum(-1)             # [N, H]: row k's window ends at the row that came with byte k
        m = (num.to(torch.float32) >= W * PROP).reshape(-1)[t["pflat"]].to(torch.uint8)
        t_hist[sl] = torch.gather(seq, 1, t["hidx"])
        t_sum[sl] = torch.gather(cums, 1, t["last"])[:, 0]
        t_seen[sl] += t["lens"]
        return m

    legs += [("mfcc_pool", mfcc), ("deltas_pool_cols13", deltas), ("vad_pool_cols13", vad_pool), ("torch_vad_pool_cols13", torch_vad_pool)]

    def timed(fn, reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / reps * 1e3

    for _, fn in legs:  # warm-up: code objects, every input of the ring once
        for _ in range(args.ring):
            fn()
    torch.cuda.synchronize()
    us = {name: [] for name, _ in legs}
    for _ in range(args.rounds):
        for name, fn in legs:
            us[name].append(timed(fn, args.reps))
    res = {"clips": n_clips, "rows_packed": R, "pool": P, "active": N, "max_rows": H, "reps": args.reps, "rounds": args.rounds, "ring": args.ring,
           "scalars": [THR, SCALE, L, PROP], "device": torch.cuda.get_device_name()}
    for name, _ in legs:
        v = us[name]
        res[name] = {"us_per_call_median": statistics.median(v), "us_min": min(v), "us_max": max(v)}
    for c in (13, 40):
        res[f"kept_fraction_cols{c}"] = kept_fraction[c]
        for leg in (res[f"select_packed_cols{c}"], res[f"torch_select_cols{c}"]):
            leg["bytes_per_call"] = sel_bytes[c]
            leg["gb_per_s"] = sel_bytes[c] / leg["us_per_call_median"] * 1e-3
            leg["hbm_fraction"] = leg["gb_per_s"] * 1e9 / HBM_PEAK
        for ours, theirs in ((f"vad_packed_cols{c}", f"torch_vad_cols{c}"), (f"select_packed_cols{c}", f"torch_select_cols{c}")):
            res[theirs]["over_ours"] = res[theirs]["us_per_call_median"] / res[ours]["us_per_call_median"]
    res["torch_vad_pool_cols13"]["over_ours"] = res["torch_vad_pool_cols13"]["us_per_call_median"] / res["vad_pool_cols13"]["us_per_call_median"]
    res["vad_pool_cols13"]["over_mfcc_pool"] = res["vad_pool_cols13"]["us_per_call_median"] / res["mfcc_pool"]["us_per_call_median"]
    res["vad_pool_cols13"]["over_deltas_pool"] = res["vad_pool_cols13"]["us_per_call_median"] / res["deltas_pool_cols13"]["us_per_call_median"]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
