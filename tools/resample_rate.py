"""µs per call of the resampler: ss_resample_device on a dense batch, ss_resample_packed_device on packed clips, float and 16-bit PCM
input, for 48 kHz -> 16 kHz and 44.1 kHz -> 16 kHz, and ss_resample_stream_packed_device over a pool of stream states beside the MFCC
pool call -- all from one process, next to the baseline a user has today.

    python tools/resample_rate.py [--clips 1024] [--seconds 10] [--pool 4096] [--active 1024] [--max-periods 4] [--reps 20]
                                  [--rounds 5] [--ring 8] [--rates 48000,44100]

Dense workload: `--clips` clips of `--seconds` s.  Packed workload: `--clips` clips of 1 .. 16 s (uniform).  bytes_per_call is the
input once plus the output once (4 or 2 bytes per input sample, 4 per output); hbm_fraction reads it against 8.0 TB/s (the spec
peak; a float4 copy reaches about 79 % of it).  Every leg alternates between two input blocks, each far larger than the 256 MiB
Infinity Cache, so no call finds its samples on the die.
Baseline (needs only torch): conv1d with stride o over the dense [n x (2 width + o)] bank on a zero-padded dense float batch, plus
the interleave of the n phase rows -- torchaudio.functional.resample's own scheme.  For the packed workload it runs on the clips
padded to the longest one (the padding copy is not timed); the PCM legs are compared with the same float baseline (the int16 ->
float copy a user needs first is not timed either).  over_baseline = baseline / library call.
Pool workload: a pool of `--pool` streams of which `--active` deliver 1 .. `--max-periods` periods in a tick, in random slot order,
every stream in steady state, beside ss_mfcc_stream_packed_device on `--active` entries of 1 .. 4 hops.
Protocol: every leg is warmed up, then `--rounds` rounds alternate the legs, each timed with HIP events around `--reps` back-to-back
calls on one stream.  From the second round on a one-wave clock probe (ss_shader_clock_probe_async) is queued on a side stream just
ahead of the leg's launches and sleeps through most of them: clock_ghz is the shader clock the part held during the very launches
that were timed.  Reported per leg: the median over the rounds, the fastest and the slowest round.
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
STEP = 160


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=1024)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--pool", type=int, default=4096)
    ap.add_argument("--active", type=int, default=1024)
    ap.add_argument("--max-periods", type=int, default=4)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--ring", type=int, default=8)
    ap.add_argument("--rates", default="48000,44100")
    args = ap.parse_args()

    import numpy as np
    import torch
    import torch.nn.functional as F

    import speechsauce_amd as ss
    from speechsauce_amd import _lib

    lib = _lib.lib()
    new = 16000
    sp = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    side = torch.cuda.Stream()
    words = torch.zeros(2, dtype=torch.int64, device="cuda")
    rng = np.random.default_rng(0)
    B = args.clips
    legs = []   # (name, call, reps, info)

    def bank(orig):
        """the dense [n x (2 width + o)] f32 bank a user builds today (torchaudio's _get_sinc_resample_kernel, f64 then f32)"""
        rs = ss._get_resampler(orig, new)
        o, n, width, taps = rs.info.o, rs.info.n, rs.info.width, rs.info.taps
        h = np.zeros((n, taps), np.float32)
        first = np.zeros(n, np.int32)
        count = np.zeros(n, np.int32)
        _lib.check(lib.ss_resample_taps(orig, new, 6, 0.99, h.ctypes.data, first.ctypes.data, count.ctypes.data))
        dense = np.zeros((n, 2 * width + o), np.float32)
        for i in range(n):
            dense[i, first[i]:first[i] + count[i]] = h[i, :count[i]]
        return rs, torch.from_numpy(dense).cuda()[:, None, :]

    def baseline(x, kernel, o, width, out_len):
        y = F.conv1d(F.pad(x, (width, width + o))[:, None], kernel, stride=o)   # [B, n, periods]
        return y.transpose(1, 2).reshape(x.shape[0], -1)[:, :out_len]

    for orig in [int(v) for v in args.rates.split(",")]:
        rs, kernel = bank(orig)
        o, n, width = rs.info.o, rs.info.n, rs.info.width
        tag = f"{orig // 1000}k"
        # ---- dense ----
        L = int(args.seconds * orig)
        m = rs.out_len(L)
        xs = [torch.randn((B, L), device="cuda").mul_(0.1) for _ in range(2)]
        ps = [(x * 32768.0).clamp_(-32768, 32767).to(torch.int16) for x in xs]
        out = torch.empty((B, m), device="cuda")
        flip = [0]

        def dense(pcm, xs=xs, ps=ps, rs=rs, L=L, m=m, out=out):
            def call():
                flip[0] ^= 1
                if pcm:
                    _lib.check(lib.ss_resample_i16_device(rs.handle, ps[flip[0]].data_ptr(), B, L, L, 2.0 ** -15, out.data_ptr(), m, sp))
                else:
                    _lib.check(lib.ss_resample_device(rs.handle, xs[flip[0]].data_ptr(), B, L, L, out.data_ptr(), m, sp))
            return call

        def dense_base(xs=xs, kernel=kernel, o=o, width=width, m=m):
            def call():
                flip[0] ^= 1
                baseline(xs[flip[0]], kernel, o, width, m)
            return call

        legs.append((f"dense_{tag}_f32", dense(False), args.reps, {"bytes_per_call": B * (L * 4 + m * 4)}))
        legs.append((f"dense_{tag}_i16", dense(True), args.reps, {"bytes_per_call": B * (L * 2 + m * 4)}))
        legs.append((f"dense_{tag}_baseline", dense_base(), max(args.reps // 4, 2), {}))
        # ---- packed: clips of 1 .. 16 s ----
        lens = rng.integers(orig, 16 * orig + 1, B)
        so = np.zeros(B + 1, np.int64)
        np.cumsum(lens, out=so[1:])
        oo = np.empty_like(so)
        _lib.check(lib.ss_resample_packed_offsets(orig, new, B, so.ctypes.data, oo.ctypes.data))
        tin, tout = int(so[-1]), int(oo[-1])
        d_so, d_oo = torch.from_numpy(so).cuda(), torch.from_numpy(oo).cuda()
        pk = [torch.randn(tin, device="cuda").mul_(0.1) for _ in range(2)]
        pp = [(x * 32768.0).clamp_(-32768, 32767).to(torch.int16) for x in pk]
        pout = torch.empty(tout, device="cuda")
        Lmax = int(lens.max())
        padded = torch.zeros((B, Lmax), device="cuda")   # what the baseline needs: the clips as a zero-padded dense batch
        for b in range(0, B, max(B // 64, 1)):            # (a sample of the clips is enough for a timing: the rest stays zero)
            padded[b, :int(lens[b])] = pk[0][int(so[b]):int(so[b + 1])]

        def packed(pcm, pk=pk, pp=pp, rs=rs, d_so=d_so, d_oo=d_oo, tin=tin, tout=tout, pout=pout):
            def call():
                flip[0] ^= 1
                if pcm:
                    _lib.check(lib.ss_resample_packed_i16_device(rs.handle, pp[flip[0]].data_ptr(), B, d_so.data_ptr(), 2.0 ** -15, d_oo.data_ptr(),
                                                                 tin, tout, pout.data_ptr(), sp))
                else:
                    _lib.check(lib.ss_resample_packed_device(rs.handle, pk[flip[0]].data_ptr(), B, d_so.data_ptr(), d_oo.data_ptr(), tin, tout,
                                                             pout.data_ptr(), sp))
            return call

        def packed_base(padded=padded, kernel=kernel, o=o, width=width, rs=rs, Lmax=Lmax):
            def call():
                baseline(padded, kernel, o, width, rs.out_len(Lmax))
            return call

        legs.append((f"packed_{tag}_f32", packed(False), args.reps, {"bytes_per_call": tin * 4 + tout * 4, "seconds_of_audio": tin / orig}))
        legs.append((f"packed_{tag}_i16", packed(True), args.reps, {"bytes_per_call": tin * 2 + tout * 4}))
        legs.append((f"packed_{tag}_baseline", packed_base(), max(args.reps // 4, 2), {"padded_to_samples": Lmax}))
        # ---- pool: a ring of ticks ----
        P, N = args.pool, args.active
        n_state = C.c_size_t()
        _lib.check(lib.ss_resample_stream_state_len(rs.handle, C.byref(n_state)))
        rpool = torch.randn((P, n_state.value), device="cuda").mul_(0.1)
        rpool[:, -1] = rs.info.latency_periods   # steady state
        ticks = []
        for _ in range(args.ring):
            per = rng.integers(1, args.max_periods + 1, N)
            s = np.zeros(N + 1, np.int64)
            np.cumsum(per * o, out=s[1:])
            ticks.append({"n_in": int(s[-1]), "x": torch.randn(int(s[-1]), device="cuda").mul_(0.1), "so": torch.from_numpy(s).cuda(),
                          "slots": torch.from_numpy(rng.permutation(P)[:N].astype(np.int32)).cuda()})
        rout = torch.empty(N * args.max_periods * n, device="cuda")
        at = [0]

        def pool_call(ticks=ticks, rs=rs, rpool=rpool, rout=rout, P=P, N=N):
            def call():
                at[0] += 1
                t = ticks[at[0] % args.ring]
                _lib.check(lib.ss_resample_stream_packed_device(rs.handle, t["x"].data_ptr(), N, t["so"].data_ptr(), t["n_in"], t["slots"].data_ptr(),
                                                                P, rpool.data_ptr(), rout.data_ptr(), sp))
            return call

        mean_in = sum(t["n_in"] for t in ticks) / len(ticks)
        legs.append((f"pool_{tag}", pool_call(), 5 * args.reps,
                     {"bytes_per_call": int(mean_in * 4 + mean_in / o * n * 4 + 2 * N * n_state.value * 4), "state_len": n_state.value}))

    # ---- the MFCC pool call beside it ----
    cfg = ss.SpeechConfig(_lib.make_params())
    P, N = args.pool, args.active
    mticks = []
    for _ in range(args.ring):
        hops = rng.integers(1, 5, N)
        s = np.zeros(N + 1, np.int64)
        np.cumsum(hops * STEP, out=s[1:])
        mticks.append({"rows": int(hops.sum()), "x": torch.randn(int(s[-1]), device="cuda").mul_(0.1), "so": torch.from_numpy(s).cuda(),
                       "ro": torch.from_numpy(s // STEP).cuda(), "slots": torch.from_numpy(rng.permutation(P)[:N].astype(np.int32)).cuda()})
    fpool = torch.randn((P, STEP), device="cuda").mul_(0.1)
    fout = torch.empty((N * 4, 13), device="cuda")
    mat = [0]

    def mfcc_pool():
        mat[0] += 1
        t = mticks[mat[0] % args.ring]
        _lib.check(lib.ss_mfcc_stream_packed_device(cfg.handle, t["x"].data_ptr(), N, t["so"].data_ptr(), t["ro"].data_ptr(), t["rows"],
                                                    t["slots"].data_ptr(), P, 100, fpool.data_ptr(), fout.data_ptr(), sp))

    legs.append(("mfcc_pool", mfcc_pool, 5 * args.reps, {}))

    def timed(fn, reps, probe_us):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        if probe_us:
            _lib.check(lib.ss_shader_clock_probe_async(C.c_void_p(side.cuda_stream), int(probe_us), C.c_void_p(words.data_ptr())))
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        ghz = None
        if probe_us:
            cyc, ticks_ = words.tolist()
            ghz = cyc / (10.0 * ticks_) if ticks_ else None
        return a.elapsed_time(b) / reps * 1e3, ghz

    for _, fn, _, _ in legs:  # warm-up: code objects, the handles' tables, both input blocks
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    us = {name: [] for name, _, _, _ in legs}
    ghz = {name: [] for name, _, _, _ in legs}
    for r in range(args.rounds):
        for name, fn, reps, _ in legs:
            probe = 0
            if r > 0:  # sleep through about 80 % of what the leg took last round
                probe = min(max(0.8 * us[name][-1] * reps, 10.0), 1e6)
            t, g = timed(fn, reps, probe)
            us[name].append(t)
            if g:
                ghz[name].append(g)
    res = {"clips": B, "seconds": args.seconds, "pool": args.pool, "active": args.active, "max_periods": args.max_periods, "reps": args.reps,
           "rounds": args.rounds, "ring": args.ring, "device": torch.cuda.get_device_name(), "kernel_last": lib.ss_last_kernel_name().decode()}
    for name, _, reps, info in legs:
        v = us[name]
        leg = dict(info, us_per_call_median=statistics.median(v), us_min=min(v), us_max=max(v), reps=reps)
        if ghz[name]:
            leg["clock_ghz"] = statistics.median(ghz[name])
        if "bytes_per_call" in leg:
            leg["gb_per_s"] = leg["bytes_per_call"] / leg["us_per_call_median"] * 1e-3
            leg["hbm_fraction"] = leg["gb_per_s"] * 1e9 / HBM_PEAK
        res[name] = leg
    for name in list(us):
        base = name.rsplit("_", 1)[0] + "_baseline"
        if base in res and not name.endswith("_baseline"):
            res[name]["over_baseline"] = res[base]["us_per_call_median"] / res[name]["us_per_call_median"]
        if name.startswith("pool_"):
            res[name]["over_mfcc_pool"] = res[name]["us_per_call_median"] / res["mfcc_pool"]["us_per_call_median"]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
