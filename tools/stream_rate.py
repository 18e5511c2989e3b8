"""Rows/s and µs per call of the streaming mel spectrogram (ss_mel_spectrogram_stream_device) beside the one-shot call.

    python tools/stream_rate.py [--streams 1024] [--hops 16] [--reps 50]

Workloads, 16 kHz mel spectrogram at the cfg3 shape (2048 / 512, 128 filters) unless stated, measured with HIP events on one
stream after warm-up:
  continuous   n streams x `hops` hops per call, continuous mode (the rows and the state advance: two launches per call)
  oneshot      ss_mel_spectrogram_device on n clips that give the same real rows per clip (zeros(n_pad H) ++ chunk)
  live         n streams x 1 hop per call, continuous mode, captured once in a torch.cuda graph and replayed (µs per call)
  reference    as continuous, reference mode, at H = 600 (does not divide 2048): on the dedicated kernel's streaming build, and on
               the generic kernel's (the lab library's ss_debug_force_generic)
Prints one JSON line.  Measuring only: not collected by pytest, not part of bench.py.
"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mfcc-rust_amd"))

REF, CONT = 0, 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=1024)
    ap.add_argument("--hops", type=int, default=16)
    ap.add_argument("--reps", type=int, default=50)
    args = ap.parse_args()

    import torch

    import speechsauce_amd as ss
    from speechsauce_amd import _lib

    lib = _lib.lib()
    B = args.streams
    st = torch.cuda.current_stream()
    sp = C.c_void_p(st.cuda_stream)

    def setup(**kw):
        cfg = ss.SpeechConfig(_lib.make_params(sample_rate=16000, fft_points=2048, num_filters=128, high_frequency=8000.0, **kw))
        H = 2048 - _state_len(lib, cfg)
        return cfg, H

    def timed(fn, reps):
        fn()
        torch.cuda.synchronize()
        kernel = lib.ss_last_kernel_name().decode()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / reps * 1e-3, kernel

    res = {"streams": B, "hops": args.hops, "device": torch.cuda.get_device_name()}

    # (a) continuous, and the one-shot call on the same real rows
    cfg, H = setup(frame_length=0.032)
    S = 2048 - H
    n_pad = 2048 // H - 1
    x = torch.randn((B, args.hops * H), device="cuda").mul_(0.1)
    state = torch.zeros((B, S), device="cuda")
    out = torch.empty((B, 128, args.hops), device="cuda")

    def cont():
        _lib.check(lib.ss_mel_spectrogram_stream_device(cfg.handle, CONT, x.data_ptr(), B, args.hops * H, args.hops * H,
                                                          state.data_ptr(), out.data_ptr(), sp))

    t, k = timed(cont, args.reps)
    rows = B * args.hops
    res["continuous"] = {"rows": rows, "s_per_call": t, "rows_per_s": rows / t, "kernel": k}
    L = (args.hops + n_pad) * H
    xo = torch.randn((B, L), device="cuda").mul_(0.1)
    outo = torch.empty((B, 128, args.hops + n_pad), device="cuda")

    def oneshot():
        _lib.check(lib.ss_mel_spectrogram_device(cfg.handle, xo.data_ptr(), B, L, L, outo.data_ptr(), sp))

    t, k = timed(oneshot, args.reps)
    res["oneshot"] = {"rows": rows, "s_per_call": t, "rows_per_s": rows / t, "kernel": k}
    res["continuous_over_oneshot"] = res["continuous"]["rows_per_s"] / res["oneshot"]["rows_per_s"]

    # (b) one hop per call, graph-replayed
    x1 = torch.randn((B, H), device="cuda").mul_(0.1)
    out1 = torch.empty((B, 128, 1), device="cuda")

    def live():
        _lib.check(lib.ss_mel_spectrogram_stream_device(cfg.handle, CONT, x1.data_ptr(), B, H, H, state.data_ptr(), out1.data_ptr(),
                                                          C.c_void_p(torch.cuda.current_stream().cuda_stream)))

    side = torch.cuda.Stream()
    side.wait_stream(st)
    with torch.cuda.stream(side):
        live()
    st.wait_stream(side)
    torch.cuda.synchronize()
    kernel = lib.ss_last_kernel_name().decode()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        live()
    t, _ = timed(g.replay, args.reps * 4)
    res["live_graph"] = {"rows": B, "us_per_call": t * 1e6, "rows_per_s": B / t, "kernel": kernel}
    eager_t, _ = timed(live, args.reps * 4)
    res["live_eager"] = {"rows": B, "us_per_call": eager_t * 1e6, "kernel": kernel}

    # (c) reference mode at H = 600: the dedicated streaming build, then the generic one
    cfg6, H6 = setup(frame_length=600 / 16000)
    S6 = 2048 - H6
    n6 = args.hops * H6
    x6 = torch.randn((B, n6), device="cuda").mul_(0.1)
    state6 = torch.zeros((B, S6), device="cuda")
    r, rr = C.c_size_t(), C.c_size_t()
    _lib.check(lib.ss_stream_rows(C.byref(cfg6.params), REF, n6, C.byref(r), C.byref(rr)))
    out6 = torch.empty((B, 128, r.value), device="cuda")

    def ref():
        _lib.check(lib.ss_mel_spectrogram_stream_device(cfg6.handle, REF, x6.data_ptr(), B, n6, n6, state6.data_ptr(), out6.data_ptr(), sp))

    t, k = timed(ref, args.reps)
    res["reference_h600"] = {"rows": B * r.value, "real_rows": B * rr.value, "s_per_call": t, "rows_per_s": B * r.value / t, "kernel": k}
    cfg.device_status()
    lab = _lib.lab()
    with _lib.use_library(lab):
        cfg6g = ss.SpeechConfig(_lib.make_params(sample_rate=16000, fft_points=2048, num_filters=128, high_frequency=8000.0,
                                                 frame_length=600 / 16000))
        state6.zero_()

        def ref_generic():
            _lib.check(lab.ss_mel_spectrogram_stream_device(cfg6g.handle, REF, x6.data_ptr(), B, n6, n6, state6.data_ptr(),
                                                            out6.data_ptr(), sp))

        try:
            lab.ss_debug_force_generic(1)
            t, _ = timed(ref_generic, max(1, args.reps // 5))
            k = lab.ss_last_kernel_name().decode()
        finally:
            lab.ss_debug_force_generic(0)
    res["reference_h600_generic"] = {"rows": B * r.value, "s_per_call": t, "rows_per_s": B * r.value / t, "kernel": k}
    print(json.dumps(res))


def _state_len(lib, cfg):
    from speechsauce_amd import _lib

    S = C.c_size_t()
    _lib.check(lib.ss_stream_state_len(C.byref(cfg.params), C.byref(S)))
    return S.value


if __name__ == "__main__":
    main()
