#!/usr/bin/env python3
"""Which kernel serves which call: one tiny call per (configuration, entry point, sample type) through the device-pointer C ABI,
and what ss_last_kernel_name() reports afterwards.  Prints one JSON object {configuration: {case: kernel name}}; a call the API
rejects is recorded as {"status": code, "error": message} instead of a name.

usage: tools/selection_census.py [out.json]      (SS_LIB_PATH=<another build's libspeechsauce_amd.so> runs the census on that build)

tests/test_kernel_selection.py reruns census() and compares it case by case with tests/golden/kernel_selection.json, which is this
tool's output on an MI355X (256 CUs) before the launchers of ss_api.hip were folded onto shared argument builders: the selection
ladders of launch_frames / launch_stft and their streaming / packed / pool forms must keep picking the same kernels.

Shapes: two rows (STFT path) or four frames (MFCC path: the batch-table builds of the *_batches_device calls need four) per clip and
two or three clips -- selection does not depend on more.  The one exception is the 2048-point mel kernel's choice between its eight- and twelve-wave build (launch_mel_c1024, ss_mel2048.hip: twelve_waves_win), which
goes by the work units per CU: units = channels * ceil(rows / 2), per_cu = ceil(units / CUs), twelve waves where
1.29 * ceil(per_cu / 12) < ceil(per_cu / 8) -- first true at per_cu = 9, i.e. at 8 * CUs + 1 units.  With two rows per channel a
unit is a channel, so the census calls the 2048-point configuration with 8 * CUs channels (eight waves) and 8 * CUs + 1 (twelve).
"""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mfcc-rust_amd"))

PCM_SCALE = 2.0 ** -15
CONTINUOUS = 1  # SS_STREAM_CONTINUOUS
REFERENCE = 0   # SS_STREAM_REFERENCE

# name -> make_params switches (16 kHz, 20 ms frames at a 10 ms stride, 40 filters, 13 cepstra unless said otherwise).  The STFT
# path needs fft_points >= 2 * frame_size, so the 512-point mel kernel gets a configuration with 10 ms frames of its own; the
# 4096-point kernels serve long frames (MFCC: the 44.1 kHz shape with 4096-sample frames; mel: 1024-sample chunks).
CONFIGS = {
    "fft256": dict(fft_points=256, frame_length=0.01, frame_stride=0.005),
    "fft512": dict(fft_points=512),
    "fft1024": dict(fft_points=1024),
    "fft2048": dict(fft_points=2048),
    "fft4096": dict(sample_rate=44100, fft_points=4096, frame_length=4096 / 44100, frame_stride=1024 / 44100, num_cepstral=40,
                    num_filters=256, high_frequency=22050.0),
    "chirpz400": dict(fft_points=400, frame_length=0.01, frame_stride=0.005),
    "fft512_wide64": dict(fft_points=512, num_filters=64),
    "fft512_window": dict(fft_points=512, mfcc_window="hann"),
    "fft512_preemph": dict(fft_points=512, preemph_coef=0.97),
    "fft512_center_reflect": dict(fft_points=512, framing="center", pad_mode="reflect"),
    "fft512_center_constant": dict(fft_points=512, framing="center", pad_mode="constant"),
    "fft512_fullp": dict(fft_points=512, mel_scale="slaney"),
    "fft512_ortho": dict(fft_points=512, dct_norm="ortho"),
    "fft512_stft": dict(fft_points=512, frame_length=0.01, frame_stride=0.005),
    "fft512_stft_fullp": dict(fft_points=512, frame_length=0.01, frame_stride=0.005, mel_scale="slaney"),
    "fft2048_fullp": dict(fft_points=2048, mel_scale="slaney"),
    "fft2048_bank6321": dict(fft_points=2048, frame_length=0.032, frame_stride=0.032, num_filters=128, high_frequency=8000.0),
    "fft4096_stft": dict(sample_rate=44100, fft_points=4096, frame_length=1024 / 44100, frame_stride=1024 / 44100, num_filters=128),
}


def census(lib) -> dict:
    """Run every case on `lib` (a loaded libspeechsauce_amd.so with its prototypes set: speechsauce_amd._lib.load / lib)."""
    import torch

    from speechsauce_amd import _lib

    assert torch.cuda.is_available(), "the census launches kernels: it needs a HIP device"
    dev = torch.device("cuda:0")
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    stream = torch.cuda.current_stream().cuda_stream
    g = torch.Generator(device="cpu").manual_seed(0)
    n_x = 5 << 20  # samples: the largest call is 2 blocks of 8 * CUs + 1 channels of 2 hops of 512 samples
    xf = (torch.rand(n_x, generator=g) * 0.2 - 0.1).to(dev)
    xi = (xf * 32768.0).to(torch.int16)
    out0 = torch.zeros(9 << 20, device=dev)  # the largest output: stft of 8 * CUs + 1 channels, 2 rows of 1025 bins
    out1 = torch.zeros(1 << 16, device=dev)
    state = torch.zeros(1 << 16, device=dev)

    def result(rc):
        torch.cuda.synchronize()
        if rc == _lib.SS_OK:
            return lib.ss_last_kernel_name().decode()
        return {"status": rc, "error": lib.ss_last_error_string().decode()}

    def sizes(fn, p, *args, n_out=1):
        """a host-only size helper of the ABI: its outputs, or the error record"""
        outs = [C.c_size_t(0) for _ in range(n_out)]
        rc = fn(C.byref(p), *args, *[C.byref(o) for o in outs])
        return rc, [o.value for o in outs]

    def offsets(fn, p, so):
        ro = np.zeros(len(so), dtype=np.int64)
        rc = fn(C.byref(p), len(so) - 1, so.ctypes.data, ro.ctypes.data)
        return rc, ro

    def dev_i64(a):
        return torch.from_numpy(a).to(dev)

    def run_config(p):
        cases = {}
        cfg = C.c_void_p()
        rc = lib.ss_config_create(C.byref(p), C.byref(cfg))
        if rc != _lib.SS_OK:
            return {"ss_config_create": result(rc)}
        try:
            run_mfcc_path(p, cfg, cases)
            run_stft_path(p, cfg, cases)
            rc = lib.ss_config_device_status(cfg)
            cases["device_status"] = "ok" if rc == _lib.SS_OK else result(rc)
        finally:
            torch.cuda.synchronize()
            lib.ss_config_destroy(cfg)
        return cases

    def checked(key, n_floats0, n_floats1=0, n_state=0):
        """the census never launches over a buffer it did not size: a case that would not fit is a bug of this tool"""
        assert n_floats0 <= out0.numel() and n_floats1 <= out1.numel() and n_state <= state.numel(), key

    # ---- MFCC path: mfcc / mfe / power spectrum; dense, packed, dense stream, pool; batches -----------------------------------------
    def run_mfcc_path(p, cfg, cases):
        rc, (flen, step) = sizes(lib.ss_frame_sizes, p, n_out=2)
        if rc != _lib.SS_OK:
            cases["ss_frame_sizes"] = result(rc)
            return
        B, n = 3, flen + 4 * step
        rc, (T,) = sizes(lib.ss_num_frames, p, n)
        if rc != _lib.SS_OK:
            cases["ss_num_frames"] = result(rc)
            return
        F, M, ceps = p.fft_points // 2 + 1, p.num_filters, p.num_cepstral
        checked("dense", B * T * max(F, M, ceps), B * T)
        assert 9 * B * n <= n_x
        X, XI, O0, O1 = xf.data_ptr(), xi.data_ptr(), out0.data_ptr(), out1.data_ptr()
        cases["mfcc_batch"] = result(lib.ss_mfcc_batch_device(cfg, X, B, n, n, O0, stream))
        cases["mfcc_batch_i16"] = result(lib.ss_mfcc_batch_i16_device(cfg, XI, B, n, n, PCM_SCALE, O0, stream))
        cases["mfe_batch"] = result(lib.ss_mfe_batch_device(cfg, X, B, n, n, O0, O1, stream))
        cases["mfe_batch_i16"] = result(lib.ss_mfe_batch_i16_device(cfg, XI, B, n, n, PCM_SCALE, O0, O1, stream))
        cases["power_spectrum_batch"] = result(lib.ss_power_spectrum_batch_device(cfg, X, B, n, n, O0, stream))
        # a frames matrix (power_spectrum(frames, fft_points)): three rows, each one frame of flen samples
        cases["power_spectrum_frames"] = result(lib.ss_power_spectrum_frames_device(cfg, X, B, flen, flen, O0, stream))
        # the batches call: 2 batches (one group) and 9 (a full group of eight and a single; the name is the last launch's)
        for nb in (2, 9):
            checked("batches", nb * B * T * ceps)
            xs = (C.c_void_p * nb)(*[X + 4 * b * B * n for b in range(nb)])
            outs = (C.c_void_p * nb)(*[O0 + 4 * b * B * T * ceps for b in range(nb)])
            counts = (C.c_size_t * nb)(*[B] * nb)
            cases[f"mfcc_batches_{nb}"] = result(lib.ss_mfcc_batches_device(cfg, nb, xs, counts, n, n, outs, stream))
        # packed clips of three lengths
        so = np.cumsum([0, n, n + step, n + 3 * step]).astype(np.int64)
        rc, fo = offsets(lib.ss_packed_frame_offsets, p, so)
        if rc != _lib.SS_OK:
            cases["ss_packed_frame_offsets"] = result(rc)
        else:
            rows, dso, dfo = int(fo[-1]), dev_i64(so), dev_i64(fo)
            checked("packed", rows * max(M, ceps), rows)
            a = (3, dso.data_ptr())
            cases["mfcc_packed"] = result(lib.ss_mfcc_packed_device(cfg, X, *a, dfo.data_ptr(), rows, O0, stream))
            cases["mfcc_packed_i16"] = result(lib.ss_mfcc_packed_i16_device(cfg, XI, *a, PCM_SCALE, dfo.data_ptr(), rows, O0, stream))
            cases["mfe_packed"] = result(lib.ss_mfe_packed_device(cfg, X, *a, dfo.data_ptr(), rows, O0, O1, stream))
            cases["mfe_packed_i16"] = result(lib.ss_mfe_packed_i16_device(cfg, XI, *a, PCM_SCALE, dfo.data_ptr(), rows, O0, O1, stream))
        # dense streams: three streams, two hops per call
        rc, (S,) = sizes(lib.ss_frame_stream_state_len, p)
        if rc != _lib.SS_OK:
            cases["ss_frame_stream_state_len"] = result(rc)
            return
        ns = 2 * step
        checked("stream", B * 2 * max(M, ceps), B * 2, 3 * S)
        ST = state.data_ptr()
        cases["mfcc_stream"] = result(lib.ss_mfcc_stream_device(cfg, X, B, ns, ns, 98, ST, O0, stream))
        cases["mfe_stream"] = result(lib.ss_mfe_stream_device(cfg, X, B, ns, ns, ST, O0, O1, stream))
        # the pool: two entries (two hops, one hop) on rows 2 and 0 of a pool of three
        so = np.cumsum([0, 2 * step, step]).astype(np.int64)
        rc, ro = offsets(lib.ss_frame_stream_packed_row_offsets, p, so)
        if rc != _lib.SS_OK:
            cases["ss_frame_stream_packed_row_offsets"] = result(rc)
            return
        rows, dso, dro = int(ro[-1]), dev_i64(so), dev_i64(ro)
        slots = torch.tensor([2, 0], dtype=torch.int32, device=dev)
        checked("pool", rows * max(M, ceps), rows, 3 * S)
        a = (2, dso.data_ptr(), dro.data_ptr(), rows, slots.data_ptr(), 3)
        cases["mfcc_stream_packed"] = result(lib.ss_mfcc_stream_packed_device(cfg, X, *a, 98, ST, O0, stream))
        cases["mfcc_stream_packed_i16"] = result(lib.ss_mfcc_stream_packed_i16_device(cfg, XI, *a, PCM_SCALE, 98, ST, O0, stream))
        cases["mfe_stream_packed"] = result(lib.ss_mfe_stream_packed_device(cfg, X, *a, ST, O0, O1, stream))
        cases["mfe_stream_packed_i16"] = result(lib.ss_mfe_stream_packed_i16_device(cfg, XI, *a, PCM_SCALE, ST, O0, O1, stream))

    # ---- STFT path: mel spectrogram / stft; dense, packed, dense stream, pool; batches ---------------------------------------------
    def run_stft_path(p, cfg, cases):
        hop, n_pad, wnorm = C.c_size_t(0), C.c_size_t(0), C.c_float(0)
        rc = lib.ss_stft_sizes(C.byref(p), C.byref(hop), C.byref(n_pad), C.byref(wnorm))
        if rc != _lib.SS_OK:
            cases["ss_stft_sizes"] = result(rc)
            return
        hop = hop.value
        B, n = 3, 2 * hop
        rc, (R, _) = sizes(lib.ss_stft_rows, p, n, n_out=2)
        if rc != _lib.SS_OK:
            cases["ss_stft_rows"] = result(rc)
            return
        F, M = p.fft_points // 2 + 1, p.num_filters
        per_row = max(2 * F, M)
        X, XI, O0, ST = xf.data_ptr(), xi.data_ptr(), out0.data_ptr(), state.data_ptr()

        def dense(tag, chans):
            checked("dense" + tag, chans * R * per_row)
            assert chans * n <= n_x
            cases["mel" + tag] = result(lib.ss_mel_spectrogram_device(cfg, X, chans, n, n, O0, stream))
            cases["mel_i16" + tag] = result(lib.ss_mel_spectrogram_i16_device(cfg, XI, chans, n, n, PCM_SCALE, O0, stream))
            cases["stft" + tag] = result(lib.ss_stft_device(cfg, X, chans, n, n, O0, stream))
            cases["stft_i16" + tag] = result(lib.ss_stft_i16_device(cfg, XI, chans, n, n, PCM_SCALE, O0, stream))

        def batches(tag, nb, chans):
            checked("batches" + tag, nb * chans * R * M)
            assert nb * chans * n <= n_x
            xs = (C.c_void_p * nb)(*[X + 4 * b * chans * n for b in range(nb)])
            outs = (C.c_void_p * nb)(*[O0 + 4 * b * chans * R * M for b in range(nb)])
            counts = (C.c_size_t * nb)(*[chans] * nb)
            cases[f"mel_batches_{nb}{tag}"] = result(lib.ss_mel_spectrogram_batches_device(cfg, nb, xs, counts, n, n, outs, stream))

        dense("", B)
        batches("", 2, B)
        batches("", 9, B)
        if p.fft_points == 2048:  # both sides of the eight / twelve-wave rule (see the module docstring): R = 2, a unit is a channel
            assert R == 2
            dense("@8cu", 8 * cus)
            dense("@8cu+1", 8 * cus + 1)
            batches("@8cu+1", 2, 8 * cus + 1)  # blocks that select the twelve-wave build on their own share one launch
        # packed clips of two lengths
        so = np.cumsum([0, 2 * hop, 3 * hop]).astype(np.int64)
        rc, ro = offsets(lib.ss_packed_row_offsets, p, so)
        if rc != _lib.SS_OK:
            cases["ss_packed_row_offsets"] = result(rc)
        else:
            rows, dso, dro = int(ro[-1]), dev_i64(so), dev_i64(ro)
            checked("packed", rows * per_row)
            a = (2, dso.data_ptr())
            cases["mel_packed"] = result(lib.ss_mel_spectrogram_packed_device(cfg, X, *a, dro.data_ptr(), rows, O0, stream))
            cases["mel_packed_i16"] = result(lib.ss_mel_spectrogram_packed_i16_device(cfg, XI, *a, PCM_SCALE, dro.data_ptr(), rows, O0, stream))
            cases["stft_packed"] = result(lib.ss_stft_packed_device(cfg, X, *a, dro.data_ptr(), rows, O0, stream))
            cases["stft_packed_i16"] = result(lib.ss_stft_packed_i16_device(cfg, XI, *a, PCM_SCALE, dro.data_ptr(), rows, O0, stream))
        # dense streams: three streams, two hops per call, both modes
        rc, (S,) = sizes(lib.ss_stream_state_len, p)
        if rc != _lib.SS_OK:
            cases["ss_stream_state_len"] = result(rc)
            return
        for mode, tag in ((CONTINUOUS, "continuous"), (REFERENCE, "reference")):
            rc, (Rs, _) = sizes(lib.ss_stream_rows, p, mode, n, n_out=2)
            if rc != _lib.SS_OK:
                cases["ss_stream_rows_" + tag] = result(rc)
                continue
            checked("stream", B * Rs * per_row, 0, B * S)
            cases["mel_stream_" + tag] = result(lib.ss_mel_spectrogram_stream_device(cfg, mode, X, B, n, n, ST, O0, stream))
            cases["stft_stream_" + tag] = result(lib.ss_stft_stream_device(cfg, mode, X, B, n, n, ST, O0, stream))
        # the pool: two entries (two hops, one hop) on rows 2 and 0 of a pool of three
        so = np.cumsum([0, 2 * hop, hop]).astype(np.int64)
        rc, ro = offsets(lib.ss_stream_packed_row_offsets, p, so)
        if rc != _lib.SS_OK:
            cases["ss_stream_packed_row_offsets"] = result(rc)
            return
        rows, dso, dro = int(ro[-1]), dev_i64(so), dev_i64(ro)
        slots = torch.tensor([2, 0], dtype=torch.int32, device=dev)
        checked("pool", rows * per_row, 0, 3 * S)
        a = (2, dso.data_ptr(), dro.data_ptr(), rows, slots.data_ptr(), 3)
        cases["mel_stream_packed"] = result(lib.ss_mel_spectrogram_stream_packed_device(cfg, X, *a, ST, O0, stream))
        cases["mel_stream_packed_i16"] = result(lib.ss_mel_spectrogram_stream_packed_i16_device(cfg, XI, *a, PCM_SCALE, ST, O0, stream))
        cases["stft_stream_packed"] = result(lib.ss_stft_stream_packed_device(cfg, X, *a, ST, O0, stream))
        cases["stft_stream_packed_i16"] = result(lib.ss_stft_stream_packed_i16_device(cfg, XI, *a, PCM_SCALE, ST, O0, stream))

    return {name: run_config(_lib.make_params(**kw)) for name, kw in CONFIGS.items()}


def main() -> int:
    from speechsauce_amd import _lib

    text = json.dumps(census(_lib.lib()), indent=1, sort_keys=True)
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as f:
            f.write(text + "\n")
    print(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
