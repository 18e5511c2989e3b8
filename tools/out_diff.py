#!/usr/bin/env python3
"""Compare the OUTPUT BYTES of two builds of libspeechsauce_amd.so on a fixed list of small calls: the output-side sibling of
tools/isa_diff.py, for a change that must not move a bit (a refactor of the quad kernels of ss_quad256.h or of the frame stages of
ss_frame32.h).

usage: python tools/out_diff.py BEFORE_LIB AFTER_LIB      (needs a GPU)

Each library runs the whole list in a fresh child process of its own (started with subprocess, SS_LIB_PATH set to it: no process
ever loads both), which writes every case's raw outputs and the name of the kernel that served it to a temporary directory.  The
parent then compares the files byte for byte and prints one line per case: `same` / `DIFFERENT`, the kernel, the byte count.  A
case whose kernel is not the one it is listed under counts as different.  If the first child fails, the second is not started.
Exit status 1 if any case differs.  The cases are at most a few hundred frames each:
  ss_mfcc_c256w    80 filters; frame lengths 320 / 400 / 512 x magnitude / power x mfcc / mfe x window off / on (all 24 builds) on a
                   batch of 3 clips of 99 / 98 / 97 frames (297 / 294 / 291: never a multiple of 4; the reciprocal path); 20
                   cepstra; 5 clips of 3 frames (the dividing path); centred framing with reflect and with zero padding; fused
                   pre-emphasis
  ss_kaldi_c256    frame lengths 257 / 400 / 512 x fbank / MFCC x power / magnitude, dense; packed clips of 1..7 frames with an
                   entry shorter than a frame among them; an odd frame shift (the single-float load path)
  ss_mel_c256      mel with the bank inside bin 128 and past it (fullp), stft, an odd hop, a clip shorter than one window
  ss_mfcc_c256x2   frame lengths 160 / 200 x 13 / 20 cepstra on 3 clips of 198 / 197 frames (594 / 591, not a multiple of 8), mfe, a
                   clip with a silent second half (the two-pass guard), a pure tone on a bin centre and a full-scale square wave
                   (the tiny-bin rerun)
  ss_mfcc_c512     22050 Hz, fft 1024, frame length 883, hop 221, on 3 clips of 7 frames (21 frames = 11 pairs: a pair straddles each
                   clip boundary, the last one is half dead; the clip length comes from SpeechConfig.num_frames): magnitude / power x
                   mfcc / mfe x rect / hann x contract / centred (all 16 builds) and the same eight with fused pre-emphasis 0.97;
                   centred frames with reflect and with constant padding, with and without pre-emphasis; a Slaney bank past bin
                   fft_points / 4 (fullp); frame length 1024 (no zero tail); 41 and 127 filters; 33 and 64 cepstra; one clip of one frame
  ss_mfcc_c1024    44100 Hz, fft 2048, frame length 1765, hop 441: the same list, over all 24 builds (the `pre` ones included)
  ss_mel_c512      fft 1024, 16 kHz, hop 512: a bank to Nyquist and one held below bin 256, stft, an odd hop (441) at an odd clip
                   length, a clip shorter than one window, an odd row count (the clip's last pair half dead)
  ss_mel_c2048     fft 4096, 44.1 kHz, hop 1024: the same without the odd row count (one row per wave); odd hop 1103
A measuring tool: not collected by pytest.
"""
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_TIMEOUT_S = 300


def cases(ss, np, torch):
    """-> [(name, expected kernel prefix, thunk -> tensor or tuple of tensors)]"""
    from speechsauce_amd import _lib

    rng = np.random.default_rng(20240)

    def noise(*shape):
        return torch.from_numpy((0.1 * rng.standard_normal(shape)).astype(np.float32)).cuda()

    out = []

    def front(kernel, name, fn, sig, **params):
        cfg = ss.SpeechConfig(_lib.make_params(**params))
        out.append((name, kernel, lambda: fn(sig, cfg)))

    # ---- ss_mfcc_c256w ----
    x98 = noise(3, 16160)  # 99 / 98 / 97 frames per clip at frame lengths 320 / 400 / 512
    for flen in (320, 400, 512):
        for exp in (1, 2):
            for fn, what in ((ss._internal_mfcc_batch, "mfcc"), (ss._internal_mfe_batch, "mfe")):
                for win in ("rect", "hann"):
                    front("ss_mfcc_c256w", f"c256w {what} flen{flen} exp{exp} {win}", fn, x98, frame_length=flen / 16000, num_filters=80,
                          spectrum_exponent=exp, mfcc_window=win)
    w = dict(frame_length=0.025, num_filters=80)
    for exp in (1, 2):
        front("ss_mfcc_c256w", f"c256w mfcc 20 cepstra exp{exp}", ss._internal_mfcc_batch, x98, num_cepstral=20, spectrum_exponent=exp, **w)
    x3 = noise(5, 400 + 3 * 160)  # 3 frames per clip: no reciprocal below 4
    front("ss_mfcc_c256w", "c256w mfcc 5 clips x 3 frames", ss._internal_mfcc_batch, x3, **w)
    front("ss_mfcc_c256w", "c256w mfe 5 clips x 3 frames", ss._internal_mfe_batch, x3, **w)
    for pad in ("reflect", "constant"):
        front("ss_mfcc_c256w", f"c256w mfcc centred {pad}", ss._internal_mfcc_batch, x98, framing="center", pad_mode=pad, mfcc_window="hann", **w)
    front("ss_mfcc_c256w", "c256w mfcc pre-emphasis", ss._internal_mfcc_batch, x98, preemph_coef=0.97, **w)
    front("ss_mfcc_c256w", "c256w mfe pre-emphasis hann", ss._internal_mfe_batch, x98, preemph_coef=0.97, mfcc_window="hann", **w)

    # ---- ss_kaldi_c256 ----
    def kaldi_cfg(flen, shift, mfcc, power):
        key = (16000.0, flen / 16.0, shift / 16.0, 23 if mfcc else 80, 13 if mfcc else 0, 20.0, 0.0, 0.97, 22.0 if mfcc else 0.0, "povey", 0.42,
               True, power, False, True, 1.0, 1.0)
        return ss._get_kaldi_config(key, 0)

    xk = 0.3 * noise(3, 16000)
    for flen in (257, 400, 512):
        for mfcc in (False, True):
            for power in (True, False):
                name = f"kaldi {'mfcc' if mfcc else 'fbank'} flen{flen} {'power' if power else 'magnitude'}"
                out.append((name, "ss_kaldi_c256", lambda c=kaldi_cfg(flen, 160, mfcc, power), m=mfcc: ss._kaldi_dense(xk, c, m, not m)))
    out.append(("kaldi fbank odd shift 161", "ss_kaldi_c256", lambda c=kaldi_cfg(400, 161, False, True): ss._kaldi_dense(xk, c, False, True)))
    out.append(("kaldi mfcc odd shift 161", "ss_kaldi_c256", lambda c=kaldi_cfg(400, 161, True, True): ss._kaldi_dense(xk, c, True, False)))

    def kaldi_packed(cfg, x, so, fo, mfcc):
        # the C entry point itself: the Python front refuses an entry shorter than a frame.  The kernel skips it (no row) and raises
        # the handle's error word, which is read and dropped here; every row belongs to a valid clip and is written
        lib, stream = _lib.lib(), C.c_void_p(torch.cuda.current_stream().cuda_stream)
        n, rows = so.size - 1, int(fo[-1])
        dso, dfo = torch.from_numpy(so).cuda(), torch.from_numpy(fo).cuda()
        res = torch.full((rows, 13 if mfcc else 80), -1.0, device="cuda")
        en = torch.full((rows,), -1.0, device="cuda")
        if mfcc:
            _lib.check(lib.ss_kaldi_mfcc_packed_device(cfg.handle, x.data_ptr(), n, dso.data_ptr(), dfo.data_ptr(), rows, res.data_ptr(), stream))
        else:
            _lib.check(lib.ss_kaldi_fbank_packed_device(cfg.handle, x.data_ptr(), n, dso.data_ptr(), dfo.data_ptr(), rows, res.data_ptr(), en.data_ptr(), stream))
        torch.cuda.synchronize()
        try:
            cfg.device_status()
        except _lib.SpeechSauceError:
            pass
        return res, en

    for shift in (160, 161):
        Ts = [1, 2, 3, 4, 0, 5, 6, 7]
        extra = [0, 3, 0, 1, 0, 0, 7, 2]
        lens = [400 + (t - 1) * shift + e if t else 120 for t, e in zip(Ts, extra)]
        so = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        fo = np.concatenate([[0], np.cumsum(Ts)]).astype(np.int64)
        xp = 0.3 * noise(int(so[-1]))
        for mfcc in (False, True):
            name = f"kaldi {'mfcc' if mfcc else 'fbank'} packed 1..7 frames and an empty entry, shift {shift}"
            out.append((name, "ss_kaldi_c256", lambda c=kaldi_cfg(400, shift, mfcc, True), m=mfcc, x=xp, s=so, o=fo: kaldi_packed(c, x, s, o, m)))

    # ---- ss_mel_c256 ----
    xm = noise(3, 16000)
    m = dict(fft_points=512, frame_length=0.016, frame_stride=0.016, num_filters=40)
    mel = ss._internal_mel_spectrogram
    front("ss_mel_c256", "mel bank to 8 kHz (fullp)", mel, xm, **m)
    front("ss_mel_c256", "mel bank to 3.9 kHz", mel, xm, high_frequency=3900.0, **m)
    front("ss_mel_c256", "mel 80 filters", mel, xm, **dict(m, num_filters=80))
    front("ss_mel_c256", "mel odd hop", mel, noise(3, 15000), sample_rate=15000, **dict(m, frame_length=0.01502, frame_stride=0.01502))
    front("ss_mel_c256", "mel clip shorter than a window", mel, noise(2, 300), **m)
    out.append(("stft", "ss_mel_c256<stft>", lambda: torch.view_as_real(ss.stft(xm, 16000, frame_length=0.016, fft_length=512))))
    out.append(("stft odd hop", "ss_mel_c256<stft>", lambda x=noise(2, 15000): torch.view_as_real(ss.stft(x, 15000, frame_length=0.01502, fft_length=512))))
    out.append(("stft clip shorter than a window", "ss_mel_c256<stft>", lambda x=noise(300): torch.view_as_real(ss.stft(x, 16000, frame_length=0.016, fft_length=512))))

    # ---- ss_mfcc_c256x2 ----
    x8 = noise(3, 16000)
    t8 = dict(sample_rate=8000, fft_points=256, num_filters=40)
    for flen in (160, 200):
        for ceps in (13, 20):
            front("ss_mfcc_c256x2", f"c256x2 mfcc flen{flen} {ceps} cepstra", ss._internal_mfcc_batch, x8, frame_length=flen / 8000, num_cepstral=ceps, **t8)
        front("ss_mfcc_c256x2", f"c256x2 mfe flen{flen} power hann", ss._internal_mfe_batch, x8, frame_length=flen / 8000, spectrum_exponent=2,
              mfcc_window="hann", **t8)
    half = x8.clone()
    half[:, 8000:] = 0.0
    front("ss_mfcc_c256x2", "c256x2 mfcc silent second half", ss._internal_mfcc_batch, half, **t8)
    front("ss_mfcc_c256x2", "c256x2 mfe silent second half", ss._internal_mfe_batch, half, **t8)
    n = np.arange(8000)
    tone = torch.from_numpy(np.stack([0.5 * np.sin(2 * np.pi * 1000.0 * n / 8000.0), 0.25 * np.cos(2 * np.pi * 500.0 * n / 8000.0)]).astype(np.float32)).cuda()
    square = torch.from_numpy(np.stack([np.where((n // 4) % 2 == 0, 1.0, -1.0), np.where((n // 8) % 2 == 0, 1.0, -1.0)]).astype(np.float32)).cuda()
    for sig, what in ((tone, "tone on a bin centre"), (square, "full-scale square wave")):
        front("ss_mfcc_c256x2", f"c256x2 mfcc {what}, 256-sample frames", ss._internal_mfcc_batch, sig, frame_length=0.032, **t8)
        front("ss_mfcc_c256x2", f"c256x2 mfe {what}, 256-sample frames", ss._internal_mfe_batch, sig, frame_length=0.032, spectrum_exponent=2, **t8)

    # ---- ss_mfcc_c512 / ss_mfcc_c1024: two frames per wave ----
    def clip_len(frames, **params):
        """shortest clip that num_frames gives `frames` frames"""
        cfg = ss.SpeechConfig(_lib.make_params(**params))

        def count(n):
            try:
                return cfg.num_frames(n)
            except _lib.SpeechSauceError:  # shorter than one frame
                return 0

        return next(n for n in range(1, 1 << 20) if count(n) == frames)

    mfcc, mfe = (ss._internal_mfcc_batch, "mfcc"), (ss._internal_mfe_batch, "mfe")
    for kernel, tag, sr, nfft, flen, hop, M in (("ss_mfcc_c512", "c512", 22050, 1024, 883, 221, 64), ("ss_mfcc_c1024", "c1024", 44100, 2048, 1765, 441, 128)):
        b = dict(sample_rate=sr, fft_points=nfft, frame_length=flen / sr, frame_stride=hop / sr, num_filters=M, num_cepstral=20)
        centred = dict(framing="center", pad_mode="reflect")
        # 3 clips of 7 frames = 21 frames = 11 pairs: a pair straddles each clip boundary, the last one is half dead
        x7, x7c = noise(3, clip_len(7, **b)), noise(3, clip_len(7, **b, **centred))
        for pre in (0.0, 0.97):  # (ss_mfcc_c1024 has builds of its own for fused pre-emphasis)
            for exp in (1, 2):
                for fn, what in (mfcc, mfe):
                    for win in ("rect", "hann"):
                        sw = dict(spectrum_exponent=exp, mfcc_window=win, preemph_coef=pre)
                        front(kernel, f"{tag} {what} exp{exp} {win} pre{pre} contract", fn, x7, **b, **sw)
                        if pre == 0.0:
                            front(kernel, f"{tag} {what} exp{exp} {win} centred reflect", fn, x7c, **b, **sw, **centred)
        front(kernel, f"{tag} mfcc hann centred constant", mfcc[0], x7c, mfcc_window="hann", **dict(b, framing="center", pad_mode="constant"))
        front(kernel, f"{tag} mfcc pre0.97 centred reflect", mfcc[0], x7c, preemph_coef=0.97, **b, **centred)
        front(kernel, f"{tag} mfe pre0.97 hann centred constant", mfe[0], x7c, preemph_coef=0.97, mfcc_window="hann",
              **dict(b, framing="center", pad_mode="constant"))
        # a bank that reaches past bin fft_points / 4: the build with the whole P row, by its full name
        for (fn, what), build in ((mfcc, "<lib>"), (mfe, "<mfe,lib>")):
            front(kernel + build, f"{tag} {what} slaney bank to Nyquist (fullp)", fn, x7, mel_scale="slaney", mel_norm="slaney", **b)
        full = dict(b, frame_length=nfft / sr)  # no zero tail
        front(kernel, f"{tag} mfcc frame length {nfft}", mfcc[0], noise(3, clip_len(7, **full)), **full)
        front(kernel, f"{tag} mfe frame length {nfft} hann", mfe[0], noise(3, clip_len(7, **full)), mfcc_window="hann", **full)
        for filt in (41, 127):  # an odd count, and one whose DCT rows end in float4 padding
            front(kernel, f"{tag} mfcc {filt} filters", mfcc[0], x7, **dict(b, num_filters=filt))
        for ceps in (33, 64):
            front(kernel, f"{tag} mfcc {ceps} cepstra", mfcc[0], x7, **dict(b, num_filters=127, num_cepstral=ceps))
        front(kernel, f"{tag} mfcc one clip of one frame", mfcc[0], noise(1, clip_len(1, **b)), **b)
        front(kernel, f"{tag} mfe one clip of one frame", mfe[0], noise(1, clip_len(1, **b)), **b)

    # ---- ss_mel_c512 (two rows per wave) / ss_mel_c2048 (one) ----
    for kernel, tag, sr, nfft, hop, odd_hop, M in (("ss_mel_c512", "mel1024", 16000, 1024, 512, 441, 80),
                                                   ("ss_mel_c2048", "mel4096", 44100, 4096, 1024, 1103, 128)):
        def mp(h):  # (a quarter sample over: the hop comes out as h whether the library truncates or rounds)
            return dict(sample_rate=sr, fft_points=nfft, frame_length=(h + 0.25) / sr, frame_stride=(h + 0.25) / sr, num_filters=M)

        def st(x, h, sr=sr, nfft=nfft):
            return lambda: torch.view_as_real(ss.stft(x, sr, frame_length=(h + 0.25) / sr, fft_length=nfft))

        rows = ss.SpeechConfig(_lib.make_params(**mp(hop))).stft_rows
        xe = noise(3, next(n for n in range(6 * hop, 12 * hop, hop) if rows(n)[0] % 2 == 0))
        front(kernel, f"{tag} mel bank to Nyquist", mel, xe, **mp(hop))
        front(kernel, f"{tag} mel bank below bin {nfft // 4}", mel, xe, high_frequency=0.2 * sr, **mp(hop))
        out.append((f"{tag} stft", kernel + "<stft>", st(xe, hop)))
        xo = noise(3, 7 * odd_hop + 1 if odd_hop % 2 == 0 else 7 * odd_hop)  # an odd hop at an odd clip length
        front(kernel, f"{tag} mel odd hop {odd_hop}, odd clip length", mel, xo, **mp(odd_hop))
        out.append((f"{tag} stft odd hop {odd_hop}, odd clip length", kernel + "<stft>", st(xo, odd_hop)))
        xs = noise(2, nfft // 2 + 188)
        front(kernel, f"{tag} mel clip shorter than a window", mel, xs, **mp(hop))
        out.append((f"{tag} stft clip shorter than a window", kernel + "<stft>", st(xs, hop)))
        if kernel == "ss_mel_c512":  # an odd row count: the last pair of a clip is half dead
            xr = noise(3, next(n for n in range(6 * hop, 12 * hop, hop) if rows(n)[0] % 2 == 1))
            front(kernel, f"{tag} mel odd row count", mel, xr, **mp(hop))
            out.append((f"{tag} stft odd row count", kernel + "<stft>", st(xr, hop)))
    return out


def child(outdir):
    sys.path.insert(0, os.path.join(ROOT, "mfcc-rust_amd"))
    import numpy as np
    import torch

    import speechsauce_amd as ss
    from speechsauce_amd import _lib

    lib = _lib.lib()
    index = []
    for i, (name, kernel, thunk) in enumerate(cases(ss, np, torch)):
        res = thunk()
        torch.cuda.synchronize()
        got = lib.ss_last_kernel_name().decode()
        parts = res if isinstance(res, (tuple, list)) else (res,)
        blob = b"".join(p.detach().cpu().contiguous().numpy().tobytes() for p in parts)
        with open(os.path.join(outdir, f"{i:03d}.bin"), "wb") as f:
            f.write(blob)
        index.append({"name": name, "want": kernel, "kernel": got, "bytes": len(blob)})
    with open(os.path.join(outdir, "index.json"), "w") as f:
        json.dump(index, f)


def main():
    if len(sys.argv) == 3 and sys.argv[1] == "--child":
        child(sys.argv[2])
        return 0
    if len(sys.argv) != 3:
        print(__doc__)
        return 2
    with tempfile.TemporaryDirectory() as td:
        dirs = []
        for tag, libpath in (("before", sys.argv[1]), ("after", sys.argv[2])):
            d = os.path.join(td, tag)
            os.mkdir(d)
            env = dict(os.environ, SS_LIB_PATH=os.path.abspath(libpath))
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", d], env=env, timeout=CHILD_TIMEOUT_S)
            if r.returncode != 0:
                print(f"{tag} ({libpath}): the child ended with status {r.returncode}; nothing further is run")
                return 1
            dirs.append(d)
        ib, ia = (json.load(open(os.path.join(d, "index.json"))) for d in dirs)
        bad = 0 if len(ib) == len(ia) else 1
        for i, (b, a) in enumerate(zip(ib, ia)):
            fb, fa = (open(os.path.join(d, f"{i:03d}.bin"), "rb").read() for d in dirs)
            served = a["kernel"].startswith(a["want"]) and a["kernel"] == b["kernel"]
            same = fb == fa and len(fb) > 0 and served
            bad += 0 if same else 1
            note = "" if served else f"  (wanted {a['want']}, before ran {b['kernel']})"
            print(f"{'same     ' if same else 'DIFFERENT'}  {a['name']}: {a['kernel']}, {len(fa)} bytes{note}")
        print(f"{len(ia)} cases, {bad} different")
        return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
