"""Seeded sweep over the configuration space: every case goes through the public Python front (hence through whichever
kernel build the dispatcher picks: the builds of the 512-point kernel, the wide-bank one, the 256-, 1024-, 2048- and
4096-point kernels, the mel-spectrogram kernels, the generic kernel) and is compared with the oracle.

The metric here is the block metric, max|got - want| / max|want| over the whole block, on white noise: it finds a wrong
kernel, table or dispatch for any shape, but on MFCC it is dominated by column 0 (ln of the frame energy) and on mel outputs
by the loudest band.  The strict bars -- column 0 and the cepstra apart, every cepstral column and every mel band against its
own maximum -- live in tests/test_gpu_parity_strict.py (the three BASELINE configurations) and
tests/test_gpu_parity_families.py (one configuration per kernel family)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RTOL = 1e-4


def _rel(got, want):
    return float(np.abs(np.asarray(got, np.float64) - want).max() / max(np.abs(want).max(), 1e-30))


def _cases(n, seed):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        sr = int(rng.choice([8000, 16000, 22050, 44100]))
        n_fft = int(rng.choice([256, 512, 512, 512, 1024, 2048, 4096]))
        flen = int(rng.integers(n_fft // 4, n_fft + 1))
        if rng.random() < 0.7:
            flen &= ~1  # even frame lengths reach the dedicated kernels
        step = int(rng.integers(max(8, flen // 8), flen + 1))
        if rng.random() < 0.7:
            step &= ~1
        M = int(rng.choice([20, 26, 40, 40, 48, 64, 128, 256, 23, 41, 79, 127]))
        C = int(rng.integers(1, min(M, 40) + 1))
        kw = dict(sample_rate=sr, fft_points=n_fft, frame_length=(flen + 0.25) / sr, frame_stride=(step + 0.25) / sr,
                  num_cepstral=C, num_filters=M, low_frequency=float(rng.choice([0.0, 50.0, 300.0])),
                  high_frequency=float(sr / 2 * rng.choice([1.0, 1.0, 0.8])), dc_elimination=bool(rng.random() < 0.7))
        sw = {}
        if rng.random() < 0.3:
            sw["mfcc_window"] = str(rng.choice(["hann", "vorbis"]))
        if rng.random() < 0.25:
            sw["preemph_coef"] = 0.97
            sw["preemph_shift"] = int(rng.choice([1, 1, 2, 5]))
        if rng.random() < 0.25:
            sw["spectrum_exponent"] = 2
        if rng.random() < 0.25:
            sw["dct_norm"] = "ortho"
        if rng.random() < 0.15:
            sw.update(framing="center", pad_mode=str(rng.choice(["reflect", "constant"])))
        if rng.random() < 0.2:
            sw.update(mel_scale=str(rng.choice(["slaney", "htk"])), mel_norm=str(rng.choice(["none", "slaney"])))
        batch = int(rng.choice([1, 3, 9]))
        n_samples = int(flen + step * rng.integers(1, 40) + rng.integers(0, step))
        out.append((kw, sw, batch, n_samples))
    return out


SEEN = set()


@pytest.mark.parametrize("block", range(6))
def test_random_configurations(ss, oracle, sslib, block):
    import torch

    kernels = set()
    for i, (kw, sw, batch, n) in enumerate(_cases(24, 1000 + block)):
        try:
            p = oracle.make_params(**kw, **sw)
            oracle.filterbank(p)
            T = oracle.num_frames(p, n)
        except oracle.OracleError:
            continue  # a combination the reference itself rejects (filter edges outside the spectrum, no frames, ...)
        x = (np.random.default_rng(7 * i + block).standard_normal((batch, n)) * 0.1).astype(np.float32)
        args = dict(frame_length=kw["frame_length"], frame_stride=kw["frame_stride"], num_cepstral=kw["num_cepstral"],
                    num_filters=kw["num_filters"], fft_length=kw["fft_points"], low_frequency=kw["low_frequency"],
                    high_frequency=kw["high_frequency"], dc_elimination=kw["dc_elimination"])
        got = ss.mfcc_batch(torch.from_numpy(x).cuda(), kw["sample_rate"], **args, **sw).cpu().numpy()
        kernels.add(sslib.ss_last_kernel_name().decode().split("<")[0])
        SEEN.add(sslib.ss_last_kernel_name().decode().split("<")[0])
        assert got.shape == (batch, T, kw["num_cepstral"]), (kw, sw)
        for b in {0, batch - 1}:
            assert _rel(got[b], oracle.mfcc(p, x[b])) <= RTOL, (kw, sw, b)
        margs = {k: v for k, v in args.items() if k not in ("num_cepstral", "dc_elimination")}
        feat, en = ss.mfe_batch(torch.from_numpy(x).cuda(), kw["sample_rate"], **margs, **sw)
        wf, we = oracle.mfe(p, x[batch - 1])
        assert _rel(feat[batch - 1].cpu().numpy(), wf) <= RTOL and _rel(en[batch - 1].cpu().numpy(), we) <= RTOL, (kw, sw)
    assert kernels  # at least one case ran


def test_sweep_reached_every_frame_kernel():
    """The seeded sweep above is only worth its name if the dispatcher sent cases to every frame-path kernel family."""
    if not SEEN:
        pytest.skip("runs after test_random_configurations in the same process")
    want = {"ss_mfcc_c256", "ss_mfcc_c256w", "ss_mfcc_c256x2", "ss_mfcc_c512", "ss_mfcc_c1024", "ss_mfcc_c2048", "ss_front_generic"}
    assert want <= SEEN, sorted(want - SEEN)


def test_random_mel_spectrogram_configurations(ss, oracle, sslib):
    """STFT branch (feature.rs:151-174): random fft sizes / hops / filter counts / channel counts, 1-D and 2-D inputs."""
    rng = np.random.default_rng(4242)
    ran = 0
    for i in range(40):
        sr = int(rng.choice([8000, 16000, 44100]))
        n_fft = int(rng.choice([256, 512, 1024, 2048, 2048, 4096]))
        hop = int(rng.integers(n_fft // 16, n_fft // 2 + 1))
        if rng.random() < 0.6:
            hop &= ~1
        M = int(rng.choice([20, 40, 64, 128]))
        kw = dict(sample_rate=sr, fft_points=n_fft, frame_length=(hop + 0.5) / sr, frame_stride=(hop + 0.5) / sr, num_cepstral=13,
                  num_filters=M, low_frequency=0.0, high_frequency=float(sr / 2 * rng.choice([1.0, 0.9])))
        ch = int(rng.choice([1, 1, 2, 5]))
        n = int(rng.integers(hop * 3, hop * 40))
        if rng.random() < 0.5:
            n &= ~1
        try:
            p = oracle.make_params(**kw)
            oracle.filterbank(p)
            oracle.stft_rows(p, n)
        except oracle.OracleError:
            continue
        x = (np.random.default_rng(100 + i).standard_normal((ch, n)) * 0.1).astype(np.float32)
        args = dict(frame_length=kw["frame_length"], frame_stride=kw["frame_stride"], num_filters=M, fft_length=n_fft,
                    high_frequency=kw["high_frequency"])
        sig = x[0] if ch == 1 and rng.random() < 0.5 else x
        got = ss.mel_spectrogram(sig, sr, **args)
        want = oracle.mel_spectrogram(p, sig)
        assert got.shape == want.shape, (kw, ch, n)
        assert _rel(got, want) <= RTOL, (kw, ch, n)
        ran += 1
    assert ran >= 20


def test_uninitialised_lds_never_reaches_results(ss, oracle, sslab):
    """LDS keeps what the previous kernel left in it.  Every sweep configuration (and a list of named ones: windowed and
    librosa builds, mel / stft kernels, chirp-z) runs once normally and once right after ss_debug_poison_lds (a kernel of the LAB
    library; the launches under test are the product library's) has filled every
    CU's LDS with 0xFFFFFFFF (NaN as f32, -1 as i32): the results must be finite and bit-identical -- a kernel that multiplies
    a padded zero with a table word it never wrote, or reads a pad bin it never cleared, fails here."""
    import torch

    def both(fn):
        a = fn()
        assert sslab.ss_debug_poison_lds(None) == 0
        b = fn()
        torch.cuda.synchronize()
        return a, b

    def same(a, b, what):
        a = [t.cpu().numpy() for t in (a if isinstance(a, tuple) else (a,))]
        b = [t.cpu().numpy() for t in (b if isinstance(b, tuple) else (b,))]
        for u, v in zip(a, b):
            assert np.all(np.isfinite(v)), what
            assert np.array_equal(u, v), what

    ran = 0
    for block in range(6):
        for i, (kw, sw, batch, n) in enumerate(_cases(24, 1000 + block)):
            try:
                p = oracle.make_params(**kw, **sw)
                oracle.filterbank(p)
                oracle.num_frames(p, n)
            except oracle.OracleError:
                continue
            x = torch.from_numpy((np.random.default_rng(7 * i + block).standard_normal((batch, n)) * 0.1).astype(np.float32)).cuda()
            args = dict(frame_length=kw["frame_length"], frame_stride=kw["frame_stride"], num_cepstral=kw["num_cepstral"],
                        num_filters=kw["num_filters"], fft_length=kw["fft_points"], low_frequency=kw["low_frequency"],
                        high_frequency=kw["high_frequency"], dc_elimination=kw["dc_elimination"])
            same(*both(lambda: ss.mfcc_batch(x, kw["sample_rate"], **args, **sw)), (kw, sw))
            margs = {k: v for k, v in args.items() if k not in ("num_cepstral", "dc_elimination")}
            same(*both(lambda: ss.mfe_batch(x, kw["sample_rate"], **margs, **sw)), (kw, sw, "mfe"))
            ran += 1
    assert ran > 60
    # named configurations
    lib = dict(framing="center", pad_mode="reflect", mfcc_window="hann", spectrum_exponent=2, mel_scale="slaney", mel_norm="slaney", dct_norm="ortho")
    x16 = torch.from_numpy((np.random.default_rng(5).standard_normal((5, 16000)) * 0.1).astype(np.float32)).cuda()
    x44 = torch.from_numpy((np.random.default_rng(6).standard_normal((3, 30000)) * 0.1).astype(np.float32)).cuda()
    named = [
        (x16, 16000, dict(), {}), (x16, 16000, dict(), dict(mfcc_window="hann")), (x16, 16000, dict(), dict(preemph_coef=0.97)),
        (x16, 16000, dict(frame_length=260 / 16000), dict(lib, pad_mode="constant")), (x16, 16000, dict(frame_length=0.025, num_filters=80), lib),
        (x16, 8000, dict(fft_length=256), dict(mfcc_window="hann")), (x16, 16000, dict(fft_length=400, frame_length=0.025), {}),
        (x44, 22050, dict(fft_length=1024, frame_length=700 / 22050, frame_stride=256 / 22050, num_filters=64, num_cepstral=20), dict(mfcc_window="hann")),
        (x44, 44100, dict(fft_length=2048, frame_length=1500 / 44100, frame_stride=512 / 44100, num_filters=128, num_cepstral=20), lib),
        (x44, 44100, dict(fft_length=4096, frame_length=3000 / 44100, frame_stride=1024 / 44100, num_filters=128, num_cepstral=20), dict(mfcc_window="hann")),
    ]
    for x, sr, kw, sw in named:
        same(*both(lambda: ss.mfcc_batch(x, sr, **kw, **sw)), (sr, kw, sw))
    for nfft, sr, hop, M in ((512, 16000, 256, 40), (1024, 16000, 512, 80), (2048, 16000, 512, 128), (4096, 44100, 1024, 128), (400, 16000, 200, 40), (256, 8000, 128, 20)):
        x = x44 if sr == 44100 else x16
        same(*both(lambda: ss.mel_spectrogram(x, sr, frame_length=hop / sr, frame_stride=hop / sr, num_filters=M, fft_length=nfft)), ("mel", nfft))


def test_post_processing_on_poisoned_lds(ss, sslab):
    """cmvn / cmvnw / derivative kernels (processing.rs:222-380) give bit-identical results after ss_debug_poison_lds."""
    import torch

    feats = torch.from_numpy((np.random.default_rng(9).standard_normal((6, 98, 13))).astype(np.float32)).cuda()
    for fn in (lambda: ss.cmvn(feats, False), lambda: ss.cmvn(feats, True), lambda: ss.cmvnw(feats, 301, False),
               lambda: ss.cmvnw(feats, 51, True), lambda: ss.derivative_extraction(feats, 2), lambda: ss.extract_derivative_feature(feats)):
        a = fn().cpu().numpy()
        assert sslab.ss_debug_poison_lds(None) == 0
        b = fn().cpu().numpy()
        assert np.all(np.isfinite(b)) and np.array_equal(a, b)
