"""The Whisper log-mel specification of include/speechsauce_amd.h (ss_whisper_*) restated in numpy: log_mel() in f64 (the reference
of every test), log_mel_f32() with every array held in f32 (its score against f64 is the yardstick of the kernel's), the Slaney
bank as librosa.filters.mel builds it, the silent-frame rule by brute force and as the closed form, and the seeded inputs of the
tests."""
import numpy as np

SR, N_FFT, HOP, BINS = 16000, 400, 160, 201


def window(dtype=np.float64):
    n = np.arange(N_FFT, dtype=np.float64)
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * n / N_FFT)).astype(dtype)


def _hz_to_mel(f):
    f = np.asarray(f, np.float64)
    f_sp, min_log_hz = 200.0 / 3.0, 1000.0
    logstep = np.log(6.4) / 27.0
    return np.where(f >= min_log_hz, min_log_hz / f_sp + np.log(np.maximum(f, 1e-300) / min_log_hz) / logstep, f / f_sp)


def _mel_to_hz(m):
    m = np.asarray(m, np.float64)
    f_sp, min_log_hz = 200.0 / 3.0, 1000.0
    min_log_mel, logstep = min_log_hz / f_sp, np.log(6.4) / 27.0
    return np.where(m >= min_log_mel, min_log_hz * np.exp(logstep * (m - min_log_mel)), f_sp * m)


def mel_bank(n_mels):
    """librosa.filters.mel(sr=16000, n_fft=400, n_mels=n_mels, htk=False, norm="slaney") in f64, [n_mels x 201]"""
    fft_f = np.arange(BINS, dtype=np.float64) * SR / N_FFT
    mel_f = _mel_to_hz(np.linspace(_hz_to_mel(0.0), _hz_to_mel(SR / 2.0), n_mels + 2))
    fdiff = np.diff(mel_f)
    ramps = mel_f[:, None] - fft_f[None, :]
    lower = -ramps[:-2] / fdiff[:-1, None]
    upper = ramps[2:] / fdiff[1:, None]
    w = np.maximum(0.0, np.minimum(lower, upper))
    return w * (2.0 / (mel_f[2:n_mels + 2] - mel_f[:n_mels]))[:, None]


def power(x, n_frames, dtype=np.float64):
    """P [n_frames x 201] of one clip, padded or trimmed to n_frames * 160 samples"""
    N = n_frames * HOP
    a = np.zeros(N, dtype)
    x = np.asarray(x, dtype)[:N]
    a[:x.size] = x
    p = np.pad(a, N_FFT // 2, mode="reflect")
    w = window(dtype)
    idx = HOP * np.arange(n_frames)[:, None] + np.arange(N_FFT)[None, :]
    spec = np.fft.rfft((p[idx] * w).astype(dtype), axis=1)
    if dtype == np.float32:
        spec = spec.astype(np.complex64)
        return (spec.real * spec.real + spec.imag * spec.imag).astype(np.float32)
    return np.abs(spec) ** 2


def log_mel(x, n_mels, n_frames):
    """the specification, f64: [n_mels x n_frames]"""
    mel = mel_bank(n_mels) @ power(x, n_frames).T
    l = np.log10(np.maximum(mel, 1e-10))
    l = np.maximum(l, l.max() - 8.0)
    return (l + 4.0) / 4.0


def log_mel_f32(x, n_mels, n_frames):
    """the same with every array in f32 (numpy's pocketfft transforms in the precision of its input)"""
    B = mel_bank(n_mels).astype(np.float32)
    mel = (B @ power(x, n_frames, np.float32).T).astype(np.float32)
    l = np.log10(np.maximum(mel, np.float32(1e-10))).astype(np.float32)
    l = np.maximum(l, np.float32(l.max() - np.float32(8.0)))
    return ((l + np.float32(4.0)) / np.float32(4.0)).astype(np.float32)


def silent_frames_brute(length, n_frames):
    """per frame: every sample index of the frame, after reflection, lies at or beyond min(length, N)"""
    N = n_frames * HOP
    L = min(length, N)
    idx = np.pad(np.arange(N), N_FFT // 2, mode="reflect")
    return [bool((idx[HOP * t:HOP * t + N_FFT] >= L).all()) for t in range(n_frames)]


def first_silent(length, n_frames):
    """the closed form of the header: the first silent frame, n_frames if there is none"""
    L = min(length, n_frames * HOP)
    if L == 0:
        return 0
    return min(max(2, -(-(L + N_FFT // 2) // HOP)), n_frames)


def to_bf16_bits(a):
    """ss_pad_packed's bfloat16 rule on f32 values -> uint16 bit patterns"""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint32)
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    r = np.where(nan, (u >> 16) | 0x40, r)
    return r.astype(np.uint16)


def make_input(kind, n, seed):
    """the seeded inputs of the tests: 'normal' = standard_normal * 0.1, 'pcm' = the same x 32768 (unscaled), 'tone' = a 440 Hz tone
    of amplitude 0.5 plus noise at -60 dB"""
    rng = np.random.default_rng(seed)
    if kind == "normal":
        return (rng.standard_normal(n) * 0.1).astype(np.float32)
    if kind == "pcm":
        return (rng.standard_normal(n) * 0.1 * 32768.0).astype(np.float32)
    if kind == "tone":
        t = np.arange(n, dtype=np.float64) / SR
        return (0.5 * np.sin(2.0 * np.pi * 440.0 * t) + 0.5e-3 * rng.standard_normal(n)).astype(np.float32)
    raise ValueError(kind)


WAVES = 8  # ss::whisper::kWaves: waves of the persistent workgroup, one workgroup per CU


def loop_clips(num_cus):
    """clips of the loop test (tests/test_whisper_loop.py): one 16-frame unit each, 3 * waves * CUs + 5 of them"""
    return 3 * WAVES * num_cus + 5
