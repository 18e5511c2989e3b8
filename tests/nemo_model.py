"""The NeMo / Parakeet log-mel specification of include/speechsauce_amd.h (ss_nemo_*) restated in numpy: features() in f64 (the
reference of every test), the same with every array held in f32 (its score against f64 is the yardstick of the kernel's), the
Slaney bank as librosa.filters.mel builds it (tests/whisper_model.py's mel-scale helpers at n_fft = 512), the torch.stft wording of
transformers' ParakeetFeatureExtractor lines, and the seeded inputs and shapes of the tests."""
import numpy as np

from whisper_model import _hz_to_mel, _mel_to_hz

SR, N_FFT, HOP, BINS = 16000, 512, 160, 257
GUARD = 2.0 ** -24
NORM_EPS = float(np.float32(1e-5))  # the parameter is an f32, widened
PREEMPH = float(np.float32(0.97))   # likewise


def window(W=400, dtype=np.float64):
    n = np.arange(W, dtype=np.float64)
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * n / (W - 1))).astype(dtype)


def mel_bank(n_mels):
    """librosa.filters.mel(sr=16000, n_fft=512, n_mels=n_mels, fmin=0, fmax=8000, htk=False, norm="slaney") in f64, [n_mels x 257]"""
    fft_f = np.arange(BINS, dtype=np.float64) * SR / N_FFT
    mel_f = _mel_to_hz(np.linspace(_hz_to_mel(0.0), _hz_to_mel(SR / 2.0), n_mels + 2))
    fdiff = np.diff(mel_f)
    ramps = mel_f[:, None] - fft_f[None, :]
    lower = -ramps[:-2] / fdiff[:-1, None]
    upper = ramps[2:] / fdiff[1:, None]
    w = np.maximum(0.0, np.minimum(lower, upper))
    return w * (2.0 / (mel_f[2:n_mels + 2] - mel_f[:n_mels]))[:, None]


def num_frames(n_samples):
    return n_samples // HOP


def preemphasized(x, c=PREEMPH, dtype=np.float64):
    """step 2 on the clip's own samples: y[i] = fmaf(-c, x[i - 1], x[i]), x[-1] = 0 (f32: the f64 value, exact but for its last
    bit, rounded once)"""
    x = np.asarray(x, np.float64)
    y = x.copy()
    y[1:] -= c * x[:-1]
    return y.astype(dtype)


def power(x, W=400, c=PREEMPH, dtype=np.float64):
    """P [T x 257] of one clip: steps 1 - 4"""
    T, half = num_frames(len(x)), W // 2
    y = np.concatenate([np.zeros(half, dtype), preemphasized(x, c, dtype), np.zeros(W, dtype)])  # zero before and behind the clip
    idx = HOP * np.arange(T)[:, None] + np.arange(W)[None, :]  # frame t starts at clip sample t H - N / 2 + lo = t H - W / 2
    s = (y[idx] * window(W, dtype)).astype(dtype)
    spec = np.fft.rfft(s, n=N_FFT, axis=1)  # the live samples at positions 0 .. W - 1
    if dtype == np.float32:
        spec = spec.astype(np.complex64)
        return (spec.real * spec.real + spec.imag * spec.imag).astype(np.float32)
    return np.abs(spec) ** 2


def log_mel(x, n_mels, W=400, c=PREEMPH, guard=GUARD):
    """steps 1 - 6 in f64: [T x n_mels]"""
    B = mel_bank(n_mels).astype(np.float32).astype(np.float64)  # the bank is rounded to f32
    return np.log(power(x, W, c) @ B.T + guard)


def normalized(l, eps=NORM_EPS):
    """step 8 in f64 on rows [T x n_mels]; T = 1: the deviation is 0"""
    l = np.asarray(l, np.float64)
    T = l.shape[0]
    if T == 0:
        return l.copy()
    mean = l.sum(axis=0) / T
    var = ((l - mean) ** 2).sum(axis=0) / (T - 1) if T > 1 else np.zeros(l.shape[1])
    return (l - mean) / (np.sqrt(var) + eps)


def features(x, n_mels, normalize=True, W=400, c=PREEMPH):
    """the specification, f64"""
    l = log_mel(x, n_mels, W, c)
    return normalized(l) if normalize else l


def features_f32(x, n_mels, normalize=True, W=400, c=PREEMPH):
    """the same with every array in f32 (numpy's pocketfft transforms in the precision of its input); step 8 keeps its f64 sums"""
    B = mel_bank(n_mels).astype(np.float32)
    l = np.log((power(x, W, c, np.float32) @ B.T).astype(np.float32) + np.float32(GUARD)).astype(np.float32)
    return normalized(l).astype(np.float32) if normalize else l


def block_metric(got, want):
    return float(np.abs(np.asarray(got, np.float64) - want).max() / np.abs(want).max())


def extractor_wording(x, n_mels, W=400, c=0.97, normalize=True):
    """The lines of transformers' ParakeetFeatureExtractor (__call__ and _torch_extract_fbank_features) on one unpadded clip, in
    torch f32 on the CPU; the extractor's librosa bank is mel_bank() rounded to f32.  -> [T x n_mels], T = features_lengths."""
    import torch

    feats = torch.from_numpy(np.asarray(x, np.float32))[None, :]
    feats = torch.cat([feats[:, :1], feats[:, 1:] - c * feats[:, :-1]], dim=1)
    win = torch.hann_window(W, periodic=False)
    stft = torch.stft(feats, N_FFT, hop_length=HOP, win_length=W, window=win, return_complex=True, pad_mode="constant")
    mag = torch.sqrt(torch.view_as_real(stft).pow(2).sum(-1)).pow(2)
    mel = torch.from_numpy(mel_bank(n_mels).astype(np.float32)) @ mag
    mel = torch.log(mel + 2 ** -24).permute(0, 2, 1)
    T = (len(x) + N_FFT // 2 * 2 - N_FFT) // HOP
    mel = mel[0, :T]
    if not normalize:
        return mel.numpy()
    mean = mel.sum(dim=0) / T
    var = ((mel - mean) ** 2).sum(dim=0) / (T - 1)
    return ((mel - mean) / (torch.sqrt(var) + 1e-5)).numpy()


# ---- the inputs and shapes of the GPU tests (tests/test_nemo.py; their f32 yardstick is taken in tests/test_nemo_cpu.py) ----
# every edge case of the loader: one row whose frame overhangs both ends; the same plus a sample; two rows, the clip shorter than
# the window by 80, by one sample, equal to it, longer by one; three rows, the last of them wholly inside its clip (the quad still
# takes the per-sample path); 18 rows: an edge quad, three interior quads and an interior quad with redone lanes
GPU_LENS = (160, 161, 320, 399, 400, 401, 560, 3000)
GPU_BANDS = (80, 128)


def make_input(n, seed):
    """seeded noise at 0.1"""
    return (np.random.default_rng(seed).standard_normal(n) * 0.1).astype(np.float32)


def gpu_clip(L):
    return make_input(L, 1000 + L)


# the persistent loop (tests/test_nemo.py::test_dense_loop): 64 clips of 200 frames are 3200 quads, more than 12 waves x 256 CUs
LOOP_CLIPS, LOOP_FRAMES, WAVES = 64, 200, 12


def loop_quads():
    return LOOP_CLIPS * LOOP_FRAMES // 4
