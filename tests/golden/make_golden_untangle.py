"""Outputs of every build of the 512-point MFCC kernel template (ss_mfcc_c256) on seeded inputs, recorded from the library as it
stood BEFORE the real-FFT untangle took its partner value by a row_mirror DPP read instead of ds_bpermute_b32.  That change moves
bits between lanes and leaves the arithmetic, its order and its contraction alone, so every output has to stay bit-identical:
tests/test_untangle_dpp_identity.py runs `cases()` on the current build and compares with array_equal, no tolerance.

Run on the GPU box against the library to record:  python tests/golden/make_golden_untangle.py  ->  untangle_dpp_v1.npz
(whole clips chosen by seeded index lists, so that the file stays small)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "untangle_dpp_v1.npz")
SR = 16000


def _noise(seed, shape, scale=0.1):
    return (np.random.default_rng(seed).standard_normal(shape) * scale).astype(np.float32)


def _pick(seed, n, k):
    return np.sort(np.random.default_rng(seed).choice(n, size=k, replace=False))


def cases(ss, torch):
    """-> (arrays {name: ndarray}, kernels {case: kernel name}) of the library `ss` runs on."""
    dev = "cuda:0"
    last = lambda: ss._lib.lib().ss_last_kernel_name().decode()
    host = lambda t: t.detach().cpu().numpy()
    arrays, kernels = {}, {}

    # cfg2: bench.py's headline shape, 1024 clips of 1 s
    x = torch.from_numpy(_noise(1234, (1024, SR))).to(dev)
    out = host(ss.mfcc_batch(x, SR))
    kernels["cfg2"] = last()
    arrays["cfg2"] = out[_pick(1, 1024, 6)]

    # mfe: features + frame energy
    x = torch.from_numpy(_noise(2, (64, SR))).to(dev)
    feat, en = ss.mfe_batch(x, SR)
    kernels["mfe"] = last()
    idx = _pick(2, 64, 4)
    arrays["mfe_feat"], arrays["mfe_energy"] = host(feat)[idx], host(en)[idx]

    # power rows: all 257 bins of every frame
    x = torch.from_numpy(_noise(3, (16, SR))).to(dev)
    pw = host(ss.power_spectrum_of_signal(x, SR))
    kernels["power"] = last()
    arrays["power"] = pw[_pick(3, 16, 2)]

    # frame window + fused pre-emphasis in front of the transform (MFCC and mfe)
    x = torch.from_numpy(_noise(4, (16, SR))).to(dev)
    out = host(ss.mfcc_batch(x, SR, mfcc_window="hann", preemph_coef=0.97))
    kernels["win_pre"] = last()
    arrays["win_pre"] = out[_pick(4, 16, 4)]
    feat, en = ss.mfe_batch(x, SR, mfcc_window="hann", preemph_coef=0.97)
    kernels["win_pre_mfe"] = last()
    arrays["win_pre_mfe_feat"], arrays["win_pre_mfe_energy"] = host(feat)[:2], host(en)[:2]

    # packed clips of different lengths, one launch
    lengths = [16000, 5000, 481, 8000, 12345, 640, 2001, 960]
    x = torch.from_numpy(_noise(5, (sum(lengths),))).to(dev)
    out, fo = ss.mfcc_packed(x, lengths, SR)
    kernels["packed"] = last()
    arrays["packed"], arrays["packed_fo"] = host(out), host(fo)

    # streaming: three streams, a chunk of ten hops and then one hop (every frame of the second call reaches into the state)
    xs = _noise(6, (3, 11 * 160))
    st = ss.MfccStream(3, SR, norm_frames=99)
    arrays["stream_a"] = host(st(torch.from_numpy(xs[:, :1600].copy()).to(dev)))
    kernels["stream"] = last()
    arrays["stream_b"] = host(st(torch.from_numpy(xs[:, 1600:].copy()).to(dev)))
    se = ss.MfeStream(3, SR)
    feat, en = se(torch.from_numpy(xs[:, :1600].copy()).to(dev))
    kernels["stream_mfe"] = last()
    arrays["stream_mfe_feat"], arrays["stream_mfe_energy"] = host(feat), host(en)

    # two batches behind one batch table (ss_mfcc_batches_device)
    xa, xb = torch.from_numpy(_noise(7, (9, SR))).to(dev), torch.from_numpy(_noise(8, (130, SR))).to(dev)
    oa, ob = ss.mfcc_batch([xa, xb], SR)
    kernels["batches"] = last()
    arrays["batches_a"], arrays["batches_b"] = host(oa)[_pick(7, 9, 3)], host(ob)[_pick(8, 130, 4)]

    # short clips: 3 x 6 frames = 18, so the last quad holds two frames
    x = torch.from_numpy(_noise(9, (3, 1280))).to(dev)
    out = host(ss.mfcc_batch(x, SR))
    kernels["short"] = last()
    assert (out.shape[0] * out.shape[1]) % 4 != 0, out.shape
    arrays["short"] = out

    # all-zero clips: the zero-handling branches of the energy and the mel stage
    x = torch.zeros((2, SR), dtype=torch.float32, device=dev)
    arrays["zero"] = host(ss.mfcc_batch(x, SR))
    kernels["zero"] = last()
    feat, en = ss.mfe_batch(x, SR)
    arrays["zero_mfe_feat"], arrays["zero_mfe_energy"] = host(feat), host(en)
    return arrays, kernels


# every case runs on a build of the ss_mfcc_c256 template (the c256m / c256v / c256s names are its batch-table, packed and
# streaming builds)
KERNEL_PREFIX = "ss_mfcc_c256"


if __name__ == "__main__":
    root = os.path.dirname(os.path.dirname(HERE))
    sys.path.insert(0, os.path.join(root, "mfcc-rust_amd"))
    import torch

    import speechsauce_amd as ss

    arrays, kernels = cases(ss, torch)
    for k, v in kernels.items():
        assert v.startswith(KERNEL_PREFIX), (k, v)
        print(f"{k:12s} {v}")
    out = sys.argv[1] if len(sys.argv) > 1 else OUT
    np.savez_compressed(out, **arrays, **{"kernel_" + k: np.array(v) for k, v in kernels.items()})
    print(f"wrote {out}: {os.path.getsize(out)} bytes, {len(arrays)} arrays")
