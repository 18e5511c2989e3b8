"""The persistent loop of ss_whisper_c200: one dense and one packed call sized so that every wave takes at least two further units
from its workgroup's LDS counter (3 * waves * CUs + 5 units of one short clip each; tests/test_whisper_cpu.py checks that arithmetic
for 64, 256 and 304 CUs).  The big call equals, bit for bit, the concatenation of calls on consecutive sub-blocks, and sampled clips
meet the f64 restatement at the bar."""
import numpy as np
import pytest

import whisper_model as wm

pytestmark = pytest.mark.gpu

BAR = 1e-4


@pytest.fixture(scope="module")
def setup(sslib):
    import torch

    import speechsauce_amd as ss

    assert torch.cuda.is_available()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = wm.loop_clips(cus)
    rng = np.random.default_rng(11)
    dense = torch.from_numpy((rng.standard_normal((n, 1280)) * 0.1).astype(np.float32)).cuda()  # 8 frames: one unit per clip
    return ss, torch, n, dense


def test_dense_call_equals_its_sub_blocks(setup):
    ss, torch, n, x = setup
    big = ss.whisper_log_mel(x, n_mels=128)  # [n, 128, 8]
    assert big.shape == (n, 128, 8)
    cuts = [0, 1, 9, n // 3, n // 3 + 257, n - 4, n]
    parts = [ss.whisper_log_mel(x[a:b], n_mels=128) for a, b in zip(cuts[:-1], cuts[1:])]
    assert torch.equal(big, torch.cat(parts))
    xs = x.cpu().numpy()
    got = big.cpu().numpy()
    for b in (0, 1, n // 2, n - 6, n - 1):
        assert np.abs(got[b] - wm.log_mel(xs[b], 128, 8)).max() <= BAR


def test_packed_call_equals_its_sub_blocks(setup):
    ss, torch, n, x = setup
    rng = np.random.default_rng(12)
    lens = rng.integers(1281, 1441, n)  # 8 frames of their own, padded to the 9-frame window: odd and even offsets
    lens[::97] = 0
    so = np.concatenate([[0], np.cumsum(lens)])
    packed = torch.from_numpy((rng.standard_normal(int(so[-1])) * 0.1).astype(np.float32)).cuda()
    big, blen = ss.whisper_log_mel_packed(packed, lens, n_mels=128, n_frames=9, dtype="bfloat16")
    assert big.shape == (n, 128, 9)
    cuts = [0, 3, n // 2 + 1, n - 7, n]
    outs, ls = zip(*[ss.whisper_log_mel_packed(packed[so[a]:so[b]], lens[a:b], n_mels=128, n_frames=9, dtype="bfloat16")
                     for a, b in zip(cuts[:-1], cuts[1:])])
    assert torch.equal(big.view(torch.int16), torch.cat(outs).view(torch.int16)) and torch.equal(blen, torch.cat(ls))
    assert blen.cpu().tolist() == [min(int(k) // 160, 9) for k in lens]
    f32, _ = ss.whisper_log_mel_packed(packed, lens, n_mels=128, n_frames=9)
    xs, got = packed.cpu().numpy(), f32.cpu().numpy()
    for b in (0, 2, 97, n // 2, n - 1):
        assert np.abs(got[b] - wm.log_mel(xs[so[b]:so[b + 1]], 128, 9)).max() <= BAR
