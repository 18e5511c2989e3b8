#!/usr/bin/env python3
"""Records tests/golden/whisper_v1.npz from transformers.WhisperFeatureExtractor (its numpy implementation: no download, no
device): the [M x 100] features of a seeded 1 s clip for 80 and 128 mels and a few rows of both mel banks.  tests/test_whisper_cpu.py
holds the numpy restatement (tests/whisper_model.py) to these at 5e-6.

    python tools/whisper_golden.py            # writes the fixture
    python tools/whisper_golden.py --check    # compares a fresh recording with the committed file
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATH = os.path.join(ROOT, "tests", "golden", "whisper_v1.npz")
SEED, N = 2026, 16000
BANK_ROWS = (0, 1, 17, 40, 79)


def record():
    from transformers import WhisperFeatureExtractor

    x = (np.random.default_rng(SEED).standard_normal(N) * 0.1).astype(np.float32)
    out = {"seed": np.int64(SEED), "n_samples": np.int64(N), "bank_rows": np.array(BANK_ROWS, np.int64)}
    for m in (80, 128):
        fe = WhisperFeatureExtractor(feature_size=m)
        feats = fe(x, sampling_rate=16000, padding="longest", return_tensors="np")["input_features"][0]
        assert feats.shape == (m, N // 160), feats.shape
        out[f"features_{m}"] = np.ascontiguousarray(feats, np.float32)
        bank = np.asarray(fe.mel_filters, np.float64)  # [201 x M]
        out[f"bank_{m}"] = np.ascontiguousarray(bank.T[list(BANK_ROWS)])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true")
    args = ap.parse_args()
    got = record()
    if args.check:
        want = np.load(PATH)
        for k, v in got.items():
            assert np.array_equal(want[k], v), k
        print("whisper_v1.npz matches a fresh recording")
        return 0
    np.savez_compressed(PATH, **got)
    print(f"wrote {PATH} ({os.path.getsize(PATH)} bytes)")
    return 0


if __name__ == "__main__":
    sys.exit(main())
