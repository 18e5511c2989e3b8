"""The real-FFT untangle of ss_mfcc_c256 reads its partner value Z[256 - k] from the row_mirror lane of the DPP row (lanes hold a
permuted column, ss_wave.h: untangle_col) instead of fetching it with ds_bpermute_b32.  A DPP read moves bits unchanged and the
arithmetic, its order and its FMA contraction were not touched, so every output of every build of the template has to be
bit-identical to the library before the change: tests/golden/untangle_dpp_v1.npz was recorded from that library by
tests/golden/make_golden_untangle.py, and the same seeded calls are repeated here.  array_equal, no tolerance, nothing skipped."""
import os

import numpy as np
import pytest

from common import BENCH_KERNELS

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "untangle_dpp_v1.npz")

ARRAYS = ["cfg2", "mfe_feat", "mfe_energy", "power", "win_pre", "win_pre_mfe_feat", "win_pre_mfe_energy", "packed", "packed_fo",
          "stream_a", "stream_b", "stream_mfe_feat", "stream_mfe_energy", "batches_a", "batches_b", "short", "zero", "zero_mfe_feat",
          "zero_mfe_energy"]


@pytest.fixture(scope="module")
def recomputed(ss, sslib):
    import torch
    from golden.make_golden_untangle import cases

    return cases(ss, torch)


def test_fixture_is_complete():
    want = np.load(FIXTURE)
    assert sorted(k for k in want.files if not k.startswith("kernel_")) == sorted(ARRAYS)
    assert want["cfg2"].shape == (6, 98, 13) and want["power"].shape == (2, 98, 257) and want["short"].shape == (3, 6, 13)
    assert str(want["kernel_cfg2"]) == BENCH_KERNELS["cfg2"].decode()
    for k in want.files:
        if not k.startswith("kernel_") and k != "packed_fo":
            assert want[k].dtype == np.float32 and np.isfinite(want[k]).all(), k
    assert os.path.getsize(FIXTURE) < 1 << 20


@pytest.mark.gpu
def test_same_kernel_builds(recomputed):
    want = np.load(FIXTURE)
    _, kernels = recomputed
    assert kernels["cfg2"] == BENCH_KERNELS["cfg2"].decode()
    for case, name in kernels.items():
        assert name == str(want["kernel_" + case]), (case, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ARRAYS)
def test_bit_identical(recomputed, name):
    want = np.load(FIXTURE)[name]
    got = recomputed[0][name]
    assert got.shape == want.shape and got.dtype == want.dtype
    diff = int((got.view(np.uint32) != want.view(np.uint32)).sum()) if got.dtype == np.float32 else int((got != want).sum())
    print(f"{name}: {got.size} values, {diff} differ in their bits")
    assert np.array_equal(got, want)
    if got.dtype == np.float32:  # array_equal takes -0.0 == +0.0: the bit patterns too
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
