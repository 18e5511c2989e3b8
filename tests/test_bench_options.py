"""bench.py's plain line (no --full) and --dump-outputs: the plain run carries the contract's keys and nothing that takes runs of
its own; the dumped block is the last timed step's output, bounded in size, and the same launch on the same seeded input."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def test_dump_outputs_writes_small_blocks_whole(tmp_path):
    import torch

    import bench

    out = torch.arange(10 * 98 * 13, dtype=torch.float32).reshape(10, 98, 13)
    bench.dump_outputs(torch, str(tmp_path / "d"), "mfcc", out)
    got = np.load(tmp_path / "d" / "mfcc.npy")
    assert got.dtype == np.float32
    np.testing.assert_array_equal(got, out.numpy())


def test_dump_outputs_samples_large_blocks_by_seeded_clips(tmp_path):
    import torch

    import bench

    clips = 13000  # 13000 x 98 x 13 float32 = 66.2 MB: above the 64 MB bound
    out = torch.arange(clips, dtype=torch.float32)[:, None, None] + torch.zeros(clips, 98, 13)
    for d in ("a", "b"):
        bench.dump_outputs(torch, str(tmp_path / d), "mfcc", out)
    a, b = np.load(tmp_path / "a" / "mfcc.npy"), np.load(tmp_path / "b" / "mfcc.npy")
    np.testing.assert_array_equal(a, b)  # the same clips on every run
    assert a.dtype == np.float32 and a.shape[1:] == (98, 13) and a.nbytes <= bench.DUMP_MAX_BYTES
    assert a.shape[0] == bench.DUMP_MAX_BYTES // (98 * 13 * 4)
    want = np.sort(np.random.default_rng(0).choice(clips, a.shape[0], replace=False))
    np.testing.assert_array_equal(a[:, 0, 0], want.astype(np.float32))  # whole clips, in clip order


@pytest.mark.gpu
def test_plain_line_and_dumped_outputs(tmp_path, oracle):
    """`bench.py --gpus 1 --steps 20 --warmup 5 --dump-outputs DIR`: the contract's keys, ms_per_step of the 20 timed steps, no CPU
    baseline / clock / board / stored profile / secondary legs; DIR/mfcc.npy is the last step's block, equal bit for bit to one
    more launch of the same build on the same seeded input batch, and within RTOL of the oracle on sampled clips."""
    import ctypes as C

    import torch

    import bench
    from common import BENCH_KERNELS, RTOL, rel
    from speechsauce_amd import SpeechConfig, _lib, make_params

    steps, warmup = 20, 5
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup),
                        "--dump-outputs", str(tmp_path / "out")], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["metric"] == "mfcc_frames_per_sec" and d["unit"] == "frames/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
    assert d["n_gpus"] == 1 and d["steps"] == steps and d["warmup"] == warmup and d["value"] > 1e9
    frames_per_step = 1024 * 98
    assert abs(d["value"] * d["ms_per_step"] * 1e-3 - frames_per_step) < 1e-6 * frames_per_step
    for k in ("secondary", "value_pipelined", "pipelined", "cpu_baseline", "cpu_baseline_all_cores"):
        assert k not in d, k
    r = d["roofline"]
    assert r["kernel"].encode() == BENCH_KERNELS["cfg2"] and r["algorithmic_bytes_per_launch"] == 70754304
    for k in ("clock_ghz_measured", "board", "traffic", "cycles_per_launch"):
        assert k not in r, k

    got = np.load(tmp_path / "out" / "mfcc.npy")
    assert got.dtype == np.float32 and got.shape == (1024, 98, 13) and np.isfinite(got).all()
    # the last timed step read batch (steps - 1) % n_buf of bench.py's ring, seeded 1 + i (rank 0)
    n_buf = max(2, -(-300 * 2**20 // (4 * 1024 * 16000)))
    x = bench.synth_batch(torch, 1024, 16000, 1 + (steps - 1) % n_buf, torch.device("cuda", 0))
    cfg = SpeechConfig(make_params(sample_rate=16000))
    o = torch.empty((1024, 98, 13), dtype=torch.float32, device="cuda:0")
    lib = _lib.lib()
    _lib.check(lib.ss_mfcc_batch_device(cfg.handle, x.data_ptr(), 1024, 16000, 16000, o.data_ptr(),
                                        C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    assert lib.ss_last_kernel_name() == BENCH_KERNELS["cfg2"]
    np.testing.assert_array_equal(got, o.cpu().numpy())
    xh = x.cpu().numpy()
    op = oracle.make_params(sample_rate=16000)
    for b in (0, 511, 1023):
        assert rel(got[b], oracle.mfcc(op, xh[b])) <= RTOL, b
