"""The argument-block builders of mfcc-rust_amd/csrc/ss_launch_args.h under AddressSanitizer + UBSan (CPU only):
tools/hosttest/test_launch_args.cpp includes that header and compares, for every builder and every flavour of call site (dense
MFCC / mfe / power, streaming with pad_mode = reflect, packed, pool; mel from the 2048 / 1024 / 4096-point tables; stft output; the
256-point and the wide-bank 512-point family), the block the builder returns with one written out field by field as the call
sites wrote theirs before the builders existed -- memcmp over the whole struct, distinct values in every table and FrontArgs
field -- and dct_scales bit for bit against its three formulas.  A stand-alone host program: nothing is loaded into Python and
nothing touches a GPU (the header pulls in ss_device.h, so the compiler is hipcc in host-only mode)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)


@pytest.mark.skipif(HIPCC is None, reason="needs hipcc")
def test_launch_args_sanitized(tmp_path):
    exe = str(tmp_path / "test_launch_args")
    cmd = [HIPCC, "--offload-host-only", "-x", "hip", "-std=c++17", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "mfcc-rust_amd", "csrc"),
           os.path.join(ROOT, "tools", "hosttest", "test_launch_args.cpp"), "-o", exe]
    subprocess.run(cmd, check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "all checks passed" in r.stdout
