"""The host-pointer calls' stager of mfcc-rust_amd/csrc/ss_host_stage.h under AddressSanitizer + UBSan (CPU only):
tools/hosttest/test_host_stage.cpp runs HostStageT over a malloc-backed backend that logs every call and fails its k-th one.  A packed
call (3 clips, one empty, 3 columns, a table that ends below total_rows) and a pool call (6 rows, slots {2, 0, 5}, len 4 and 0) are
held to their exact call logs -- counts, sizes, directions, a zero-byte item allocates 16 bytes and copies nothing -- and then failed
at every k in turn: the first failure's status and message as exact strings ("host staging: ..", "<name>: device error",
"hipMemcpy D2H: ..", "hipMemcpy D2H (pool rows): .."), nothing but frees after it, the caller's output and pool bit-identical (NaN
payloads) and every block freed (the leak check).  A stand-alone host program: nothing is loaded into Python and nothing touches a
GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_host_stage_sanitized(tmp_path):
    exe = str(tmp_path / "test_host_stage")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "mfcc-rust_amd", "csrc"),
           os.path.join(ROOT, "tools", "hosttest", "test_host_stage.cpp"), "-o", exe]
    subprocess.run(cmd, check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "all checks passed" in r.stdout
