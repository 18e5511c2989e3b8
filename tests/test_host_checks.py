"""The table and pool rules of mfcc-rust_amd/csrc/ss_host_checks.h under AddressSanitizer + UBSan (CPU only):
tools/hosttest/test_host_checks.cpp includes that header, supplies ss::fail and compares every message as an exact string -- the
slot rule (empty, single, duplicate in the last position, -1, == pool_streams, INT32_MAX, a permutation of the whole pool), the
clip table and the pool's row offsets (a bad first offset, a decrease, two clips past total_rows of which the first is named, empty
clips, the last offset == total_rows), ranges_overlap at its boundaries, and the pool-row gather / scatter bit for bit (6 rows,
slots {2, 0, 5}, NaN payloads, len 4, 1 and 0: exactly the named rows change).  A stand-alone host program: nothing is loaded into
Python and nothing touches a GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_host_checks_sanitized(tmp_path):
    exe = str(tmp_path / "test_host_checks")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "mfcc-rust_amd", "csrc"),
           os.path.join(ROOT, "tools", "hosttest", "test_host_checks.cpp"), "-o", exe]
    subprocess.run(cmd, check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "all checks passed" in r.stdout
