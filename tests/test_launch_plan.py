"""The launch arithmetic of mfcc-rust_amd/csrc/ss_launch_plan.h under AddressSanitizer + UBSan (CPU only):
tools/hosttest/test_launch_plan.cpp includes that header alone and checks that the multiply-high reciprocal of n_frames divides
exactly (every d in 2..4096, a few thousand random d < 2^31, x at the edges of the quotient steps and at random), that the
CU-capped grid and the unit split keep their invariants, that the quad_src address-range test flips at its three boundaries and
that the plans of the headline shapes are the literal ones worked out by hand.  It also includes ss_quad256.h, whose host part is
the quad kernels' frame locate and launch plan: locate_frame against plain division for groups of 4 and 8 frames at and next to
the clip boundaries, with the reciprocal exactly where plan_groups enables it."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_launch_plan_sanitized(tmp_path):
    exe = str(tmp_path / "test_launch_plan")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I" + os.path.join(ROOT, "mfcc-rust_amd", "csrc"), os.path.join(ROOT, "tools", "hosttest", "test_launch_plan.cpp"), "-o", exe]
    subprocess.run(cmd, check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "all checks passed" in r.stdout
