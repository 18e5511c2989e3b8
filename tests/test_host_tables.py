"""Host-side table builders under AddressSanitizer + UBSan (CPU only): tools/hosttest/fuzz_tables.cpp builds the LDS blocks of
every kernel for pseudo-random valid configurations and checks that each filter's weights reach exactly one (slot, lane) bit
for bit, that no lane reads past its P row and that the cosine rows are the host DCT table in the kernel's layout -- and, for
pseudo-random valid ss_kaldi_params, the same of the Kaldi front end's block with its appended window.  Its --digest
mode (one line of flags, sizes and a hash of the table bytes per block: what two builds of ss_host.cpp are compared by) runs here
too, twice, so that it stays buildable, clean under the sanitizers and deterministic."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_table_builders_sanitized(tmp_path):
    exe = str(tmp_path / "fuzz_tables")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "include"),
           "-I" + os.path.join(ROOT, "mfcc-rust_amd", "csrc"), os.path.join(ROOT, "tools", "hosttest", "fuzz_tables.cpp"),
           os.path.join(ROOT, "mfcc-rust_amd", "csrc", "ss_host.cpp"), "-o", exe]
    subprocess.run(cmd, check=True, timeout=300)
    for seed in ("12345", "777"):
        r = subprocess.run([exe, "1000", seed], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
        assert "all checks passed" in r.stdout
    digests = [subprocess.run([exe, "--digest", "60", "12345"], capture_output=True, text=True, timeout=300) for _ in range(2)]
    for r in digests:
        assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert digests[0].stdout and digests[0].stdout == digests[1].stdout
    # the named configurations and the random ones, ten blocks each, none rejected by build_tables; then the Kaldi front end's block,
    # one line for each of its random configurations
    assert digests[0].stdout.count("\n") >= 11 * 60 and " fnv " in digests[0].stdout
    assert digests[0].stdout.count("| kaldi512 ok 1 ") >= 60 and "| kaldi512 ok 0 " not in digests[0].stdout
