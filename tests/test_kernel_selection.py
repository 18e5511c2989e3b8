"""Which kernel serves which call, pinned: tools/selection_census.py makes one tiny call per (configuration, entry point, sample
type) through the device-pointer C ABI -- fft_points 256 / 512 / 1024 / 2048 / 4096 and a chirp-z length; at 512 the wide bank, the
frame window, fused pre-emphasis, centred frames with either pad mode, a bank up to fs/2 and the ortho DCT; at 2048 a channel count
on each side of the eight / twelve-wave rule; mfcc, mfe, power spectrum, mel and stft in their dense, packed, dense-stream and pool
forms, float and 16-bit PCM, and the two *_batches_device calls with 2 and 9 batches -- and records ss_last_kernel_name() (or the
status and message of a call the API rejects).  tests/golden/kernel_selection.json is that census on an MI355X from before the
launchers of ss_api.hip were folded onto shared argument builders and one candidate step; the census must still read the same, case
by case."""
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_kernel_selection_matches_the_fixture(sslib):
    spec = importlib.util.spec_from_file_location("selection_census", os.path.join(ROOT, "tools", "selection_census.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    with open(os.path.join(ROOT, "tests", "golden", "kernel_selection.json")) as f:
        want = json.load(f)
    got = tool.census(sslib)
    assert sorted(got) == sorted(want), "the configurations of the census and of the fixture differ"
    bad = []
    for name in sorted(want):
        for case in sorted(set(want[name]) | set(got[name])):
            w, g = want[name].get(case, "<no such case>"), got[name].get(case, "<no such case>")
            if w != g:
                bad.append(f"{name} / {case}: fixture {w!r}, now {g!r}")
    assert not bad, "\n".join(bad)
    assert sum(len(v) for v in want.values()) > 400  # (the fixture is the whole census, not a stub)
