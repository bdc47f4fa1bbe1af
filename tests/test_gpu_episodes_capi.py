"""Episode statistics and normalisation through the C-ABI without Python in the process:
examples/c_api_episodes_demo (a C++ host program linked to libwab_hip.so) runs a hand-made segment
through wab_episode_stats_update in two calls, with and without a handle, a count-only call and
wab_normalize_episode_returns, and compares everything with the same arithmetic on the host."""
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEMO = os.path.join(REPO, "examples", "bin", "c_api_episodes_demo")


@pytest.mark.gpu
def test_c_caller_of_the_episode_functions():
    if not os.path.exists(DEMO):
        pytest.fail("examples/bin/c_api_episodes_demo not built (__graft_entry__.build())")
    r = subprocess.run([DEMO], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("OK: 45 x 150 segment in two calls"), r.stdout
