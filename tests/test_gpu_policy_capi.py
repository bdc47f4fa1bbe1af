"""The closed loop with no Python in the process: examples/c_api_policy_demo (a C++ host program
linked to libwab_hip.so) runs 200 envs for 20 steps of wab_policy_act + wab_step_features and
checks every action against the sampling rule of its probs row and keyed draw itself."""
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEMO = os.path.join(REPO, "examples", "bin", "c_api_policy_demo")


@pytest.mark.gpu
def test_c_caller_steps_a_closed_loop():
    if not os.path.exists(DEMO):
        pytest.fail("examples/bin/c_api_policy_demo not built (__graft_entry__.build())")
    r = subprocess.run([DEMO], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1 and lines[0].startswith("OK "), r.stdout
