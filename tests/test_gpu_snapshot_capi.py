"""Snapshots with no Python in the process: examples/c_api_snapshot_demo (a C++ host program linked
to libwab_hip.so) saves 128 envs after 20 steps, replays the next 30 steps after a rewind in the
same handle and again in two fresh handles of 64 envs restored from a host copy of the records,
and compares every output byte for byte itself."""
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEMO = os.path.join(REPO, "examples", "bin", "c_api_snapshot_demo")


@pytest.mark.gpu
def test_c_caller_rewinds_and_resumes():
    if not os.path.exists(DEMO):
        pytest.fail("examples/bin/c_api_snapshot_demo not built (__graft_entry__.build())")
    r = subprocess.run([DEMO], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1 and lines[0].startswith("OK "), r.stdout
