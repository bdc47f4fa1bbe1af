"""wab_gae and wab_whiten through the C-ABI without Python in the process:
examples/c_api_gae_demo (a C++ host program linked to libwab_hip.so) runs a hand-made segment
through wab_gae with and without a handle, with and without last_value and with one output alone,
then whitens the advantages, and compares everything with the same arithmetic on the host."""
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEMO = os.path.join(REPO, "examples", "bin", "c_api_gae_demo")


@pytest.mark.gpu
def test_c_caller_of_the_advantage_functions():
    if not os.path.exists(DEMO):
        pytest.fail("examples/bin/c_api_gae_demo not built (__graft_entry__.build())")
    r = subprocess.run([DEMO], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("OK: 37 x 300 segment, advantages and targets equal the host's contract"), r.stdout
