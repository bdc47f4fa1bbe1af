"""wab_rollout_policy's surface without a GPU: the header declares the two entry points, the
ctypes mirror exports them under the same ABI version, and PragmaticObsWrapper.rollout_policy
has the documented options."""
import inspect
import os
import re

from wab_gym_amd import _lib
from wab_gym_amd.wrappers import PragmaticObsWrapper

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "wab.h")


def header_text():
    with open(HEADER) as f:
        return f.read()


def test_header_declares_the_two_entry_points():
    src = re.sub(r"/\*.*?\*/", "", header_text(), flags=re.S)
    assert re.search(r"\bint\s+wab_rollout_policy_fused\s*\(\s*const\s+wab_handle\s*\*\s*\w+\s*,\s*const\s+wab_policy\s*\*", src)
    m = re.search(r"\bint\s+wab_rollout_policy\s*\(([^;]*)\)\s*;", src)
    assert m, "wab_rollout_policy is not declared"
    args = [a.strip() for a in m.group(1).split(",")]
    names = [re.split(r"[\s*]+", a)[-1] for a in args]
    assert names == ["h", "p", "features0", "T", "obs_seq", "actions", "value", "probs", "reward", "done", "features",
                     "features_last", "gamma", "bootstrap", "returns", "stream"]


def test_both_are_exported_by_the_ctypes_mirror():
    assert "wab_rollout_policy" in _lib.EXPORTED
    assert "wab_rollout_policy_fused" in _lib.EXPORTED


def test_abi_version_of_header_and_mirror_agree():
    m = re.search(r"#define\s+WAB_ABI_VERSION\s+(\d+)", header_text())
    assert m and int(m.group(1)) == _lib.ABI_VERSION
    assert _lib.ABI_VERSION >= 8  # the version that added wab_rollout_policy


def test_rollout_policy_signature():
    sig = inspect.signature(PragmaticObsWrapper.rollout_policy)
    assert list(sig.parameters)[:3] == ["self", "policy", "T"]
    want = {"gamma": 0.99, "store_planes": False, "store_features": True, "return_probs": False, "fused": None}
    for name, default in want.items():
        assert name in sig.parameters, name
        got = sig.parameters[name].default
        assert got == default and type(got) is type(default), (name, got)
