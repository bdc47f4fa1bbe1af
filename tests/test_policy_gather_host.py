"""Rows gathered by an index (wab_policy_grad_gather, wab_policy_grad_ppo_gather,
wab_policy_evaluate_gather, wab_policy_grad_bad_rows) on the CPU: the header and its mirror, the
checks of an index that need no device, and the contract with rows= (reference_loss_and_grad,
reference_ppo_loss_and_grad): the same function on gathered copies, exactly; an index outside the
source is the clamped source row with action -1."""
import os
import re

import numpy as np
import pytest
import torch

import policy_grad_cases as pgc
import ppo_cases as ppc
from wab_gym_amd import _lib, policy

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "wab.h")
GATHER = {"wab_policy_grad_gather": "wab_policy_grad", "wab_policy_grad_ppo_gather": "wab_policy_grad_ppo",
          "wab_policy_evaluate_gather": "wab_policy_evaluate"}
M = 300


def header_args(src, name):
    """The parameter list of `int name(...);` in the header, split at its commas."""
    m = re.search(r"\bint\s+%s\(([^;]*?)\);" % name, src, re.S)
    assert m, name
    return [a.strip() for a in m.group(1).split(",")]


def test_header_declares_the_gather_calls_and_the_mirror_follows():
    src = open(HEADER).read()
    assert re.search(r"^#define\s+WAB_HAS_POLICY_GATHER\s+1\s*$", src, re.M)
    version = int(re.search(r"#define\s+WAB_ABI_VERSION\s+(\d+)", src).group(1))
    assert version == _lib.ABI_VERSION
    for name, plain in GATHER.items():
        args, base = header_args(src, name), header_args(src, plain)
        # the contiguous call's arguments, then the index and the source's length
        assert [re.sub(r"\s+", " ", a) for a in args[:len(base)]] == [re.sub(r"\s+", " ", a) for a in base], name
        assert args[len(base):] == ["const int32_t* rows", "int64_t M"], name
        assert name in _lib.EXPORTED
    assert header_args(src, "wab_policy_grad_bad_rows") == header_args(src, "wab_policy_grad_bad_actions")
    assert "wab_policy_grad_bad_rows" in _lib.EXPORTED
    # the mirror's argtypes, read from _lib.load()'s own text: no library is needed for this
    text = open(_lib.__file__).read()
    counts = {"wab_policy_grad": 15, "wab_policy_grad_ppo": 20, "wab_policy_evaluate": 10}
    for name, plain in GATHER.items():
        assert len(header_args(src, plain)) == counts[plain]
        assert len(header_args(src, name)) == counts[plain] + 2
        assert re.search(r"L\.%s\.argtypes = L\.%s\.argtypes \+ \[P, I64\]" % (name, plain), text), name
    assert re.search(r"L\.wab_policy_grad_bad_rows\.argtypes = \[P, P, P, P\]", text)


def test_check_row_index_accepts_and_refuses():
    cpu = torch.device("cpu")
    perm = torch.randperm(40, dtype=torch.int32)
    assert policy.check_row_index(perm, cpu) == 40
    assert policy.check_row_index(perm.to(torch.int64), cpu) == 40
    assert policy.check_row_index(perm[8:24], cpu) == 16  # a slice of a permutation
    assert policy.check_row_index(perm[:0], cpu) == 0
    refused = {
        "int32": perm.float(),
        "1-d": perm.view(5, 8),
        "contiguous": perm[::2],
        "device": perm.to("meta"),
        "tensor": [0, 1, 2],
    }
    for word, rows in refused.items():
        with pytest.raises(ValueError, match=word):
            policy.check_row_index(rows, cpu)
    with pytest.raises(ValueError, match="device"):
        policy.check_row_index(perm, torch.device("meta"))


def index(n, seed=3):
    """A permutation prefix of the M source rows with one duplicate."""
    r = np.random.RandomState(seed).permutation(M)[:n].astype(np.int64)
    r[n // 2] = r[0]
    return r


def same(got, want):
    for k in pgc.GRAD_NAMES:
        assert torch.equal(got["grads"][k], want["grads"][k]), k
    for g, w in zip(got["loss"], want["loss"]):
        assert float(g) == float(w)
    for k in ("logp", "value", "entropy") + (("ratio", "clipped", "value_clipped") if "ratio" in want else ()):
        assert torch.equal(got[k], want[k]), k
    if "ppo" in want:
        assert [float(x) for x in got["ppo"]] == [float(x) for x in want["ppo"]]


@pytest.mark.parametrize("net", ("ref", "odd"))
def test_reference_with_rows_is_the_reference_on_gathered_copies(net):
    sd, c = pgc.state_dict(net), ppc.case(net, M)
    r = index(129)
    kw = dict(clip=ppc.CLIP, value_clip=ppc.VALUE_CLIP, value_coef=0.5, entropy_coef=0.01)
    got = policy.reference_ppo_loss_and_grad(sd, c["x"], c["a"], c["adv"], c["t"], c["old_logp"],
                                             old_value=c["old_value"], rows=r, **kw)
    want = policy.reference_ppo_loss_and_grad(sd, c["x"][r], c["a"][r], c["adv"][r], c["t"][r], c["old_logp"][r],
                                              old_value=c["old_value"][r], **kw)
    same(got, want)
    assert got["logp"].shape == (129,) and float(got["ppo"][3]) > 0
    # a [T, B, F] source is its [T B, F] rows
    T = 3
    got3 = policy.reference_ppo_loss_and_grad(
        sd, c["x"].reshape(T, M // T, -1), c["a"].reshape(T, -1), c["adv"].reshape(T, -1), c["t"].reshape(T, -1),
        c["old_logp"].reshape(T, -1), old_value=c["old_value"].reshape(T, -1), rows=torch.as_tensor(r, dtype=torch.int32),
        **kw)
    same(got3, want)
    a2c = policy.reference_loss_and_grad(sd, c["x"], c["a"], c["adv"], c["t"], 0.5, 0.01, rows=r)
    same(a2c, policy.reference_loss_and_grad(sd, c["x"][r], c["a"][r], c["adv"][r], c["t"][r], 0.5, 0.01))


@pytest.mark.parametrize("net", ("ref", "odd"))
def test_a_bad_index_is_the_clamped_source_row_with_action_minus_one(net):
    sd, c = pgc.state_dict(net), ppc.case(net, M)
    r = index(129)
    places, values = (0, 64, 127, 128), (-1, M, 2 ** 31 - 1, -2 ** 31)
    bad = r.copy()
    bad[list(places)] = values
    clamped = np.clip(bad, 0, M - 1)
    a = c["a"][clamped].copy()
    a[list(places)] = -1
    kw = dict(clip=ppc.CLIP, value_clip=ppc.VALUE_CLIP, value_coef=0.5, entropy_coef=0.01)
    got = policy.reference_ppo_loss_and_grad(sd, c["x"], c["a"], c["adv"], c["t"], c["old_logp"],
                                             old_value=c["old_value"], rows=bad, **kw)
    want = policy.reference_ppo_loss_and_grad(sd, c["x"][clamped], a, c["adv"][clamped], c["t"][clamped],
                                              c["old_logp"][clamped], old_value=c["old_value"][clamped], **kw)
    same(got, want)
    # left out: logp = ratio = 0, value and entropy the clamped row's, and the sums those of the other rows
    rest = np.setdiff1d(np.arange(129), places)
    clean = policy.reference_ppo_loss_and_grad(sd, c["x"][clamped], c["a"][clamped], c["adv"][clamped], c["t"][clamped],
                                               c["old_logp"][clamped], old_value=c["old_value"][clamped], **kw)
    for i in places:
        assert float(got["logp"][i]) == 0.0 and float(got["ratio"][i]) == 0.0
        assert float(got["value"][i]) == float(clean["value"][i]) and float(got["entropy"][i]) == float(clean["entropy"][i])
    assert torch.equal(got["logp"][rest], clean["logp"][rest]) and torch.equal(got["ratio"][rest], clean["ratio"][rest])
    only = policy.reference_ppo_loss_and_grad(sd, c["x"][clamped][rest], c["a"][clamped][rest], c["adv"][clamped][rest],
                                              c["t"][clamped][rest], c["old_logp"][clamped][rest],
                                              old_value=c["old_value"][clamped][rest], **kw)
    assert float(got["ppo"][0]) == float(only["ppo"][0]) and float(got["ppo"][2]) == float(only["ppo"][2])
    for g, w in zip(got["loss"][:3], only["loss"][:3]):
        assert abs(float(g) - float(w)) <= 1e-12 * max(1.0, abs(float(w)))
    for k in pgc.GRAD_NAMES:
        assert float((got["grads"][k] - only["grads"][k]).abs().max()) <= 1e-12 * max(1.0, float(only["grads"][k].abs().max())), k
