"""The action rule on the CPU (include/wab.h, WAB_HAS_ACTION_RULE): the header and its ctypes
mirror, check_action_rule's refusals, select_reference's greedy ties and its sample mode, and
reference_forward's temperature."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import action_rule_cases as arc
import policy_cases as pc
from wab_gym_amd import _lib, policy

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "wab.h")


def test_header_declares_the_rule_and_keeps_the_abi():
    src = open(HEADER).read()
    assert re.search(r"^#define WAB_HAS_ACTION_RULE 1\b", src, flags=re.M)
    assert re.search(r"enum\s*\{\s*WAB_ACT_SAMPLE = 0,\s*WAB_ACT_GREEDY = 1\s*\}", src)
    abi = int(re.search(r"^#define WAB_ABI_VERSION (\d+)", src, flags=re.M).group(1))
    assert abi == _lib.ABI_VERSION == 14
    flat = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\bint\s+wab_policy_set_action_rule\s*\(\s*wab_policy\*\s*p,\s*const wab_action_rule\*\s*rule\s*\)\s*;",
                     flat)
    assert re.search(r"\bint\s+wab_policy_get_action_rule\s*\(\s*const wab_policy\*\s*p,\s*wab_action_rule\*\s*out\s*\)\s*;",
                     flat)
    for name in ("wab_policy_set_action_rule", "wab_policy_get_action_rule"):
        assert name in _lib.EXPORTED
    assert _lib.ACTION_MODE == {"sample": 0, "greedy": 1}


def test_the_struct_is_eight_bytes():
    assert ctypes.sizeof(_lib.WabActionRule) == 8
    assert _lib.WabActionRule.mode.offset == 0 and _lib.WabActionRule.temperature.offset == 4


@pytest.mark.parametrize("tau", [0, -1, float("nan"), float("inf"), -float("inf"), 1e39, 1e-39, 3e38])
def test_check_action_rule_refuses_the_temperature(tau):
    """0, negative, NaN, inf; and a float32 reciprocal that is inf (1e-39, a subnormal float32),
    of a temperature that is itself inf in float32 (1e39), or subnormal (3e38: 1 / 3e38 < 2^-126)."""
    with pytest.raises(ValueError, match="temperature"):
        policy.check_action_rule("sample", tau)
    with pytest.raises(ValueError, match="temperature"):
        policy.check_action_rule("greedy", tau)


def test_check_action_rule_refuses_an_unknown_mode():
    for mode in ("argmax", "", None, 1, "GREEDY"):
        with pytest.raises(ValueError, match="mode"):
            policy.check_action_rule(mode, 1.0)


def test_check_action_rule_returns_the_float32_reciprocal():
    assert policy.check_action_rule("sample", 1.0) == (0, np.float32(1.0), np.float32(1.0))
    assert policy.check_action_rule("greedy", 0.5) == (1, np.float32(0.5), np.float32(2.0))
    m, tau, inv = policy.check_action_rule("greedy", 0.7)
    assert tau.dtype == np.float32 and inv.dtype == np.float32
    assert inv == np.float32(1.0) / np.float32(0.7) and m == 1
    # the largest and smallest temperatures whose reciprocal is still a normal float32
    policy.check_action_rule("sample", 2.0 ** 126)
    policy.check_action_rule("sample", 2.0 ** -126)
    with pytest.raises(ValueError):
        policy.check_action_rule("sample", 2.0 ** 127)  # 1 / t = 2^-127: subnormal


def greedy(p):
    B = len(p)
    z = np.zeros(B, np.int64)
    return policy.select_reference(np.asarray(p, np.float32), pc.SEED, np.arange(B), z, z, "greedy")


def test_select_reference_greedy_ties_go_to_the_lowest_index():
    assert greedy([[0.1, 0.4, 0.1, 0.4, 0.0]]).tolist() == [1]      # a two-way tie at the top
    assert greedy([[0.4, 0.1, 0.1, 0.4, 0.0]]).tolist() == [0]
    assert greedy([[0.2] * 5]).tolist() == [0]                      # all equal
    assert greedy([[1.0 / 6] * 6]).tolist() == [0]
    assert greedy([[np.nan] * 5]).tolist() == [0]                   # a row of NaNs
    assert greedy([[0.0, 0.0, 0.0, 0.0, 1.0], [0.0, 0.3, 0.7, 0.0, 0.0]]).tolist() == [4, 2]
    # a NaN never compares greater, and nothing compares greater than a NaN that is `best`
    assert greedy([[0.1, np.nan, 0.5, 0.2, 0.2]]).tolist() == [2]
    assert greedy([[np.nan, 0.5, 0.1, 0.2, 0.2]]).tolist() == [0]
    out = greedy([[0.25, 0.75]])
    assert out.dtype == np.int8 and out.tolist() == [1]


def test_select_reference_greedy_is_the_first_maximum_of_the_spread_nets():
    for which in ("ref", "odd", "wide"):
        x = arc.FEATURES[which]()
        sd = arc.spread(which)
        assert arc.assert_reference_spreads(sd, x) == arc.ARGMAX_COUNTS[which]
        p32 = policy.reference_forward(sd, x)[0].numpy().astype(np.float32)
        assert np.array_equal(greedy(p32), arc.first_max(p32))


def test_select_reference_sample_mode_is_sample_reference():
    x = pc.ref_features(257)
    p32 = policy.reference_forward(arc.spread("ref"), x)[0].numpy().astype(np.float32)
    rng = np.random.RandomState(3)
    ids, ep, tu = np.arange(257) + 1000, rng.randint(0, 9, size=257), rng.randint(0, 5, size=257)
    want = policy.sample_reference(p32, pc.SEED, ids, ep, tu)
    assert np.array_equal(policy.select_reference(p32, pc.SEED, ids, ep, tu), want)
    assert np.array_equal(policy.select_reference(p32, pc.SEED, ids, ep, tu, mode="sample"), want)
    assert len(set(want.tolist())) >= 3
    with pytest.raises(ValueError, match="mode"):
        policy.select_reference(p32, pc.SEED, ids, ep, tu, mode="argmax")
    for mode in ("sample", "greedy"):
        with pytest.raises(ValueError, match="float32"):
            policy.select_reference(p32.astype(np.float64), pc.SEED, ids, ep, tu, mode=mode)


def test_reference_forward_temperature():
    """temperature=1.0 is the call without it, bit for bit; 0.5 is the net with action_head
    doubled, exactly (a factor 2 is exact in bf16 and in every float64 sum); the value never
    moves."""
    for which in ("ref", "odd"):
        sd, x = arc.spread(which), arc.FEATURES[which]()
        p, v = policy.reference_forward(sd, x)
        p1, v1 = policy.reference_forward(sd, x, temperature=1.0)
        assert torch.equal(p, p1) and torch.equal(v, v1)
        ph, vh = policy.reference_forward(sd, x, temperature=0.5)
        pd, vd = policy.reference_forward(arc.doubled_head(sd), x)
        assert torch.equal(ph, pd) and torch.equal(vh, v) and torch.equal(vd, v)
        assert not torch.equal(ph, p)
        # a general temperature scales the logits by the float32 reciprocal, in float64
        pt, vt = policy.reference_forward(sd, x, temperature=0.7)
        inv = float(np.float32(1.0) / np.float32(0.7))
        lg = torch.log(p) * inv
        want = torch.softmax(lg, dim=-1)
        assert float((pt - want).abs().max()) < 1e-12 and torch.equal(vt, v)


def test_tie_nets_tie_in_the_reference():
    for which in ("ref", "odd", "wide"):
        x = arc.FEATURES[which]()
        p = policy.reference_forward(arc.tie_net(which, "all"), x)[0].numpy()
        assert (p == p[:, :1]).all()
        p = policy.reference_forward(arc.tie_net(which, "pair"), x)[0].numpy()
        assert (p[:, 1] == p[:, 3]).all() and np.delete(p, [1, 3], axis=1).max() < 1e-3 and p[:, 1].min() > 0.49
