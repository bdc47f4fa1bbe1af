"""The device policy's references on the CPU (wab_gym_amd/policy.py): reference_forward on a net
small enough to follow by hand, sample_reference against the keyed RNG's definition, and E_bf16,
what the bf16 contract costs against a stock fp32 forward on the GPU test's own inputs."""
import math

import numpy as np
import pytest
import torch

import policy_cases as pc
from wab_gym_amd import policy


def test_reference_forward_by_hand():
    """A 2-2-2-2 net, A = 2.  x = (1, 0.5):
    layer 1: z = (1 + 1 + 0.5, -1 - 1) = (2.5, -2); leaky (2.5, -2 * 0.01f); bf16 (2.5, -0.02001953125)
             (0.02 = 1.28 * 2^-6; 1.28 * 128 = 163.84 -> 164 / 128 * 2^-6);
    layer 2: z = (2 * 2.5, 100 * -0.02001953125) = (5, -2.001953125); leaky, bf16 (5, -0.02001953125);
    layer 3: z = (5, -100 * 5) = (5, -500); leaky (5, -5 (just above)); clamp (4, -4): both limits;
    heads: logits 0.25 * (4, -4) = (1, -1): probs (e^2, 1) / (1 + e^2); value 0.5 * 4 + 0.25 * -4 + 1 = 2."""
    sd = {"affine1.weight": [[1.0, 2.0], [-1.0, -2.0]], "affine1.bias": [0.5, 0.0],
          "affine2.weight": [[2.0, 0.0], [0.0, 100.0]], "affine2.bias": [0.0, 0.0],
          "affine3.weight": [[1.0, 0.0], [-100.0, 0.0]], "affine3.bias": [0.0, 0.0],
          "action_head.weight": [[0.25, 0.0], [0.0, 0.25]], "action_head.bias": [0.0, 0.0],
          "value_head.weight": [[0.5, 0.25]], "value_head.bias": [1.0]}
    sd = {k: torch.tensor(v, dtype=torch.float32) for k, v in sd.items()}
    assert policy.shape_of(sd) == (2, 2, 2, 2, 2)
    hidden = []
    probs, value = policy.reference_forward(sd, torch.tensor([[1.0, 0.5]]), hidden=hidden)
    assert probs.dtype == torch.float64 and value.dtype == torch.float64
    slope = float(np.float32(0.01))
    assert hidden[0][0].tolist() == [[2.5, -2.0]]
    assert hidden[0][1].tolist() == [[2.5, -0.02001953125]]
    assert hidden[1][0].tolist() == [[5.0, -2.001953125]]
    assert hidden[1][1].tolist() == [[5.0, -0.02001953125]]
    assert hidden[2][0].tolist() == [[5.0, -500.0]]
    assert -500.0 * slope < -4.0          # the negative slope takes -500 below the lower clamp limit
    assert hidden[2][1].tolist() == [[4.0, -4.0]]
    e2 = math.exp(2.0)
    assert probs[0].tolist() == pytest.approx([e2 / (1 + e2), 1 / (1 + e2)], abs=1e-15)
    assert value.tolist() == [2.0]


def test_reference_forward_rounds_inputs_and_weights_to_bf16():
    """1/3 as a feature and as a weight are used as bf16(1/3) = 0.333984375."""
    sd = {k: torch.zeros(s) for k, s in (("affine1.weight", (1, 1)), ("affine1.bias", (1,)),
                                         ("affine2.weight", (1, 1)), ("affine2.bias", (1,)),
                                         ("affine3.weight", (1, 1)), ("affine3.bias", (1,)),
                                         ("action_head.weight", (2, 1)), ("action_head.bias", (2,)),
                                         ("value_head.weight", (1, 1)), ("value_head.bias", (1,)))}
    sd["affine1.weight"][0, 0] = 1.0 / 3.0
    hidden = []
    policy.reference_forward(sd, torch.tensor([[1.0 / 3.0]]), hidden=hidden)
    assert hidden[0][0].item() == 0.333984375 * 0.333984375


def test_state_dict_checks():
    sd = dict(pc.weights("odd"))
    del sd["value_head.bias"]
    with pytest.raises(ValueError, match="value_head.bias"):
        policy.shape_of(sd)
    sd = dict(pc.weights("odd"))
    sd["affine2.weight"] = sd["affine2.weight"][:, :-1]
    with pytest.raises(ValueError, match="affine2.weight"):
        policy.shape_of(sd)


def test_sample_reference_is_the_keyed_draw_of_site_11():
    from oracle import keyed_rng

    assert policy.SITE_POLICY == 11
    taken = [v for k, v in vars(keyed_rng).items() if k.startswith("SITE_")]
    assert 11 not in taken and max(taken) == 10  # the first id free in the oracle's list
    rng = np.random.RandomState(3)
    n, A = 500, 5
    p = rng.dirichlet(np.ones(A), size=n).astype(np.float32)
    seed = 0xC0FFEE
    env = rng.randint(0, 1 << 40, size=n)
    ep = rng.randint(0, 1 << 31, size=n)
    turn = rng.randint(0, 200, size=n)
    u = np.array([keyed_rng.draw_u(keyed_rng.episode_key(seed, int(e), int(q)), 11, int(t), [0], [0], 0)[0]
                  for e, q, t in zip(env, ep, turn)])
    assert np.array_equal(policy.keyed_u(seed, env, ep, turn), u)
    want = np.zeros(n, np.int8)
    for i in range(n):
        c = 0.0
        for k in range(A - 1):
            c += float(p[i, k])
            want[i] += c <= u[i]
    got = policy.sample_reference(p, seed, env, ep, turn)
    assert got.dtype == np.int8 and np.array_equal(got, want)
    assert len(set(got.tolist())) == A
    # the boundaries: u below the first cumulative sum, and a cumulative sum equal to u
    assert policy.sample_reference(np.array([[1.0, 0.0]], np.float32), seed, [5], [0], [0])[0] == 0
    assert policy.sample_reference(np.array([[0.0, 1.0]], np.float32), seed, [5], [0], [0])[0] == 1
    with pytest.raises(ValueError):
        policy.sample_reference(p.astype(np.float64), seed, env, ep, turn)


@pytest.mark.parametrize("which", ["ref", "odd"])
def test_weights_reach_both_clamp_limits_and_negative_slopes(which):
    sd = pc.weights(which)
    feats = pc.ref_features(257) if which == "ref" else pc.odd_features(257)
    hidden = []
    policy.reference_forward(sd, feats, hidden=hidden)
    for z, _ in hidden:
        assert (z < 0).any() and (z > 0).any()
    assert (hidden[2][1] == 4.0).any() and (hidden[2][1] == -4.0).any()
    assert ((hidden[2][1] > -4.0) & (hidden[2][1] < 4.0)).any()


def test_contract_cost_E_bf16(capsys):
    """E_bf16 = max |reference_forward - stock fp32 torch forward with unrounded weights| over the
    GPU test's inputs: the yardstick of tests/test_gpu_policy.py (the kernel must stay within half
    of it).  Printed per case; DESIGN.md records the B = 257 figures."""
    rows = []
    for which in ("ref", "odd"):
        sd = pc.weights(which)
        for B in pc.BATCHES:
            feats = pc.ref_features(B) if which == "ref" else pc.odd_features(B)
            e_p, e_v = pc.contract_cost(sd, feats)
            rows.append((which, B, e_p, e_v))
            # bf16 keeps 8 bits: the cost is far above fp32 noise and far below the outputs' scale
            assert 1e-6 < e_p < 0.1 and 1e-6 < e_v < 0.5, (which, B, e_p, e_v)
    with capsys.disabled():
        for r in rows:
            print("E_bf16 net %-3s B %3d: probs %.3e value %.3e" % r)


@pytest.mark.parametrize("shape", list(pc.EXACT_SHAPES))
def test_exact_nets_hold_their_certificate(shape):
    """The exact-arithmetic nets of tests/test_gpu_policy.py: every fp32 sum of the forward pass is
    exact in any order and the float32 activation step gives the reference's bf16 values
    (pc.exact_certificate), every column and unit carries a weight, all numbers are small dyadic,
    and the reference alone has negative pre-activations in every hidden layer and units at both
    clamp limits."""
    sd = pc.exact_net(shape)
    assert policy.shape_of(sd) == shape
    for name in policy.LAYERS:
        w, b = sd[name + ".weight"], sd[name + ".bias"]
        assert bool((w != 0).any(dim=0).all()) and bool((w != 0).any(dim=1).all()), name
        for x in (w, b):
            assert torch.equal(x * 4, (x * 4).round()) and float(x.abs().max()) <= 448, name  # multiples of 1/4
        if name != "value_head":  # sparse: three picked columns and a unit's share of the columns nobody picked
            assert int((w != 0).sum(dim=1).max()) <= 3 + -(-w.shape[1] // w.shape[0]), name
    F = shape[0]
    x = pc.exact_features(257, F)
    assert x.min() >= 0 and x.max() <= 2 and np.array_equal(x * 8, np.round(x * 8))
    assert ((x != 0) & (x != 1)).any() and (x == 1).any() and (x == 0).any()
    for B in pc.EXACT_BATCHES:
        assert pc.exact_certificate(sd, pc.exact_features(B, F)) > 0
    hidden = []
    rp, _ = policy.reference_forward(sd, x, hidden=hidden)
    assert all(bool((z < 0).any()) for z, _ in hidden)
    assert bool((hidden[2][1] == 4.0).any()) and bool((hidden[2][1] == -4.0).any())
    assert float(rp.min()) > 1e-30  # every probability a normal float32, far from underflow


def test_exact_certificate_refuses_an_ordinary_net():
    """Random weights round in nearly every sum: the certificate must not pass them."""
    with pytest.raises(AssertionError):
        pc.exact_certificate(pc.weights("odd"), pc.odd_features(65))
    assert pc._low_bit_exponent(np.array([0.0, 1.0, 0.75, -96.0, 2.0 ** -20])).tolist() == [1 << 20, 0, -2, 5, -20]


def test_policy_still_exports_every_name_it_had():
    """The numeric contracts live in wab_gym_amd/policy_reference.py; policy.py re-exports them by
    name.  Every public name policy.py had before the split resolves on it, and each moved one is
    the very object of policy_reference.  Neither module imports torch when it is imported, and
    either can be the first of the two to be imported."""
    import subprocess
    import sys

    from wab_gym_amd import policy_reference

    kept = ["LAYERS", "SITE_POLICY", "ADAM_TENSORS", "shape_of", "check_rows", "check_row_index", "check_loss_args",
            "check_ppo_args", "check_adam_args", "adam_beta_powers", "adam_state_dict", "parse_adam_state_dict",
            "DevicePolicy", "DeviceAdam"]
    moved = ["reference_forward", "reference_loss_and_grad", "reference_ppo_loss_and_grad", "pair_tree_sum",
             "adam_fresh_state", "reference_adam_step", "keyed_u", "sample_reference"]
    for name in kept + moved:
        assert hasattr(policy, name), name
    for name in moved:
        assert getattr(policy, name) is getattr(policy_reference, name), name
        assert getattr(policy, name).__module__ == "wab_gym_amd.policy_reference", name
    for name in kept[3:]:  # (the functions and classes)
        assert getattr(policy, name).__module__ == "wab_gym_amd.policy", name
    assert policy_reference.adam_beta_powers is policy.adam_beta_powers
    for first, second in (("policy", "policy_reference"), ("policy_reference", "policy")):
        code = ("import sys; import wab_gym_amd.%s as a; import wab_gym_amd.%s as b; "
                "assert 'torch' not in sys.modules; assert a.keyed_u is b.keyed_u" % (first, second))
        subprocess.run([sys.executable, "-c", code], check=True, cwd=policy.__file__.rsplit("/", 2)[0])
