"""The action rule through the C-ABI alone (ctypes on libwab_hip.so, no DevicePolicy): the
refusals, each leaving the stored rule unchanged, the getter's round trip and the NULL rule;
examples/c_api_greedy_demo (wab.h only, no Python in the process) against the Python host on the
weights it dumps; and examples/evaluate_policy.py's evaluate()."""
import ctypes
import importlib.util
import os
import subprocess

import numpy as np
import pytest
import torch

import action_rule_cases as arc
import policy_cases as pc
from wab_gym_amd import _lib, policy
from wab_gym_amd.env import BatchedWolvesAndBushesEnv
from wab_gym_amd.wrappers import PragmaticObsWrapper

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEMO = os.path.join(REPO, "examples", "bin", "c_api_greedy_demo")
INVALID = -1  # WAB_E_INVALID


def get_rule(L, p):
    out = _lib.WabActionRule(-7, -7.0)
    assert L.wab_policy_get_action_rule(p, ctypes.addressof(out)) == 0
    return int(out.mode), float(out.temperature)


def set_rule(L, p, mode, tau):
    r = _lib.WabActionRule(mode, tau)
    return L.wab_policy_set_action_rule(p, ctypes.addressof(r))


def test_refusals_leave_the_rule_and_the_getter_round_trips():
    L = _lib.load()
    p = ctypes.c_void_p()
    shp = _lib.WabPolicyShape(449, 128, 150, 128, 5)
    assert L.wab_policy_create(ctypes.addressof(shp), 0, ctypes.byref(p)) == 0
    try:
        assert get_rule(L, p) == (0, 1.0)  # a fresh policy: {WAB_ACT_SAMPLE, 1.0f}, before any load
        assert set_rule(L, p, 1, 0.75) == 0
        assert get_rule(L, p) == (1, 0.75)
        ok = _lib.WabActionRule(0, 1.0)
        out = _lib.WabActionRule()
        assert L.wab_policy_set_action_rule(None, ctypes.addressof(ok)) == INVALID
        assert L.wab_policy_get_action_rule(None, ctypes.addressof(out)) == INVALID
        assert L.wab_policy_get_action_rule(p, None) == INVALID
        assert get_rule(L, p) == (1, 0.75)
        for mode in (2, -1, 1 << 20):
            assert set_rule(L, p, mode, 1.0) == INVALID and b"mode" in L.wab_last_error(), mode
            assert get_rule(L, p) == (1, 0.75)
        # 1e39 is inf as a float32; 1e-39 a subnormal whose reciprocal is inf; 3e38's is subnormal
        for tau in (0.0, -1.0, float("nan"), float("inf"), 1e39, 1e-39, 3e38):
            for mode in (0, 1):
                assert set_rule(L, p, mode, tau) == INVALID and b"temperature" in L.wab_last_error(), tau
                assert get_rule(L, p) == (1, 0.75)
        # what check_action_rule accepts, the library accepts, and stores as given
        for tau in (2.0 ** 126, 2.0 ** -126, 0.7, 1.5):
            assert set_rule(L, p, 0, tau) == 0
            assert get_rule(L, p) == (0, float(np.float32(tau)))
        assert set_rule(L, p, 1, 0.5) == 0
        assert L.wab_policy_set_action_rule(p, None) == 0  # NULL: the default
        assert get_rule(L, p) == (0, 1.0)
    finally:
        L.wab_policy_destroy(p)


def test_load_and_the_adam_step_leave_the_rule_alone():
    env = BatchedWolvesAndBushesEnv(dict(pc.OPTS_REF), num_envs=64, seed=pc.SEED, device=DEV)
    env.reset()
    model = torch.nn.Module()
    for name, (o, i) in (("affine1", (128, 449)), ("affine2", (150, 128)), ("affine3", (128, 150)),
                         ("action_head", (5, 128)), ("value_head", (1, 128))):
        setattr(model, name, torch.nn.Linear(i, o))
    model.load_state_dict(arc.spread("ref"))
    model.to(DEV)
    pol = policy.DevicePolicy(model, env)
    pol.set_action_rule("greedy", 0.5)
    opt = policy.DeviceAdam(pol, model, lr=1e-3)
    x = torch.as_tensor(pc.ref_features(64), device=DEV)
    acts = pol.act(x).clone()
    w = torch.ones(64, device=DEV)
    pol.loss_and_grad(x, acts, w, w, into=model)
    opt.step()
    pol.load(model)
    assert pol.action_rule == ("greedy", 0.5) and opt.stats()["step"] == 1
    with pytest.raises(ValueError, match="temperature"):
        pol.set_action_rule("greedy", 0.0)
    with pytest.raises(ValueError, match="mode"):
        pol.set_action_rule("argmax")
    assert pol.action_rule == ("greedy", 0.5)


def test_c_greedy_caller_equals_python_host(tmp_path):
    if not os.path.exists(DEMO):
        pytest.fail("examples/bin/c_api_greedy_demo not built (__graft_entry__.build())")
    B, T, seed, A, F = 256, 8, 0x5EED, 5, 449
    out = tmp_path / "greedy.bin"
    r = subprocess.run([DEMO, str(B), str(T), str(seed), str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("OK c_api_greedy_demo") and "one launch" in r.stdout, r.stdout
    raw = np.fromfile(out, np.uint8)
    o = 0

    def take(n, dt):
        nonlocal o
        a = raw[o:o + n * np.dtype(dt).itemsize].view(dt)
        o += n * np.dtype(dt).itemsize
        return a

    shapes = ((128, F), (128,), (150, 128), (150,), (128, 150), (128,), (A, 128), (A,), (1, 128), (1,))
    sd = {name: torch.from_numpy(take(int(np.prod(shp)), np.float32).reshape(shp).copy())
          for name, shp in zip(policy.ADAM_TENSORS, shapes)}
    acts = take(T * B, np.int8).reshape(T, B)
    probs = take(T * B * A, np.float32).reshape(T, B, A)
    value = take(T * B, np.float32).reshape(T, B)
    rew = take(T * B, np.float32).reshape(T, B)
    done = take(T * B, np.uint8).reshape(T, B)
    assert o == raw.size
    assert len(set(acts.flatten().tolist())) >= 3 and done.any()

    env = BatchedWolvesAndBushesEnv({"max_turns": 8}, num_envs=B, seed=seed, device=DEV)
    w = PragmaticObsWrapper(env)
    w.reset()
    pol = policy.DevicePolicy(sd, env)
    pol.set_action_rule("greedy")
    got = w.rollout_policy(pol, T, return_probs=True, fused=True)
    assert np.array_equal(got["actions"].cpu().numpy(), acts)
    for name, want in (("probs", probs), ("value", value), ("reward", rew)):
        assert np.array_equal(got[name].cpu().numpy().view(np.uint32), want.view(np.uint32)), name
    assert np.array_equal(got["done"].cpu().numpy(), done)
    for t in range(T):
        assert np.array_equal(acts[t], arc.first_max(probs[t])), t
    # the sampled policy on the same weights and start acts differently
    env2 = BatchedWolvesAndBushesEnv({"max_turns": 8}, num_envs=B, seed=seed, device=DEV)
    w2 = PragmaticObsWrapper(env2)
    w2.reset()
    sampled = w2.rollout_policy(policy.DevicePolicy(sd, env2), T, return_probs=True, fused=True)
    assert np.array_equal(sampled["probs"][0].cpu().numpy().view(np.uint32), probs[0].view(np.uint32))
    assert int((sampled["actions"][0].cpu().numpy() != acts[0]).sum()) > B // 8


def test_the_evaluate_example_reports_both_modes():
    spec = importlib.util.spec_from_file_location("evaluate_policy", os.path.join(REPO, "examples", "evaluate_policy.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    B, T = 256, 16
    env = BatchedWolvesAndBushesEnv(dict(pc.OPTS_REF), num_envs=B, seed=pc.SEED, device=DEV)
    w = PragmaticObsWrapper(env)
    pol = policy.DevicePolicy(arc.spread("ref"), env)
    pol.set_action_rule("sample", 1.5)
    results = {mode: mod.evaluate(w, pol, T, mode) for mode in ("greedy", "sample")}  # (greedy on the first reset)
    assert pol.action_rule == ("sample", 1.5)  # acting() put the policy's own rule back
    for mode, r in results.items():
        # max_turns = 5: every env finishes three episodes in 16 steps
        assert r["episodes"] >= 3 * B and np.isfinite(r["mean_return"]) and np.isfinite(r["mean_length"]), (mode, r)
        assert 1.0 <= r["mean_length"] <= 5.0
    assert results["sample"] != results["greedy"]
    # the greedy evaluation is the monitor's account of a greedy rollout from a reset
    env2 = BatchedWolvesAndBushesEnv(dict(pc.OPTS_REF), num_envs=B, seed=pc.SEED, device=DEV)
    w2 = PragmaticObsWrapper(env2)
    w2.reset()
    pol2 = policy.DevicePolicy(arc.spread("ref"), env2)
    pol2.set_action_rule("greedy")
    seg = w2.rollout_policy(pol2, T, return_probs=True)
    probs, acts = seg["probs"].cpu().numpy(), seg["actions"].cpu().numpy()
    for t in range(T):
        assert np.array_equal(acts[t], arc.first_max(probs[t])), t
    assert int(seg["done"].sum()) == results["greedy"]["episodes"]
