"""wab_rollout_policy (the policy fused into the multi-step kernel, one launch for T closed-loop
steps) against the two-launch loop it replaces: a hand-made loop of DevicePolicy.act +
env.step_features, compared with torch.equal on everything the call returns and leaves behind,
and the C oracle fed the returned actions.  The bits must agree because both kernels sum through
the same device functions (wab_gym_amd/csrc/wab_policy_dev.h) in the same order."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import policy_cases as pc
from wab_gym_amd import _lib, policy
from wab_gym_amd.env import BatchedWolvesAndBushesEnv
from wab_gym_amd.wrappers import PragmaticObsWrapper, discounted_returns

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WARM = 3
NET_ODD449 = (449, 17, 40, 9, 5)      # nothing a multiple of the tile
NET_WIDE449 = (449, 200, 256, 130, 5)  # two layer-1 tiles on every wave, eight layer-2 tiles
NET_MAX449 = (449, 256, 256, 256, 5)   # every width at the limit
NET_MIN449 = (449, 1, 1, 1, 5)         # every width at its minimum
KEYS = ("features", "actions", "value", "probs", "reward", "done", "returns")
# host-side tallies of how a call ran (one launch / per-step calls): they differ by design
TALLIES = ("rollout_launches", "rollout_step_calls")


@functools.lru_cache(maxsize=None)
def state_dict(net):
    if net == "ref":
        return pc.weights("ref")
    return pc.make_state_dict({"odd": NET_ODD449, "wide": NET_WIDE449, "max": NET_MAX449, "min": NET_MIN449}[net], 4321)


def closed_loop(B, opts, net="ref", base=0, warm=None, **env_kw):
    env = BatchedWolvesAndBushesEnv(dict(opts), num_envs=B, seed=pc.SEED, device=DEV, env_id_base=base, **env_kw)
    w = PragmaticObsWrapper(env)
    w.reset()
    for a in (pc.warm_actions(B, 5, WARM) if warm is None else warm):
        w.step(torch.as_tensor(np.ascontiguousarray(a), device=DEV))
    return env, w, policy.DevicePolicy(state_dict(net), env)


def manual_rollout(env, w, pol, T, feats=None):
    """T hand-made act + step_features calls and the returns of the segment."""
    B, F, A = env.num_envs, w.feature_dim, pol.n_actions
    out = {"features": torch.empty((T, B, F), device=DEV), "actions": torch.empty((T, B), dtype=torch.int8, device=DEV),
           "value": torch.empty((T, B), device=DEV), "probs": torch.empty((T, B, A), device=DEV),
           "reward": torch.empty((T, B), device=DEV), "done": torch.empty((T, B), dtype=torch.uint8, device=DEV)}
    feats = w.observation().clone() if feats is None else feats.clone()
    for t in range(T):
        out["features"][t] = feats
        pol.act(feats, out=out["actions"][t], value=out["value"][t], probs=out["probs"][t])
        _, r, d = env.step_features(out["actions"][t], feats, store_planes=False)
        out["reward"][t] = r
        out["done"][t] = d
    w.features.copy_(feats)
    out["returns"] = discounted_returns(out["reward"], out["done"], gamma=0.99, env=env)
    return out


def left_behind(env, w):
    c = env.counters()
    return {"w.features": w.features.cpu(), "state": env.state(),
            "counters": {k: v for k, v in c.items() if k not in TALLIES},
            "env.reward": env.reward.cpu(), "env.done": env.done.cpu()}


def opts_of(which):
    return {"ref": pc.OPTS_REF, "default": {}}[which]


@functools.lru_cache(maxsize=None)
def loop_reference(B, T, which="ref", net="ref"):
    """The two-launch loop's results (on the CPU) and what it leaves behind; made once per case."""
    env, w, pol = closed_loop(B, opts_of(which), net)
    out = {k: v.cpu() for k, v in manual_rollout(env, w, pol, T).items()}
    return out, left_behind(env, w)


def assert_same(got, want, keys=KEYS):
    for k in keys:
        assert got[k] is not None and torch.equal(got[k].cpu(), want[k]), k


def assert_left_behind(env, w, want):
    got = left_behind(env, w)
    assert torch.equal(got["w.features"], want["w.features"])
    for k, v in want["state"].items():
        assert np.array_equal(got["state"][k], v), k
    assert got["counters"] == want["counters"]
    assert got["counters"]["bad_actions"] == 0
    assert torch.equal(got["env.reward"], want["env.reward"]) and torch.equal(got["env.done"], want["env.done"])


def fused_flag(env, pol):
    return int(_lib.load().wab_rollout_policy_fused(env._h, pol._p))


@pytest.mark.parametrize("T", [1, 2, 7])   # no in-loop policy pass; one; both stream parities, an odd count
@pytest.mark.parametrize("B", [64, 68, 256])  # one group; a group and a partial group of 4; four groups
def test_parity_with_the_two_launch_loop(B, T):
    env, w, pol = closed_loop(B, pc.OPTS_REF)
    assert fused_flag(env, pol) == 1
    got = w.rollout_policy(pol, T, return_probs=True, fused=True)
    want, left = loop_reference(B, T)
    assert_same(got, want)
    assert_left_behind(env, w, left)
    if T == 7:
        assert int(got["done"].sum()) > 0 and len(set(got["actions"].cpu().numpy().flatten().tolist())) > 1
    # the oracle fed the returned actions gives the same features, reward and done
    from oracle.oracle import OracleBatch

    orc = OracleBatch(dict(pc.OPTS_REF), B, pc.SEED, 0)
    orc.reset()
    for a in pc.warm_actions(B, 5, WARM):
        orc.step(a)
    acts = got["actions"].cpu().numpy()
    for t in range(T):
        assert np.array_equal(got["features"][t].cpu().numpy(), pc.oracle_features(orc)), t
        orc.step(acts[t])
        assert np.array_equal(got["reward"][t].cpu().numpy(), orc.reward), t
        assert np.array_equal(got["done"][t].cpu().numpy(), orc.done), t
    assert np.array_equal(w.features.cpu().numpy(), pc.oracle_features(orc))


def test_default_rules_instance():
    """Default options (the instance with the rules as constants), long enough for episodes to end."""
    B, T = 64, 48
    if int(loop_reference(B, T, "default")[0]["done"].sum()) == 0:
        T = 64
    want, left = loop_reference(B, T, "default")
    assert int(want["done"].sum()) > 0
    env, w, pol = closed_loop(B, {})
    assert fused_flag(env, pol) == 1
    got = w.rollout_policy(pol, T, return_probs=True, fused=True)
    assert_same(got, want)
    assert_left_behind(env, w, left)


@pytest.mark.parametrize("net,T", [("odd", 5), ("wide", 3), ("max", 3), ("min", 5)])
def test_other_widths(net, T):
    """449-17-40-9-5 (no width a multiple of the tile), 449-200-256-130-5 (the widest layers:
    two layer-1 tiles on every wave), 449-256-256-256-5 (every width at the limit) and 449-1-1-1-5
    (every width at its minimum) are fused and equal the loop."""
    B = 68
    env, w, pol = closed_loop(B, pc.OPTS_REF, net)
    assert fused_flag(env, pol) == 1
    got = w.rollout_policy(pol, T, return_probs=True, fused=True)
    want, left = loop_reference(B, T, "ref", net)
    assert_same(got, want)
    assert_left_behind(env, w, left)


def test_without_stored_features_and_with_probs():
    B, T = 68, 7
    env, w, pol = closed_loop(B, pc.OPTS_REF)
    got = w.rollout_policy(pol, T, store_features=False, return_probs=True, fused=True)
    want, left = loop_reference(B, T)
    assert got["features"] is None
    assert_same(got, want, [k for k in KEYS if k != "features"])
    assert_left_behind(env, w, left)
    # the loop with two alternating rows gives the same
    env2, w2, pol2 = closed_loop(B, pc.OPTS_REF)
    got2 = w2.rollout_policy(pol2, T, store_features=False, return_probs=True, fused=False)
    assert got2["features"] is None
    assert_same(got2, want, [k for k in KEYS if k != "features"])
    assert_left_behind(env2, w2, left)


def c_rollout(env, pol, f0, T, feats, last, probs=True):
    """wab_rollout_policy through ctypes; returns (rc, dict of device tensors)."""
    B, A = env.num_envs, pol.n_actions
    out = {"actions": torch.full((T, B), -1, dtype=torch.int8, device=DEV), "value": torch.empty((T, B), device=DEV),
           "probs": torch.empty((T, B, A), device=DEV) if probs else None, "reward": torch.empty((T, B), device=DEV),
           "done": torch.empty((T, B), dtype=torch.uint8, device=DEV), "returns": torch.empty((T, B), device=DEV),
           "scal": torch.empty((3, T, B), dtype=torch.uint8, device=DEV), "features": feats}
    s = out["scal"]
    st = _lib.WabObs(None, s[0].data_ptr(), s[1].data_ptr(), s[2].data_ptr())
    ptr = lambda x: None if x is None else x.data_ptr()  # noqa: E731
    rc = _lib.load().wab_rollout_policy(env._h, pol._p, ptr(f0), T, ctypes.addressof(st), ptr(out["actions"]),
                                        ptr(out["value"]), ptr(out["probs"]), ptr(out["reward"]), ptr(out["done"]),
                                        ptr(feats), ptr(last), 0.99, None, ptr(out["returns"]), env._stream())
    return rc, out


def test_features0_with_values_bf16_cannot_hold():
    B, T = 64, 2
    env, w, pol = closed_loop(B, pc.OPTS_REF)
    rng = np.random.RandomState(11)
    f0 = w.observation().clone()
    f0[:, 30:34] = torch.as_tensor(rng.standard_normal((B, 4)).astype(np.float32), device=DEV)
    f0[:, 36] = float(np.float32(1.0) / np.float32(3.0))
    f0[:, 448] = torch.as_tensor(rng.standard_normal(B).astype(np.float32), device=DEV)
    a0 = torch.empty(B, dtype=torch.int8, device=DEV)
    p0, v0 = torch.empty((B, 5), device=DEV), torch.empty(B, device=DEV)
    pol.act(f0, out=a0, probs=p0, value=v0)
    feats = torch.zeros((T, B, 449), device=DEV)
    last = torch.zeros((B, 449), device=DEV)
    rc, got = c_rollout(env, pol, f0, T, feats, last)
    assert rc == 0, _lib.load().wab_last_error()
    assert torch.equal(got["actions"][0], a0) and torch.equal(got["value"][0], v0) and torch.equal(got["probs"][0], p0)
    assert torch.equal(feats[0], f0)
    env2, w2, pol2 = closed_loop(B, pc.OPTS_REF)
    want = manual_rollout(env2, w2, pol2, T, feats=f0)
    got["features"] = feats
    assert_same(got, {k: v.cpu() for k, v in want.items()})
    assert torch.equal(last, w2.features)
    for k, v in env2.state().items():
        assert np.array_equal(env.state()[k], v), k


def test_shard_invariance():
    T = 7
    warm = pc.warm_actions(128, 5, WARM)
    env, w, pol = closed_loop(128, pc.OPTS_REF, warm=warm)
    whole = w.rollout_policy(pol, T, return_probs=True, fused=True)
    parts = []
    for lo in (0, 64):
        e, ww, pp = closed_loop(64, pc.OPTS_REF, base=lo, warm=warm[:, lo:lo + 64])
        parts.append((ww.rollout_policy(pp, T, return_probs=True, fused=True), ww.features))
    for k in KEYS:
        assert torch.equal(torch.cat([p[0][k] for p in parts], dim=1), whole[k]), k
    assert torch.equal(torch.cat([p[1] for p in parts], dim=0), w.features)
    assert int(whole["done"].sum()) > 0


def test_captured_in_a_graph():
    T, B = 7, 256
    env, w, pol = closed_loop(B, pc.OPTS_REF)
    w.rollout_policy(pol, T, return_probs=True, fused=True)  # eager: the kernel instance is loaded
    want, left = loop_reference(B, T)
    env2, w2, pol2 = closed_loop(B, pc.OPTS_REF)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            got = w2.rollout_policy(pol2, T, return_probs=True, fused=True)
    torch.cuda.current_stream().wait_stream(side)
    g.replay()
    torch.cuda.synchronize()
    assert_same(got, want)
    assert_left_behind(env2, w2, left)


def test_continuation():
    """Two calls of 3 and 4 steps are one of 7: the second starts from the first's features_last."""
    B = 68
    env, w, pol = closed_loop(B, pc.OPTS_REF)
    first = w.rollout_policy(pol, 3, return_probs=True, fused=True)
    second = w.rollout_policy(pol, 4, return_probs=True, fused=True)
    want, left = loop_reference(B, 7)
    for k in KEYS:
        if k != "returns":  # (each call's returns restart at its own end)
            assert torch.equal(torch.cat([first[k], second[k]], dim=0).cpu(), want[k]), k
    assert_left_behind(env, w, left)


@pytest.mark.parametrize("B,kw", [(64, {"wolf_slots": 16}), (65, {})])
def test_fallback_handles(B, kw):
    """A 16-slot handle and one whose feature slices are not 16-byte aligned take the 2 T launches."""
    T = 4
    env, w, pol = closed_loop(B, pc.OPTS_REF, **kw)
    assert fused_flag(env, pol) == 0
    with pytest.raises(NotImplementedError):
        w.rollout_policy(pol, T, fused=True)
    got = w.rollout_policy(pol, T, return_probs=True)
    env2, w2, pol2 = closed_loop(B, pc.OPTS_REF, **kw)
    want = {k: v.cpu() for k, v in manual_rollout(env2, w2, pol2, T).items()}
    assert_same(got, want)
    assert_left_behind(env, w, left_behind(env2, w2))
    # the C entry point itself runs the 2 T launches there, features stored or not
    env3, w3, pol3 = closed_loop(B, pc.OPTS_REF, **kw)
    last = torch.zeros((B, 449), device=DEV)
    rc, c = c_rollout(env3, pol3, w3.observation().clone(), T, None, last)
    assert rc == 0, _lib.load().wab_last_error()
    assert_same(c, want, [k for k in KEYS if k != "features"])
    assert torch.equal(last, w2.features)


def test_refusals():
    L = _lib.load()
    B, T = 64, 2
    env, w, pol = closed_loop(B, pc.OPTS_REF)
    f0 = w.observation().clone()
    last = torch.zeros((B, 449), device=DEV)
    before = env.state()
    # a policy of another n_actions
    p = ctypes.c_void_p()
    shp = _lib.WabPolicyShape(449, 128, 150, 128, 6)
    assert L.wab_policy_create(ctypes.addressof(shp), 0, ctypes.byref(p)) == 0

    class Raw:
        n_actions = 6

    Raw._p = p
    rc, _ = c_rollout(env, Raw, f0, T, None, last)
    assert rc == -1 and b"actions" in L.wab_last_error()
    L.wab_policy_destroy(p)
    # before the first wab_policy_load
    shp = _lib.WabPolicyShape(449, 128, 150, 128, 5)
    assert L.wab_policy_create(ctypes.addressof(shp), 0, ctypes.byref(p)) == 0
    Raw._p, Raw.n_actions = p, 5
    rc, _ = c_rollout(env, Raw, f0, T, None, last)
    assert rc == -4 and b"wab_policy_load" in L.wab_last_error()
    L.wab_policy_destroy(p)
    # features_last is required; misaligned feature rows are refused
    rc, _ = c_rollout(env, pol, f0, T, None, None)
    assert rc == -1
    rc, _ = c_rollout(env, pol, None, T, None, last)
    assert rc == -1
    odd = torch.zeros(B * 449 + 4, device=DEV)[1:B * 449 + 1].view(B, 449)
    rc, _ = c_rollout(env, pol, f0, T, None, odd)
    assert rc == -1 and b"aligned" in L.wab_last_error()
    assert L.wab_rollout_policy_fused(None, pol._p) == -1 and L.wab_rollout_policy_fused(env._h, None) == -1
    # before the first reset
    fresh = BatchedWolvesAndBushesEnv(dict(pc.OPTS_REF), num_envs=B, seed=pc.SEED, device=DEV)
    rc, _ = c_rollout(fresh, policy.DevicePolicy(pc.weights("ref"), fresh), f0, T, None, last)
    assert rc == -4 and b"wab_reset" in L.wab_last_error()
    # nothing ran
    for k, v in env.state().items():
        assert np.array_equal(before[k], v), k
