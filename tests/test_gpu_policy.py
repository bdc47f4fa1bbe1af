"""wab_policy_act on the GPU against its references (wab_gym_amd/policy.py): probs and value
against reference_forward within half of E_bf16 (what the bf16 contract itself costs on the same
inputs, tests/test_policy_host.py), actions exactly sample_reference of the kernel's own probs and
the C oracle's (episode, turn); sharding, reloading, rollout_policy eager and graph-captured, and
the refusals.  Nets whose sums are exact in any order (policy_cases.exact_net) are compared bit
for bit instead, at the shapes where policy_lds and the kernel's two instances change path, each
asserted through wab_debug_policy_plan.

Measured on an MI355X (max |kernel - reference_forward| / E_bf16, worst of the B cases): see
DESIGN.md, "wab_policy_act"."""
import ctypes

import numpy as np
import pytest
import torch

import policy_cases as pc
from wab_gym_amd import _lib, policy
from wab_gym_amd.env import BatchedWolvesAndBushesEnv
from wab_gym_amd.wrappers import PragmaticObsWrapper, discounted_returns

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def warmed_env(B, opts=None, base=0, actions=None):
    """An env reset and stepped through the warm-up actions; returns (env, features [B, 449])."""
    env = BatchedWolvesAndBushesEnv(dict(pc.OPTS_REF if opts is None else opts), num_envs=B, seed=pc.SEED,
                                    device=DEV, env_id_base=base)
    env.reset()
    feats = torch.zeros((B, 449), dtype=torch.float32, device=DEV)
    for a in (pc.warm_actions(B, env.n_actions) if actions is None else actions):
        env.step_features(np.ascontiguousarray(a), feats, store_planes=False)
    return env, feats


def check_reference_has_every_path(sd, feats):
    """Before any GPU comparison: the reference alone has units at both clamp limits and negative
    pre-activations in every hidden layer (the slope and the clamp are exercised)."""
    hidden = []
    policy.reference_forward(sd, feats, hidden=hidden)
    assert all(bool((z < 0).any()) for z, _ in hidden)
    assert bool((hidden[2][1] == 4.0).any()) and bool((hidden[2][1] == -4.0).any())


def check_outputs(sd, feats, probs, value, what):
    """max |kernel - reference_forward| <= 0.5 * E_bf16 of the same inputs; rows of probs sum to 1."""
    feats = np.asarray(feats)
    rp, rv = policy.reference_forward(sd, feats)
    e_p, e_v = pc.contract_cost(sd, feats)
    p, v = probs.cpu(), value.cpu()
    err_p = float((p.double() - rp).abs().max())
    err_v = float((v.double() - rv).abs().max())
    print("%s: probs err %.3e (E_bf16 %.3e, ratio %.3f)  value err %.3e (E_bf16 %.3e, ratio %.3f)"
          % (what, err_p, e_p, err_p / e_p, err_v, e_v, err_v / e_v))
    A = p.shape[1]
    assert float((p.double().sum(1) - 1).abs().max()) <= 4 * A * 2.0 ** -23
    assert bool((p >= 0).all())
    assert err_p <= 0.5 * e_p, (what, err_p, e_p)
    assert err_v <= 0.5 * e_v, (what, err_v, e_v)


def check_actions(actions, probs, orc, base=0):
    st = orc.state()
    want = policy.sample_reference(probs.cpu().numpy(), pc.SEED, base + np.arange(orc.B), st["episode"], st["turn"])
    assert np.array_equal(actions.cpu().numpy(), want)
    return set(st["episode"].tolist())


@pytest.mark.parametrize("B", pc.BATCHES)
def test_reference_net_on_real_features(B):
    """449-128-150-128-5 on the features wab_step_features wrote, then the closed loop up to step
    12 (max_turns = 5: envs in different episodes and turns), every action checked."""
    sd = pc.weights("ref")
    check_reference_has_every_path(sd, pc.ref_features(257))
    env, feats = warmed_env(B)
    orc = pc.oracle_after_warmup(B)
    assert np.array_equal(feats.cpu().numpy(), pc.ref_features(B))
    pol = policy.DevicePolicy(sd, env)
    probs = torch.full((B, 5), -1.0, device=DEV)
    value = torch.full((B,), 99.0, device=DEV)
    episodes = set()
    for t in range(pc.WARM_STEPS, 12):
        a = pol.act(feats, probs=probs, value=value)
        if t == pc.WARM_STEPS:
            check_outputs(sd, pc.ref_features(B), probs, value, "ref net B=%d" % B)
        episodes |= check_actions(a, probs, orc)
        orc.step(a.cpu().numpy())
        env.step_features(a, feats, store_planes=False)
        assert np.array_equal(feats.cpu().numpy(), pc.oracle_features(orc))
    check_outputs(sd, feats.cpu().numpy(), *pol_outputs(pol, feats), "ref net B=%d, step 12" % B)
    assert len(episodes) >= 2
    assert env.counters()["bad_actions"] == 0


def pol_outputs(pol, feats):
    B = feats.shape[0]
    probs = torch.empty((B, pol.n_actions), device=DEV)
    value = torch.empty((B,), device=DEV)
    pol.act(feats, probs=probs, value=value)
    return probs, value


@pytest.mark.parametrize("B", pc.BATCHES)
def test_odd_net_on_hand_made_features(B):
    """37-17-40-9 with A = 6 (nothing a multiple of the tile) on the 6-action option set."""
    sd = pc.weights("odd")
    check_reference_has_every_path(sd, pc.odd_features(257))
    env, _ = warmed_env(B, pc.OPTS_ODD)
    assert env.n_actions == 6
    orc = pc.oracle_after_warmup(B, pc.OPTS_ODD)
    pol = policy.DevicePolicy(sd, env)
    feats = torch.as_tensor(pc.odd_features(B), device=DEV)
    probs = torch.empty((B, 6), device=DEV)
    value = torch.empty((B,), device=DEV)
    a = pol.act(feats, probs=probs, value=value)
    check_outputs(sd, pc.odd_features(B), probs, value, "odd net B=%d" % B)
    check_actions(a, probs, orc)


def test_wide_net_two_layer1_tiles_per_wave():
    """50-200-256-130: h1 > 128 runs the kernel instance that holds two layer-1 tiles per wave; 256
    is the widest layer accepted."""
    B = 129
    sd = pc.weights("wide")
    x = pc.odd_features(B, 50)
    check_reference_has_every_path(sd, x)
    env, _ = warmed_env(B)
    orc = pc.oracle_after_warmup(B)
    pol = policy.DevicePolicy(sd, env)
    probs, value = pol_outputs(pol, torch.as_tensor(x, device=DEV))
    check_outputs(sd, x, probs, value, "wide net B=%d" % B)
    check_actions(pol.actions, probs, orc)


def policy_plan(pol):
    out = (ctypes.c_int32 * 5)(*[-1] * 5)
    _lib.check(_lib.load().wab_debug_policy_plan(pol._p, out), "wab_debug_policy_plan")
    return tuple(out)


# The exact nets' probabilities differ from the reference's only by expf, the sum of A terms and
# one divide.  Worst |p - p_ref| / p_ref measured on an MI355X over every exact case (p_ref the
# float64 softmax of reference_forward): EXACT_PROBS_MEASURED; the gate is four times that, rounded
# up to a power of two (expf's error varies with its argument and the cases sample only some).
EXACT_PROBS_MEASURED = 2.269e-07  # 3.81 * 2^-24, at (16, 130, 8, 8, 6), B = 128
EXACT_PROBS_GATE = 2.0 ** -20       # 9.54e-07 >= 4 * 2.269e-07 = 9.08e-07


@pytest.mark.parametrize("B", pc.EXACT_BATCHES)
@pytest.mark.parametrize("shape", list(pc.EXACT_SHAPES))
def test_exact_net_is_bit_equal(shape, B):
    """Nets whose every fp32 sum is exact in any order (pc.exact_certificate, asserted here on
    this case's own inputs): a dropped pad column, two swapped units or a wrong fragment row has no
    rounding band to hide in.  value == float32(reference value) bit for bit; actions are
    sample_reference of the kernel's own probs; probs within EXACT_PROBS_GATE of the float64
    softmax, relative; and the launch is the planned one (chunks, KC, last chunk, LDS, instance).
    Worst relative probs error measured on an MI355X over all 50 cases: 2.269e-07 (3.81 * 2^-24);
    the gate is 2^-20."""
    F, A = shape[0], shape[4]
    sd = pc.exact_net(shape)
    x = pc.exact_features(B, F)
    pc.exact_certificate(sd, x)
    check_reference_has_every_path(sd, pc.exact_features(257, F))
    opts = pc.OPTS_REF if A == 5 else pc.OPTS_ODD
    env, _ = warmed_env(B, opts)
    assert env.n_actions == A
    orc = pc.oracle_after_warmup(B, opts)
    pol = policy.DevicePolicy(sd, env)
    assert policy_plan(pol) == pc.EXACT_SHAPES[shape]
    probs, value = pol_outputs(pol, torch.as_tensor(x, device=DEV))
    rp, rv = policy.reference_forward(sd, x)
    want_v = rv.to(torch.float32)
    assert torch.equal(want_v.double(), rv)  # (the certificate: the value is a float32)
    assert np.array_equal(value.cpu().numpy().view(np.uint32), want_v.numpy().view(np.uint32))
    check_actions(pol.actions, probs, orc)
    p = probs.cpu().double()
    ratio = float(((p - rp).abs() / rp).max())
    print("exact net %s B=%d: worst |p - p_ref| / p_ref = %.3e (%.2f * 2^-24), smallest p_ref %.3e"
          % (shape, B, ratio, ratio * 2.0 ** 24, float(rp.min())))
    assert float((p.sum(1) - 1).abs().max()) <= 4 * A * 2.0 ** -23
    assert ratio <= EXACT_PROBS_GATE, (shape, B, ratio)


@pytest.mark.parametrize("B", [128, 257])
@pytest.mark.parametrize("net", [(449, 129, 150, 128, 5), (449, 256, 256, 256, 5)])
def test_widest_nets_with_random_weights(net, B):
    """The first <true> net (NT1 = 5) and the all-256 net (two chunks, 132 KB of LDS) with
    torch-initialised weights on real features, under the random-weight gate 0.5 * E_bf16."""
    sd = pc.make_state_dict(net, 77)
    check_reference_has_every_path(sd, pc.ref_features(257))
    env, feats = warmed_env(B)
    orc = pc.oracle_after_warmup(B)
    pol = policy.DevicePolicy(sd, env)
    assert policy_plan(pol)[4] == 1
    probs, value = pol_outputs(pol, feats)
    check_outputs(sd, pc.ref_features(B), probs, value, "net %s B=%d" % (net, B))
    check_actions(pol.actions, probs, orc)


def test_sharding_two_handles_give_the_actions_of_one():
    sd = pc.weights("ref")
    warm = pc.warm_actions(257, 5)
    whole, f = warmed_env(257)
    a_whole = policy.DevicePolicy(sd, whole).act(f).cpu().numpy()
    parts = []
    for lo, n in ((0, 100), (100, 157)):
        env, fs = warmed_env(n, base=lo, actions=warm[:, lo:lo + n])
        assert np.array_equal(fs.cpu().numpy(), pc.ref_features(257)[lo:lo + n])
        parts.append(policy.DevicePolicy(sd, env).act(fs).cpu().numpy())
    assert np.array_equal(np.concatenate(parts), a_whole)
    assert len(set(a_whole.tolist())) > 1


def test_null_probs_and_value_give_the_same_actions():
    env, f = warmed_env(257)
    pol = policy.DevicePolicy(pc.weights("ref"), env)
    probs, value = pol_outputs(pol, f)
    with_out = pol.actions.clone()
    out = torch.full((257,), -1, dtype=torch.int8, device=DEV)
    assert pol.act(f, out=out) is out
    assert torch.equal(out, with_out)
    only_value = torch.empty_like(value)
    pol.act(f, value=only_value)
    assert torch.equal(only_value, value) and torch.equal(pol.actions, with_out)


def test_load_twice_uses_the_second_weights():
    env, f = warmed_env(65)
    first, second = pc.weights("ref", 0), pc.weights("ref", 1)
    pol = policy.DevicePolicy(first, env)
    p1, _ = pol_outputs(pol, f)
    pol.load(second)
    p2, v2 = pol_outputs(pol, f)
    assert not torch.equal(p1, p2)
    check_outputs(second, pc.ref_features(65), p2, v2, "second load")
    module = torch.nn.Module()  # a module with the five Linears loads like a state dict
    for name, (o, i) in (("affine1", (128, 449)), ("affine2", (150, 128)), ("affine3", (128, 150)),
                         ("action_head", (5, 128)), ("value_head", (1, 128))):
        setattr(module, name, torch.nn.Linear(i, o))
    module.load_state_dict(first)
    pol.load(module.to(DEV))
    p3, _ = pol_outputs(pol, f)
    assert torch.equal(p3, p1)


def manual_rollout(env, w, pol, T):
    """T hand-made act + step_features calls, as rollout_policy documents itself."""
    B, F = env.num_envs, w.feature_dim
    out = {"features": torch.empty((T, B, F), device=DEV), "actions": torch.empty((T, B), dtype=torch.int8, device=DEV),
           "value": torch.empty((T, B), device=DEV), "reward": torch.empty((T, B), device=DEV),
           "done": torch.empty((T, B), dtype=torch.uint8, device=DEV)}
    feats = w.observation().clone()
    for t in range(T):
        out["features"][t] = feats
        pol.act(feats, out=out["actions"][t], value=out["value"][t])
        _, r, d = env.step_features(out["actions"][t], feats, store_planes=False)
        out["reward"][t] = r
        out["done"][t] = d
    w.features.copy_(feats)
    return out


def fresh_closed_loop(B):
    env = BatchedWolvesAndBushesEnv(dict(pc.OPTS_REF), num_envs=B, seed=pc.SEED, device=DEV)
    w = PragmaticObsWrapper(env)
    w.reset()
    for a in pc.warm_actions(B, 5, 3):
        w.step(torch.as_tensor(a, device=DEV))
    return env, w, policy.DevicePolicy(pc.weights("ref"), env)


KEYS = ("features", "actions", "value", "reward", "done")


@pytest.mark.parametrize("B", [65, 256])  # feature slices not 16-byte aligned / aligned
def test_rollout_policy_is_six_hand_made_steps(B):
    T = 6
    env, w, pol = fresh_closed_loop(B)
    got = w.rollout_policy(pol, T)
    env2, w2, pol2 = fresh_closed_loop(B)
    want = manual_rollout(env2, w2, pol2, T)
    for k in KEYS:
        assert torch.equal(got[k], want[k]), k
    assert torch.equal(w.features, w2.features)
    # the oracle fed the returned actions gives the same features, reward and done
    from oracle.oracle import OracleBatch

    orc = OracleBatch(dict(pc.OPTS_REF), B, pc.SEED, 0)
    orc.reset()
    for a in pc.warm_actions(B, 5, 3):
        orc.step(a)
    acts = got["actions"].cpu().numpy()
    for t in range(T):
        assert np.array_equal(got["features"][t].cpu().numpy(), pc.oracle_features(orc)), t
        orc.step(acts[t])
        assert np.array_equal(got["reward"][t].cpu().numpy(), orc.reward), t
        assert np.array_equal(got["done"][t].cpu().numpy(), orc.done), t
    assert torch.equal(got["returns"], discounted_returns(got["reward"], got["done"], gamma=0.99, env=env))
    assert int(got["done"].sum()) > 0 and len(set(acts.flatten().tolist())) > 1
    assert torch.equal(env.reward, got["reward"][-1]) and torch.equal(env.done, got["done"][-1])


def test_rollout_policy_captured_in_a_graph():
    T, B = 6, 256
    env, w, pol = fresh_closed_loop(B)
    want = w.rollout_policy(pol, T)  # eager (and every kernel loaded before the capture)
    env2, w2, pol2 = fresh_closed_loop(B)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            got = w2.rollout_policy(pol2, T)
    torch.cuda.current_stream().wait_stream(side)
    g.replay()
    torch.cuda.synchronize()
    for k in KEYS + ("returns",):
        assert torch.equal(got[k], want[k]), k
    assert env2.counters()["steps"] == env.counters()["steps"]


def test_refusals():
    L = _lib.load()
    env, f = warmed_env(64)
    with pytest.raises(ValueError, match="actions"):
        policy.DevicePolicy(pc.weights("odd"), env)          # 6 actions, the env has 5
    # the same through the C-ABI
    p = ctypes.c_void_p()
    shp = _lib.WabPolicyShape(449, 128, 150, 128, 6)
    assert L.wab_policy_create(ctypes.addressof(shp), 0, ctypes.byref(p)) == 0
    acts = torch.zeros(64, dtype=torch.int8, device=DEV)
    rc = L.wab_policy_act(env._h, p, f.data_ptr(), acts.data_ptr(), None, None, env._stream())
    assert rc == -1 and b"actions" in L.wab_last_error()
    L.wab_policy_destroy(p)
    # act before the first load
    shp = _lib.WabPolicyShape(449, 128, 150, 128, 5)
    assert L.wab_policy_create(ctypes.addressof(shp), 0, ctypes.byref(p)) == 0
    rc = L.wab_policy_act(env._h, p, f.data_ptr(), acts.data_ptr(), None, None, env._stream())
    assert rc == -4 and b"wab_policy_load" in L.wab_last_error()
    assert L.wab_policy_act(env._h, p, None, acts.data_ptr(), None, None, env._stream()) == -1
    assert L.wab_policy_load(p, None, env._stream()) == -1
    L.wab_policy_destroy(p)
    # shapes outside the ranges
    for bad in ((449, 257, 150, 128, 5), (449, 128, 0, 128, 5), (0, 128, 150, 128, 5), (449, 128, 150, 128, 9),
                (449, 128, 150, 128, 1)):
        shp = _lib.WabPolicyShape(*bad)
        assert L.wab_policy_create(ctypes.addressof(shp), 0, ctypes.byref(p)) == -1, bad
    wide = pc.make_state_dict((449, 257, 150, 128, 5), 1)
    with pytest.raises(ValueError, match="257"):
        policy.DevicePolicy(wide, env)
    # features of the wrong shape or dtype
    pol = policy.DevicePolicy(pc.weights("ref"), env)
    for bad in (f[:, :448], f[:63], f.double(), f.cpu(), f.t().contiguous().t()):
        with pytest.raises(ValueError, match="features"):
            pol.act(bad)
    with pytest.raises(ValueError, match="probs"):
        pol.act(f, probs=torch.empty((64, 6), device=DEV))
    with pytest.raises(ValueError, match="out"):
        pol.act(f, out=torch.empty(64, dtype=torch.int64, device=DEV))
    fresh = BatchedWolvesAndBushesEnv(dict(pc.OPTS_REF), num_envs=64, seed=pc.SEED, device=DEV)
    with pytest.raises(_lib.WabError, match="wab_reset"):
        policy.DevicePolicy(pc.weights("ref"), fresh).act(f)  # no env has an episode yet
