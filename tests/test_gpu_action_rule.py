"""The action rule on the GPU (wab_policy_set_action_rule; include/wab.h, "Action rule"): greedy
is the first maximum of the kernel's own probs, ties go to the lowest index, a temperature
scales the logits by its float32 reciprocal once, both reach the one-launch rollout and the
two-launch loop alike, a captured graph keeps its rule, shards agree, and evaluate and the
gradient calls ignore all of it.  The nets are action_rule_cases.spread(): their argmax moves with
the input, which each greedy test first asserts from the reference alone.

The one-launch rollout takes batches whose feature rows fill whole 16-byte units (B * 449 a
multiple of 4): B = 256 runs it (fused=True); B = 65 cannot, so there the rule is followed
through the wrapper's loop and through wab_rollout_policy's own 2 T launches."""
import numpy as np
import pytest
import torch

import action_rule_cases as arc
import policy_cases as pc
import test_gpu_policy as tgp
import test_gpu_rollout_policy as trp
from wab_gym_amd import features, policy
from wab_gym_amd.env import BatchedWolvesAndBushesEnv
from wab_gym_amd.wrappers import PragmaticObsWrapper

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BATCHES = (1, 63, 64, 65, 129, 257)  # a workgroup of the act kernel takes 128 envs, a head wave 32 columns
KEYS = trp.KEYS


def case_inputs(which, B, base=0, actions=None):
    """(env after the warm-up, features on the host [B, F]) of a net of policy_cases."""
    env, feats = tgp.warmed_env(B, pc.OPTS_ODD if which == "odd" else pc.OPTS_REF, base, actions)
    if which == "ref":
        x = feats.cpu().numpy()
        if base == 0 and actions is None:
            assert np.array_equal(x, pc.ref_features(B))
    else:
        x = pc.odd_features(B) if which == "odd" else pc.odd_features(B, 50)
    return env, x


def act_all(pol, x):
    """(actions, probs, value) on the host of one act() on features x (host or device)."""
    B = pol.env.num_envs
    f = torch.as_tensor(x, device=DEV)
    a = torch.full((B,), -1, dtype=torch.int8, device=DEV)
    p = torch.full((B, pol.n_actions), -1.0, device=DEV)
    v = torch.full((B,), 99.0, device=DEV)
    assert pol.act(f, out=a, probs=p, value=v) is a
    return a.cpu().numpy(), p.cpu().numpy(), v.cpu().numpy()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def keys_of(env, base=0):
    st = env.state()
    return pc.SEED, base + np.arange(env.num_envs), st["episode"], st["turn"]


# ------------------------------------------------------------------ 1. greedy = first maximum
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("which", ["ref", "odd", "wide"])
def test_greedy_is_the_first_maximum_of_the_kernels_own_probs(which, B):
    sd = arc.spread(which)
    assert arc.assert_reference_spreads(sd, arc.FEATURES[which]()) == arc.ARGMAX_COUNTS[which]
    env, x = case_inputs(which, B)
    pol = policy.DevicePolicy(sd, env)
    assert pol.action_rule == ("sample", 1.0)
    a_s, p_s, v_s = act_all(pol, x)
    with pol.acting(mode="greedy") as same:
        assert same is pol and pol.action_rule == ("greedy", 1.0)
        a_g, p_g, v_g = act_all(pol, x)
    assert pol.action_rule == ("sample", 1.0)
    assert np.array_equal(a_g, policy.select_reference(p_g, *keys_of(env), mode="greedy"))
    assert np.array_equal(a_g, arc.first_max(p_g))
    assert np.array_equal(a_s, policy.select_reference(p_s, *keys_of(env), mode="sample"))
    assert same_bits(p_g, p_s) and same_bits(v_g, v_s)
    tgp.check_outputs(sd, x, torch.as_tensor(p_g), torch.as_tensor(v_g), "spread %s B=%d" % (which, B))
    # against the reference: wherever its top two are further apart than E_bf16 (twice the
    # 0.5 E_bf16 that check_outputs allows each of them), the kernel's argmax is its argmax
    am, gap = arc.reference_argmax(sd, x)
    e_p = pc.contract_cost(sd, x)[0]
    clear = gap > e_p
    print("spread %s B=%d: %d of %d rows within E_bf16 = %.3e of a tie, left out" % (which, B, int((~clear).sum()), B, e_p))
    assert int((~clear).sum()) <= 0.05 * B
    assert np.array_equal(a_g[clear], am[clear])
    if B == BATCHES[-1]:  # (at the largest batch, as the reference alone showed above)
        assert len(set(a_g.tolist())) >= 3 and int((a_g != a_s).sum()) * 4 >= B


# ------------------------------------------------------------------ 2. ties
@pytest.mark.parametrize("which", ["ref", "odd"])
def test_ties_go_to_the_lowest_index(which):
    B = 65
    env, x = case_inputs(which, B)
    pol = policy.DevicePolicy(arc.tie_net(which, "all"), env)
    a_s, p_s, _ = act_all(pol, x)
    assert (p_s == p_s[:, :1]).all()  # identical head rows: identical logits, identical probabilities
    assert len(set(a_s.tolist())) >= 3
    pol.set_action_rule("greedy")
    a_g, p_g, _ = act_all(pol, x)
    assert same_bits(p_g, p_s) and (a_g == 0).all()
    # rows 1 and 3 identical, 8 above the rest: the first of the two
    pol.load(arc.tie_net(which, "pair"))
    a_g, p_g, _ = act_all(pol, x)
    assert (p_g[:, 1] == p_g[:, 3]).all() and np.delete(p_g, [1, 3], axis=1).max() < 1e-3
    assert (a_g == 1).all()
    assert pol.action_rule == ("greedy", 1.0)  # load() leaves the rule alone
    pol.set_action_rule("sample")
    a_s, _, _ = act_all(pol, x)
    assert {1, 3} <= set(a_s.tolist())  # (sampling takes both of the pair)


# ------------------------------------------------------------------ 3. temperature, exact
def closed_loop(B, sd, base=0, warm=None, opts=None):
    """trp.closed_loop with the state dict given."""
    env = BatchedWolvesAndBushesEnv(dict(pc.OPTS_REF if opts is None else opts), num_envs=B, seed=pc.SEED, device=DEV,
                                    env_id_base=base)
    w = PragmaticObsWrapper(env)
    w.reset()
    for a in (pc.warm_actions(B, 5, trp.WARM) if warm is None else warm):
        w.step(torch.as_tensor(np.ascontiguousarray(a), device=DEV))
    return env, w, policy.DevicePolicy(sd, env)


def assert_same(got, want, keys=KEYS, what=""):
    for k in keys:
        assert got[k] is not None and torch.equal(got[k].cpu(), want[k].cpu()), (what, k)


def test_temperature_one_half_is_the_net_with_the_head_doubled_act():
    B = 129
    sd = arc.spread("ref")
    env, x = case_inputs("ref", B)
    half, twice = policy.DevicePolicy(sd, env), policy.DevicePolicy(arc.doubled_head(sd), env)
    half.set_action_rule("sample", 0.5)
    assert half.action_rule == ("sample", 0.5) and twice.action_rule == ("sample", 1.0)
    plain = act_all(policy.DevicePolicy(sd, env), x)
    for mode in ("sample", "greedy"):
        half.set_action_rule(mode, 0.5)
        twice.set_action_rule(mode, 1.0)
        got, want = act_all(half, x), act_all(twice, x)
        for g, w_, name in zip(got, want, ("actions", "probs", "value")):
            assert same_bits(g, w_), (mode, name)
        assert same_bits(got[2], plain[2]) and not same_bits(got[1], plain[1])  # the value is untouched


@pytest.mark.parametrize("B", [65, 256])
def test_temperature_one_half_is_the_net_with_the_head_doubled_rollout(B):
    T = 6
    sd = arc.spread("ref")
    env, w, half = closed_loop(B, sd)
    half.set_action_rule("sample", 0.5)
    got = w.rollout_policy(half, T, return_probs=True, fused=True if B == 256 else None)
    env2, w2, twice = closed_loop(B, arc.doubled_head(sd))
    want = w2.rollout_policy(twice, T, return_probs=True, fused=True if B == 256 else None)
    assert_same(got, want)
    assert torch.equal(w.features, w2.features)
    assert env.counters()["rollout_launches"] == (1 if B == 256 else 0)
    env3, w3, plain = closed_loop(B, sd)
    assert not torch.equal(w3.rollout_policy(plain, T, return_probs=True)["probs"], got["probs"])


# ------------------------------------------------------------------ 4. temperature, general
# At a general temperature the exact nets' probabilities differ from the float64 softmax of lg'
# (the float32 product, which numpy restates exactly) by expf, the sum of A terms and one divide,
# which EXACT_PROBS_GATE = 2^-20 covers (tests/test_gpu_policy.py), and by the one rounding of
# lg' - max, at most 2^-24 |z| relative in a numerator and as much in the denominator:
# 2^-23 Zmax, Zmax the case's largest |z| in the reference (asserted < 80).
# Worst |p - p_ref| / p_ref measured on an MI355X over the 12 cases: TEMPERATURE_PROBS_MEASURED,
# beside its case's gate.
TEMPERATURE_PROBS_MEASURED = 5.125e-07  # 8.60 * 2^-24 at (1, 1, 1, 1, 5), B = 129, tau = 0.7: gate 2.103e-06 (Zmax 9.643)
TEMPERATURE_SHAPES = ((1, 1, 1, 1, 5), (17, 33, 33, 33, 5), (449, 129, 150, 128, 6))


def exact_logits(sd, x):
    """The exact nets' logits, bias included, as float32 (asserted exact) [B, A]."""
    hidden = []
    policy.reference_forward(sd, x, hidden=hidden)
    wq = sd["action_head.weight"].to(torch.bfloat16).to(torch.float64)
    lg = hidden[2][1] @ wq.T + sd["action_head.bias"].to(torch.float64)
    lg32 = lg.to(torch.float32)
    assert torch.equal(lg32.to(torch.float64), lg)
    return lg32.numpy()


@pytest.mark.parametrize("B", [1, 129])
@pytest.mark.parametrize("tau", [0.7, 1.5])
@pytest.mark.parametrize("shape", TEMPERATURE_SHAPES)
def test_general_temperature_on_exact_nets(shape, tau, B):
    F, A = shape[0], shape[4]
    sd = pc.exact_net(shape)
    x = pc.exact_features(B, F)
    pc.exact_certificate(sd, x)
    inv = np.float32(1.0) / np.float32(tau)
    lgp = exact_logits(sd, x) * inv
    assert lgp.dtype == np.float32
    z = lgp.astype(np.float64) - lgp.astype(np.float64).max(axis=1, keepdims=True)
    zmax = float(np.abs(z).max())
    assert zmax < 80
    p_ref = np.exp(z) / np.exp(z).sum(axis=1, keepdims=True)
    gate = 2.0 ** -20 + 2.0 ** -23 * zmax
    opts = pc.OPTS_REF if A == 5 else pc.OPTS_ODD
    env, _ = tgp.warmed_env(B, opts)
    pol = policy.DevicePolicy(sd, env)
    _, p_1, v_1 = act_all(pol, x)
    pol.set_action_rule("sample", tau)
    a, p, v = act_all(pol, x)
    ratio = float((np.abs(p.astype(np.float64) - p_ref) / p_ref).max())
    print("exact net %s B=%d tau=%g: worst |p - p_ref| / p_ref = %.3e (%.2f * 2^-24), gate %.3e, Zmax %.3f"
          % (shape, B, tau, ratio, ratio * 2.0 ** 24, gate, zmax))
    assert same_bits(v, v_1) and not same_bits(p, p_1)
    assert np.array_equal(a, policy.select_reference(p, *keys_of(env), mode="sample"))
    pol.set_action_rule("greedy", tau)
    a_g, p_g, v_g = act_all(pol, x)
    assert same_bits(p_g, p) and same_bits(v_g, v_1)
    assert np.array_equal(a_g, policy.select_reference(p_g, *keys_of(env), mode="greedy"))
    assert float(np.abs(p.astype(np.float64).sum(1) - 1).max()) <= 4 * A * 2.0 ** -23
    assert ratio <= gate, (shape, B, tau, ratio, gate)


# ------------------------------------------------------------------ 5. the fused rollout under greedy
def greedy_loop(B, sd=None):
    env, w, pol = closed_loop(B, arc.spread("ref") if sd is None else sd)
    pol.set_action_rule("greedy")
    return env, w, pol


def assert_greedy_segment(got, B, T):
    probs, acts = got["probs"].cpu().numpy(), got["actions"].cpu().numpy()
    for t in range(T):
        assert np.array_equal(acts[t], arc.first_max(probs[t])), t
    # max_turns = 5 and 3 warm-up steps: every env ends an episode inside the 6 steps
    assert bool((got["done"].cpu().numpy().sum(axis=0) >= 1).all())
    assert len(set(acts.flatten().tolist())) >= 3


@pytest.mark.parametrize("B", [65, 256])
def test_rollout_under_greedy_is_six_hand_made_steps(B):
    T = 6
    sd = arc.spread("ref")
    arc.assert_reference_spreads(sd, pc.ref_features(257))
    env0, w0, pol0 = greedy_loop(B)
    want = trp.manual_rollout(env0, w0, pol0, T)
    assert_greedy_segment(want, B, T)
    left = trp.left_behind(env0, w0)
    runs = {"loop": dict(fused=False)}
    runs["one launch" if B == 256 else "wrapper default"] = dict(fused=True if B == 256 else None)
    for what, kw in runs.items():
        env, w, pol = greedy_loop(B)
        assert trp.fused_flag(env, pol) == (1 if B == 256 else 0)
        got = w.rollout_policy(pol, T, return_probs=True, **kw)
        assert_same(got, want, what=what)
        trp.assert_left_behind(env, w, left)
        assert env.counters()["rollout_launches"] == (1 if kw["fused"] else 0), what
    # wab_rollout_policy itself (B = 65: its 2 T launches; B = 256: the one launch)
    env, w, pol = greedy_loop(B)
    feats, last = torch.zeros((T, B, 449), device=DEV), torch.zeros((B, 449), device=DEV)
    rc, got = trp.c_rollout(env, pol, w.observation().clone(), T, feats, last)
    assert rc == 0
    assert_same(got, want, what="wab_rollout_policy")
    assert torch.equal(last, w0.features)
    c = env.counters()
    assert (c["rollout_launches"], c["rollout_step_calls"]) == ((1, 0) if B == 256 else (0, 1))
    # packed rows: the same actions, the rows those of the float run
    env, w, pol = greedy_loop(B)
    packed = w.rollout_policy(pol, T, return_probs=True, store_features="packed")
    assert packed["features"] is None
    assert_same(packed, want, [k for k in KEYS if k != "features"], what="packed")
    ref_bits = torch.from_numpy(features.pack_reference(want["features"].cpu().numpy()))
    assert torch.equal(packed["feature_bits"].cpu(), ref_bits)
    # the sampled policy takes other actions on the same start
    env, w, pol = closed_loop(B, sd)
    sampled = w.rollout_policy(pol, T, return_probs=True)
    assert torch.equal(sampled["probs"][0], want["probs"][0])
    assert int((sampled["actions"][0] != want["actions"][0]).sum()) * 4 >= B


def test_back_to_sampling_is_a_fresh_policy():
    T, B = 6, 256
    env, w, pol = greedy_loop(B)
    pol.set_action_rule("greedy", 0.7)
    pol.set_action_rule("sample", 1.0)
    got = w.rollout_policy(pol, T, return_probs=True, fused=True)
    env2, w2, fresh = closed_loop(B, arc.spread("ref"))
    want = w2.rollout_policy(fresh, T, return_probs=True, fused=True)
    assert_same(got, want)
    trp.assert_left_behind(env, w, trp.left_behind(env2, w2))


def test_a_captured_graph_keeps_the_rule_it_was_captured_with():
    T, B = 6, 256
    env0, w0, pol0 = greedy_loop(B)
    want = w0.rollout_policy(pol0, T, return_probs=True, fused=True)  # eager (every kernel is loaded)
    assert_greedy_segment(want, B, T)
    env, w, pol = greedy_loop(B)
    snap, start = env.snapshot(), w.features.clone()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            got = w.rollout_policy(pol, T, return_probs=True, fused=True)
    torch.cuda.current_stream().wait_stream(side)
    pol.set_action_rule("sample", 0.7)  # host state: the graph's kernel arguments are already made
    for replay in range(2):
        if replay:
            env.restore(snap)
            w.features.copy_(start)
        g.replay()
        torch.cuda.synchronize()
        assert_same(got, want, what="replay %d" % replay)
        assert torch.equal(w.features, w0.features)
        for k, v in env0.state().items():
            assert np.array_equal(env.state()[k], v), (replay, k)
    assert pol.action_rule == ("sample", policy.check_action_rule("sample", 0.7)[1])


# ------------------------------------------------------------------ 6. sharding
@pytest.mark.parametrize("mode,tau", [("greedy", 1.0), ("sample", 0.7)])
def test_two_handles_give_the_actions_of_one(mode, tau):
    T = 6
    sd = arc.spread("ref")
    warm = pc.warm_actions(256, 5, trp.WARM)
    env, w, pol = closed_loop(256, sd, warm=warm)
    pol.set_action_rule(mode, tau)
    whole = w.rollout_policy(pol, T, return_probs=True, fused=True)
    parts = []
    for lo in (0, 128):
        e, ww, pp = closed_loop(128, sd, base=lo, warm=warm[:, lo:lo + 128])
        pp.set_action_rule(mode, tau)
        parts.append((ww.rollout_policy(pp, T, return_probs=True, fused=True), ww, pp))
    for k in KEYS:
        assert torch.equal(torch.cat([p[0][k] for p in parts], dim=1), whole[k]), k
    assert torch.equal(torch.cat([p[1].features for p in parts], dim=0), w.features)
    assert len(set(whole["actions"].cpu().numpy().flatten().tolist())) >= 3 and int(whole["done"].sum()) > 0
    # and one act() of each on the features the rollouts left
    a_whole = pol.act(w.features).cpu().numpy()
    a_parts = np.concatenate([pp.act(ww.features).cpu().numpy() for _, ww, pp in parts])
    assert np.array_equal(a_parts, a_whole) and len(set(a_whole.tolist())) >= 2


# ------------------------------------------------------------------ 7. what ignores the rule
def test_evaluate_and_the_gradients_ignore_the_rule():
    N = 130
    sd = arc.spread("ref")
    env, _ = tgp.warmed_env(64)
    pol = policy.DevicePolicy(sd, env)
    rng = np.random.RandomState(5)
    x = torch.as_tensor(pc.ref_features(257)[:N].copy(), device=DEV)
    acts = torch.as_tensor(rng.randint(5, size=N).astype(np.int8), device=DEV)
    weight = torch.as_tensor(rng.standard_normal(N).astype(np.float32), device=DEV)
    target = torch.as_tensor(rng.standard_normal(N).astype(np.float32), device=DEV)

    def run():
        ev = pol.evaluate(x, acts)
        old = (ev["logp"] - torch.as_tensor(rng_noise, device=DEV)).contiguous()
        lg = pol.loss_and_grad(x, acts, weight, target, entropy_coef=0.01, return_rows=True)
        pp = pol.ppo_loss_and_grad(x, acts, weight, target, old, clip=0.2, old_value=ev["value"], value_clip=0.2,
                                   entropy_coef=0.01, return_rows=True)
        pol.check()
        flat = {}
        for name, out in (("evaluate", ev), ("grad", lg), ("ppo", pp)):
            for k, v in out.items():
                if k == "grads":
                    for n, gt in v.items():
                        flat["%s.grads.%s" % (name, n)] = gt.cpu().numpy()
                else:
                    flat["%s.%s" % (name, k)] = v.cpu().numpy()
        return flat

    rng_noise = (0.05 * rng.standard_normal(N)).astype(np.float32)
    want = run()
    assert len(want) > 40 and float(np.abs(want["grad.grads.action_head.weight"]).max()) > 0
    with pol.acting(mode="greedy", temperature=0.5):
        got = run()
        _, p_half, _ = act_all(pol, pc.ref_features(64))
    for k, v in want.items():
        assert same_bits(got[k], v), k
    _, p_one, _ = act_all(pol, pc.ref_features(64))
    assert not same_bits(p_half, p_one)  # (the rule was live: act() followed it)
