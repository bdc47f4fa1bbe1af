"""The small kernel's default-rules instances (wab_step_small<8, 11, .., RULES = true>) and their
selection at wab_create.

A handle whose geometry is the default 11x11, with 8 wolf slots, and whose resolved rule fields
all equal the default options' takes instances that have those fields as constants
(wab_default_rules.h); their multi-step build reads the launch's parameters once and advances
the I/O slices by one step per step.  Every other handle takes the generic instances.  Each
test compares every output of every step, bit for bit, with the C oracle (oracle/wab_oracle.c):
a wrong constant, a slice advanced wrongly, or a selection that lets a non-default option
through shows as a mismatch.
"""
import numpy as np
import pytest

from backends import SEED

pytestmark = pytest.mark.gpu


def _env(opts, B, **kw):
    from wab_gym_amd.env import BatchedWolvesAndBushesEnv

    kw.setdefault("autoreset", True)
    env = BatchedWolvesAndBushesEnv(opts, num_envs=B, seed=SEED, device="cuda:0", validate_actions=False, **kw)
    env.reset()
    return env


def _oracle(opts, B, autoreset=True):
    from oracle.oracle import OracleBatch

    orc = OracleBatch(opts, B, SEED, 0, autoreset, 0)
    orc.reset()
    return orc


def _actions(seed, T, B, n_actions):
    return np.random.RandomState(seed).randint(n_actions, size=(T, B)).astype(np.int8)


def _eq(got, want, what):
    got = got.cpu().numpy()
    want = np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not np.array_equal(got, want.astype(got.dtype)):
        bad = np.argwhere(got != want.astype(got.dtype))[:4].tolist()
        raise AssertionError("%s differs at %s" % (what, bad))


def _rollout_vs_oracle(env, orc, a, what):
    """One wab_rollout launch of a.shape[0] steps: planes, scalars, f32 reward and done of every
    step against the oracle's step."""
    import torch

    before = env.counters()
    planes, scal, rew, done = env.rollout(torch.as_tensor(a))
    assert env.counters()["rollout_launches"] - before["rollout_launches"] == 1, "not the one-launch path"
    for t in range(a.shape[0]):
        w = "%s step %d " % (what, t)
        op, of, orl, ost, orew, odone = orc.step(a[t])
        _eq(planes[t], op, w + "planes")
        _eq(scal[t], np.stack([of, orl, ost]), w + "scalars")
        _eq(rew[t], orew, w + "reward")
        _eq(done[t], odone, w + "done")


def _state_vs_oracle(env, orc):
    gs, os_ = env.state(), orc.state()
    for key in ("x", "y", "turn", "n_wolves", "episode"):
        assert np.array_equal(gs[key], os_[key]), key
    assert np.array_equal(gs["food"].view(np.uint64), os_["food"].view(np.uint64))
    c = env.counters()
    assert c["wolf_overflow"] == 0 and c["eaten_overflow"] == 0 and c["handoff_timeouts"] == 0, c


def test_default_rollouts_chained_then_steps():
    """Default options, B = 80 (a whole group and a partial one), T = 5, three chained launches:
    the slices advance four times per launch, the last step's state write-back and step 0's
    reload are crossed twice.  The same handle then takes T wab_step calls (the per-step
    default-rules instance)."""
    import torch

    B, T = 80, 5
    env, orc = _env(None, B), _oracle(None, B)
    assert env.step_kernel == "small"
    for k in range(3):
        _rollout_vs_oracle(env, orc, _actions(100 + k, T, B, env.n_actions), "launch %d" % k)
    a = _actions(199, T, B, env.n_actions)
    for t in range(T):
        w = "wab_step %d " % t
        obs, rew, done, _ = env.step(torch.as_tensor(a[t]))
        op, of, orl, ost, orew, odone = orc.step(a[t])
        _eq(env._obs["planes"], op, w + "planes")
        _eq(env._obs["scalars"], np.stack([of, orl, ost]), w + "scalars")
        _eq(rew, orew, w + "reward")
        _eq(done.to(torch.uint8), odone, w + "done")
    _state_vs_oracle(env, orc)


@pytest.mark.parametrize("T", [1, 2])
def test_default_rollout_first_and_last_step(T):
    """T = 1 (the per-step launch) and T = 2 (step 0 and the last step with nothing between) at
    B = 64, two launches each."""
    B = 64
    env, orc = _env(None, B), _oracle(None, B)
    for k in range(2):
        _rollout_vs_oracle(env, orc, _actions(300 + 10 * T + k, T, B, env.n_actions), "T %d launch %d" % (T, k))
    _state_vs_oracle(env, orc)


@pytest.mark.parametrize("store_planes", [True, False])
def test_default_rollout_features(store_planes):
    """wab_rollout_features at B = 80, T = 3, two launches, with and without planes (both arms of
    the slices' null tests): features, scalars, reward, done and the discounted returns against
    the oracle."""
    import torch

    from oracle import oracle as O
    from test_featurizer_oracle import step_reward_values

    B, T = 80, 3
    env, orc = _env(None, B), _oracle(None, B)
    vm = np.zeros((B, 11, 11), np.uint8)
    for k in range(2):
        a = _actions(500 + k, T, B, env.n_actions)
        r = env.rollout_features(torch.as_tensor(a), gamma=0.99, store_planes=store_planes)
        assert (r["planes"] is not None) == store_planes
        rew = np.zeros((T, B), np.float32)
        done = np.zeros((T, B), np.uint8)
        for t in range(T):
            w = "launch %d step %d " % (k, t)
            op, of, orl, ost, orew, odone = orc.step(a[t])
            if store_planes:
                _eq(r["planes"][t], op, w + "planes")
            _eq(r["features"][t], O.featurize(op, of, orl, ost, vm, 11, 11), w + "features")
            _eq(r["scalars"][t], np.stack([of, orl, ost]), w + "scalars")
            _eq(r["reward"][t], orew, w + "reward")
            _eq(r["done"][t], odone, w + "done")
            rew[t], done[t] = orew, odone
        _eq(r["returns"], O.discounted_returns(rew, done, 0.99, None, exact_values=step_reward_values()),
            "launch %d returns" % k)
    _state_vs_oracle(env, orc)


# one departure from the default each: (options, env keywords)
DEPARTURES = {
    "reward_for_eating": ({"reward_for_eating": 0.25}, {}),
    "reward_per_turn": ({"reward_per_turn": 0.5}, {}),
    "max_turns": ({"max_turns": 4}, {}),
    "turns_to_empty_food": ({"turns_to_empty_food": 30}, {}),
    "turns_to_fill_food": ({"turns_to_fill_food": 4}, {}),
    "bush_power": ({"bush_power": 50}, {}),
    "max_berries_per_bush": ({"max_berries_per_bush": 100}, {}),
    "chance_wolf_on_square": ({"chance_wolf_on_square": 0.01}, {}),
    "wolf_chance_to_despawn": ({"wolf_chance_to_despawn": 0.2}, {}),
    "lookout_only": ({"lookout_only": False}, {}),
    "gatherer_only": ({"lookout_only": False, "gatherer_only": True}, {}),
    "restrict_view": ({"restrict_view": True}, {}),
    "wolves": ({"wolves": False}, {}),
    "wolves_can_move": ({"wolves_can_move": False}, {}),
    "god_mode": ({"god_mode": True}, {}),
    "autoreset": ({}, {"autoreset": False}),
    "starting_food_random": ({"starting_food": None}, {}),
    "starting_role_random": ({"starting_role": None}, {}),
    "starting_role": ({"starting_role": 0}, {}),
    "wolf_slots": ({}, {"wolf_slots": 16}),
    "eaten_capacity": ({}, {"eaten_capacity": 120}),
}


@pytest.mark.parametrize("name", sorted(DEPARTURES))
def test_single_departure_takes_a_generic_instance(name):
    """One option away from the default, B = 80, T = 3, two launches against the oracle: the
    handle must not take the default-rules instances (their constants would then show as a
    mismatch)."""
    opts, kw = DEPARTURES[name]
    B, T = 80, 3
    env, orc = _env(opts or None, B, **kw), _oracle(opts or None, B, kw.get("autoreset", True))
    assert env.step_kernel == "small"
    for k in range(2):
        _rollout_vs_oracle(env, orc, _actions(700 + k, T, B, env.n_actions), "%s launch %d" % (name, k))
    _state_vs_oracle(env, orc)
