"""env.snapshot() / env.restore() (wab_snapshot_save / wab_snapshot_restore) against the C oracle.

Every draw is keyed by (seed, global env id, episode, ...), so a restored env continues the one
timeline the oracle runs straight through: the oracle never rewinds, and an env restored to step
K must give the oracle's steps K+1, K+2, ... again.  All comparisons are bit for bit.

The set-up shared by the tests: seed 0x5EED, env_id_base 1000, 144 envs (two full 64-env groups
and 16 envs; 144 * 363 is a multiple of 16, so rollout() is one launch), the actions of step
t = 1, 2, ... drawn in that order from RandomState(7).randint(n_actions, size=144)."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEED, BASE, B = 0x5EED, 1000, 144
T = 20
N_STEPS = 85  # no test takes more

OPTION_SETS = {
    # name: (options, env kwargs, stride of the kernel under test, that kernel, snapshot step K)
    "default": ({}, {}, 0, "small", 45),
    "wolfy": ({"chance_wolf_on_square": 0.03, "wolf_chance_to_despawn": 0.2, "wolf_spawn_margin": 2},
              {"wolf_slots": 32}, 0, "small", 45),
    "31x31": ({"width": 31, "height": 31}, {}, 32, "wide", 45),
    "rect9x13": ({"width": 13, "height": 11, "turns_to_fill_food": 4, "turns_to_empty_food": 30,
                  "max_turns": 60, "reward_for_eating": 0.25, "bush_power": 60}, {}, 11, "block", 23),
}


class Record:
    """What the oracle saw: entry t is the state after step t (0: after the reset)."""

    def __init__(self, name, stride):
        from oracle.oracle import OracleBatch
        from wab_gym_amd.options import default_game_options

        opts = dict(default_game_options)
        opts.update(OPTION_SETS[name][0])
        self.opts = opts
        orc = OracleBatch(opts, B, SEED, BASE, plane_stride=stride)
        rng = np.random.RandomState(7)
        self.actions = [None]
        self.steps = []
        orc.reset()
        self._keep(orc, first=True)
        for _ in range(N_STEPS):
            a = rng.randint(orc.n_actions, size=B)
            self.actions.append(a)
            orc.step(a)
            self._keep(orc)
        # envs that got a reward_for_eating reward earlier in the episode they are in at step t
        r_eat = float(opts["reward_for_eating"])
        others = [float(opts[k]) for k in ("reward_per_turn", "reward_for_finishing", "reward_for_starving",
                                           "reward_for_being_killed")]
        eat_rewards = {np.float32((0.0 + r_eat) + x) for x in others} - {np.float32(0.0 + x) for x in others}
        ate = np.zeros(B, bool)
        self.ate = [ate.copy()]
        for t in range(1, N_STEPS + 1):
            s = self.steps[t]
            ate = (ate | np.isin(s["reward"], list(eat_rewards))) & ~s["done"].astype(bool)
            self.ate.append(ate.copy())

    def _keep(self, orc, first=False):
        s = dict(planes=orc.planes.copy(), scalars=np.stack([orc.food_turns, orc.role, orc.status]),
                 state={k: v.copy() for k, v in orc.state().items()})
        if not first:
            s.update(reward=orc.reward.copy(), done=orc.done.copy(), t_planes=orc.t_planes.copy(),
                     t_scalars=np.stack([orc.t_food_turns, orc.t_role, orc.t_status]))
        self.steps.append(s)

    def mixed(self, times):
        """The entry whose env i row is that of step times[i]."""
        out = {}
        for key in ("planes", "reward", "done", "t_planes"):
            out[key] = np.stack([self.steps[t][key][i] for i, t in enumerate(times)])
        for key in ("scalars", "t_scalars"):
            out[key] = np.stack([self.steps[t][key][:, i] for i, t in enumerate(times)], axis=1)
        out["state"] = {k: np.array([self.steps[t]["state"][k][i] for i, t in enumerate(times)])
                        for k in self.steps[0]["state"]}
        return out


@functools.lru_cache(maxsize=None)
def record(name, stride=0):
    return Record(name, stride)


def make_env(name, stride=0, n=B, base=BASE, return_terminal=True, seed=SEED, **kw):
    from wab_gym_amd.env import BatchedWolvesAndBushesEnv

    opts, env_kw = OPTION_SETS[name][:2]
    args = dict(env_kw)
    args.update(kw)
    return BatchedWolvesAndBushesEnv(opts or None, num_envs=n, seed=seed, device="cuda:0", env_id_base=base,
                                     return_terminal=return_terminal, plane_stride=stride, **args)


def host(x):
    return x.cpu().numpy()


def check_obs(env, want, rows=slice(None), what=""):
    """The env's own obs buffer and hidden state against an oracle entry (rows of the oracle's batch)."""
    assert np.array_equal(host(env._obs["planes"]), want["planes"][rows]), "planes differ " + what
    assert np.array_equal(host(env._obs["scalars"]), want["scalars"][:, rows]), "obs scalars differ " + what
    st = env.state()
    for k, v in want["state"].items():
        a, b = st[k], v[rows]
        if k == "food":
            a, b = a.view(np.uint64), b.view(np.uint64)
        assert np.array_equal(a, b), "state %s differs %s" % (k, what)


def check_step(env, want, rows=slice(None), what=""):
    """Everything one step() returned, against an oracle entry."""
    check_obs(env, want, rows, what)
    assert np.array_equal(host(env.reward).view(np.uint32), want["reward"][rows].view(np.uint32)), "reward " + what
    done = want["done"][rows].astype(bool)
    assert np.array_equal(host(env.done).astype(bool), done), "done differs " + what
    if env.terminal_observation is not None:
        term = env.terminal_observation
        assert np.array_equal(host(term["planes"])[done], want["t_planes"][rows][done]), "terminal planes " + what
        assert np.array_equal(host(term["scalars"])[:, done], want["t_scalars"][:, rows][:, done]), \
            "terminal scalars " + what


def check_counters(env):
    c = env.counters()
    assert c["wolf_overflow"] == 0 and c["eaten_overflow"] == 0 and c["handoff_timeouts"] == 0, c


def run_steps(env, rec, t0, t1, rows=slice(None)):
    """step() for t = t0+1 .. t1, each compared with the oracle's step t."""
    import torch

    for t in range(t0 + 1, t1 + 1):
        env.step(torch.as_tensor(rec.actions[t][rows]))
        check_step(env, rec.steps[t], rows, "at step %d" % t)


def start(name, stride, K, **kw):
    env = make_env(name, stride, **kw)
    rec = record(name, stride)
    env.reset()
    check_obs(env, rec.steps[0], what="after reset")
    run_steps(env, rec, 0, K)
    return env, rec


def assert_interesting(rec, K, name):
    """The snapshot step holds the state a wrong restore would lose: several wolves, a later
    episode, a partly eaten bush (an eaten-log entry)."""
    st = rec.steps[K]["state"]
    assert (st["n_wolves"] >= 2).any(), name
    assert (st["episode"] > 0).any(), name
    assert rec.ate[K].any(), name


@pytest.mark.parametrize("name", list(OPTION_SETS))
def test_rewind_per_step(name):
    _, _, stride, kernel, K = OPTION_SETS[name]
    env, rec = start(name, stride, K)
    assert env.step_kernel == kernel
    assert_interesting(rec, K, name)
    snap = env.snapshot()
    assert snap.count == B and snap.env_id_first == BASE and tuple(snap.records.shape) == (B, snap.record_bytes)
    run_steps(env, rec, K, K + T)
    obs = env.restore(snap)
    want = rec.steps[K]
    H = env.H
    for k in range(3):
        assert np.array_equal(host(obs[k]), want["planes"][:, k, :, :H]), "restore() obs grid %d" % k
    for k in range(3):
        assert np.array_equal(host(obs[3 + k]), want["scalars"][k])
    check_step(env, want, what="after restore")
    run_steps(env, rec, K, K + T)
    check_counters(env)


def test_rewind_with_large_records():
    """32 wolf slots and an eaten log of 253 entries (no multiple of 4: its bytes are padded):
    records of 1440 bytes, which go through the kernels' LDS in passes of 16 envs."""
    import ctypes

    from wab_gym_amd import _lib

    name, K = "default", OPTION_SETS["default"][4]
    env, rec = start(name, 0, K, wolf_slots=32, eaten_capacity=253)
    assert _lib.load().wab_snapshot_bytes(ctypes.addressof(env.cfg)) == 1440
    assert 64 * 1440 > 2 * 40 * 1024  # (two halvings: wab_capi.hip snapshot_params)
    snap = env.snapshot()
    # the same state in a handle of the default slots: its live entries are the same bytes
    small = make_env(name)
    small.reset()
    run_steps(small, rec, 0, K)
    big, ref = host(snap.records), host(small.snapshot().records)
    assert np.array_equal(big[:, :24 + 4 * 8], ref[:, :24 + 4 * 8])  # hdr, food, wolf slots 0..7
    assert not big[:, 24 + 4 * 8:24 + 4 * 32].any()                  # (no env has more than 3 wolves)
    assert np.array_equal(big[:, 24 + 4 * 32:][:, :4 * 80], ref[:, 24 + 4 * 8:][:, :4 * 80])  # eaten tiles
    assert np.array_equal(big[:, -16 - 4:-4], ref[:, -16 - 8:-8])    # the bitmap's 4 dwords
    run_steps(env, rec, K, K + T)
    env.restore(snap)
    check_step(env, rec.steps[K], what="after restore")
    run_steps(env, rec, K, K + T)
    check_counters(env)


def rollout_and_check(env, rec, t0, t1):
    import torch

    planes, scal, rew, done = env.rollout(torch.as_tensor(np.stack(rec.actions[t0 + 1:t1 + 1])))
    for i, t in enumerate(range(t0 + 1, t1 + 1)):
        w = rec.steps[t]
        assert np.array_equal(host(planes[i]), w["planes"]), "rollout planes at step %d" % t
        assert np.array_equal(host(scal[i]), w["scalars"]), "rollout scalars at step %d" % t
        assert np.array_equal(host(rew[i]).view(np.uint32), w["reward"].view(np.uint32)), "rollout reward %d" % t
        assert np.array_equal(host(done[i]), w["done"]), "rollout done at step %d" % t
    check_obs(env, rec.steps[t1], what="after the rollout to step %d" % t1)


@pytest.mark.parametrize("name", ["default", "31x31"])
def test_rewind_across_paths(name):
    """A snapshot taken between step() calls continues under rollout() and the other way round."""
    _, _, stride, kernel, K = OPTION_SETS[name]
    env, rec = start(name, stride, K, return_terminal=False)
    assert env.step_kernel == kernel
    assert_interesting(rec, K, name)
    snap = env.snapshot()
    rollout_and_check(env, rec, K, K + T)
    env.restore(snap)
    check_step(env, rec.steps[K], what="after restore")
    run_steps(env, rec, K, K + T)
    # a snapshot right after a rollout, restored before the next one
    rollout_and_check(env, rec, K + T, K + T + 10)
    snap2 = env.snapshot()
    rollout_and_check(env, rec, K + T + 10, K + T + 20)
    env.restore(snap2)
    check_step(env, rec.steps[K + T + 10], what="after the second restore")
    rollout_and_check(env, rec, K + T + 10, K + T + 20)
    c = env.counters()
    assert c["rollout_launches"] == 4 and c["rollout_step_calls"] == 0, c
    check_counters(env)


@pytest.mark.parametrize("name", ["default", "31x31"])
def test_masked_restore(name):
    """Only the odd envs go back to step K; the even ones go on from step K + T untouched."""
    import torch

    _, _, stride, _, K = OPTION_SETS[name]
    env, rec = start(name, stride, K)
    assert_interesting(rec, K, name)
    snap = env.snapshot()
    run_steps(env, rec, K, K + T)
    mask = np.arange(B) % 2 == 1
    env.restore(snap, mask=torch.as_tensor(mask))
    for j in range(T + 1):
        times = np.where(mask, K + j, K + T + j)
        if j > 0:
            a = np.where(mask, rec.actions[K + j], rec.actions[K + T + j])
            env.step(torch.as_tensor(a))
        check_step(env, rec.mixed(times), what="%d steps after the masked restore" % j)
    check_counters(env)


def test_restore_into_other_handles_resharded(tmp_path):
    """Snapshot -> host -> file -> two fresh, never-reset envs of 72 envs each."""
    import torch

    from wab_gym_amd import EnvSnapshot

    name = "default"
    K = OPTION_SETS[name][4]
    env, rec = start(name, 0, K)
    assert_interesting(rec, K, name)
    path = tmp_path / "envs.snapshot"
    env.snapshot().cpu().save(path)
    env.close()
    snap = EnvSnapshot.load(path)
    assert snap.device.type == "cpu" and snap.count == B
    halves = []
    for s in range(2):
        rows = slice(72 * s, 72 * s + 72)
        half = make_env(name, 0, n=72, base=BASE + 72 * s)
        half.restore(snap)
        check_step(half, rec.steps[K], rows, "after restore into shard %d" % s)
        halves.append((half, rows))
    for t in range(K + 1, K + T + 1):
        for half, rows in halves:
            half.step(torch.as_tensor(rec.actions[t][rows]))
            check_step(half, rec.steps[t], rows, "at step %d" % t)
    for half, _ in halves:
        check_counters(half)


@pytest.mark.parametrize("name,src,dst", [
    ("default", (0, "small"), (16, "wide")),
    ("default", (16, "wide"), (0, "small")),
    ("rect9x13", (11, "block"), (16, "wide")),
    ("rect9x13", (16, "wide"), (11, "block")),
    ("31x31", (32, "wide"), (31, "block")),
])
def test_restore_across_kernels(name, src, dst):
    """The record does not depend on the step kernel: a snapshot of a handle one kernel steps
    continues in a handle another kernel steps (another plane_stride), and the two handles,
    stepped on side by side, save the same bytes."""
    import torch

    K = OPTION_SETS[name][4]
    a, rec_a = start(name, src[0], K)
    assert a.step_kernel == src[1]
    assert_interesting(rec_a, K, name)
    snap = a.snapshot()
    b = make_env(name, dst[0])
    assert b.step_kernel == dst[1]
    rec_b = record(name, dst[0])
    b.restore(snap)
    check_step(b, rec_b.steps[K], what="after restore into the %s kernel's handle" % dst[1])
    assert np.array_equal(host(b.snapshot().records), host(snap.records))
    run_steps(b, rec_b, K, K + T)
    run_steps(a, rec_a, K, K + T)
    assert np.array_equal(host(a.snapshot().records), host(b.snapshot().records))
    check_counters(a)
    check_counters(b)


def test_refusals_leave_the_env_as_it_was():
    import torch

    from wab_gym_amd import (BatchedWolvesAndBushesEnvEgoCentric,
                             BatchedWolvesAndBushesEnvEgocentricJustBushes)

    name, K = "default", 10
    env, rec = start(name, 0, K)
    t = K

    def refused(other, exc, word):
        nonlocal t
        other.reset()
        other.step(torch.as_tensor(rec.actions[1]))
        with pytest.raises(exc, match=word):
            env.restore(other.snapshot())
        other.close()
        run_steps(env, rec, t, t + 1)  # the env is as it was: its next step is the oracle's
        t += 1

    refused(make_env(name, seed=SEED + 1), ValueError, "seed")
    from wab_gym_amd.env import BatchedWolvesAndBushesEnv
    refused(BatchedWolvesAndBushesEnv({"max_turns": 81}, num_envs=B, seed=SEED, device="cuda:0", env_id_base=BASE),
            ValueError, "config_hash")
    refused(make_env(name, wolf_slots=16), ValueError, "config_hash")
    refused(make_env(name, base=BASE + 4 * B), ValueError, "intersect")

    fresh = make_env(name)
    with pytest.raises(RuntimeError):
        fresh.snapshot()
    with pytest.raises(RuntimeError):
        fresh.restore(env.snapshot(), mask=torch.ones(B, dtype=torch.bool))
    with pytest.raises(RuntimeError):  # nor a part of its envs
        fresh.restore(env.snapshot(envs=(0, 64)))
    fresh.reset()
    check_obs(fresh, rec.steps[0], what="after the refused calls and a reset")
    run_steps(fresh, rec, 0, 2)

    snap = env.snapshot()
    for cls in (BatchedWolvesAndBushesEnvEgoCentric, BatchedWolvesAndBushesEnvEgocentricJustBushes):
        ego = cls(num_envs=B, seed=SEED, device="cuda:0", env_id_base=BASE)
        ego.reset()
        with pytest.raises(NotImplementedError):
            ego.snapshot()
        with pytest.raises(NotImplementedError):
            ego.restore(snap)
        ego.close()
    run_steps(env, rec, t, t + 2)
    check_counters(env)
