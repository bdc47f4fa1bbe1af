"""Episode statistics and per-episode normalisation of whole [T, B] rollout segments on device
(wab_episode_stats_update, wab_normalize_episode_returns; EpisodeStats.update_rollout,
EpisodeMonitor's rollout methods, normalized_returns).

The yardstick of the accounting is EpisodeStats.update run step by step on CPU tensors (the
per-step path, unchanged): the running return by its bits, the running length, the count and the
four record arrays, order included.  The yardstick of the normalisation is `restated_normalise`
below, the contract in sequential float64, one Python float operation at a time."""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

import golden_replay as gr
import policy_cases as pc
import returns_cases as rc
from wab_gym_amd import _lib, policy
from wab_gym_amd.env import BatchedWolvesAndBushesEnv
from wab_gym_amd.monitor import EpisodeMonitor, EpisodeStats, reward_table
from wab_gym_amd.options import default_game_options
from wab_gym_amd.wrappers import PragmaticObsWrapper, discounted_returns, normalized_returns

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# B below, at and across a wave (64) and a workgroup of the count kernel (256 threads); T below,
# at and above the walk's load chunk (32); 64 x 257 and 129 x 1000 are count tables of 320 and
# 2064 entries, more than one tile of 256; the normalisation takes its LDS kernel up to T = 128
# and the other one at 129
SHAPES = [(1, 1), (1, 64), (33, 65), (64, 257), (129, 1000), (5, 4097)]
DENSITIES = [0.0, 0.03, 0.5, 1.0]
# a count table of 66003 entries: 258 tiles, so the scan of the tile sums (256 per pass) carries
# from one pass into the next
MANY_TILES = (3, 64 * 22000 + 37)
# the default options' rewards (float32 of 0, 0.1, 1, 1.1, -0.9 = 0.1 + -1, -1) and arbitrary floats
REWARDS = np.array([0.0, 0.1, 1.0, 1.1, -0.9, -1.0, 0.25, 3.3, -1e-3], dtype=np.float32)


@functools.lru_cache(maxsize=None)
def handle_env():
    """an env of the default options: its handle carries their reward table"""
    return BatchedWolvesAndBushesEnv(num_envs=64, seed=1, device=DEV)


def make_segment(T, B, density, seed=0):
    rng = np.random.RandomState(1000 * T + B + seed)
    reward = REWARDS[rng.randint(len(REWARDS), size=(T, B))]
    done = rng.random_sample((T, B)) < density if 0.0 < density < 1.0 else np.full((T, B), density >= 1.0)
    return reward, done


def per_step_reference(reward, done, ret=None, length=None, options=default_game_options):
    """T EpisodeStats.update calls on CPU tensors, flushed after every step so that each episode's
    step is known: (records dict, ret f64 [B], length i64 [B])."""
    T, B = reward.shape
    st = EpisodeStats(options, B, "cpu", flush_every=1)
    if ret is not None:
        st.ret.copy_(torch.as_tensor(ret))
        st.length.copy_(torch.as_tensor(length))
    r, d = torch.as_tensor(reward), torch.as_tensor(done)
    steps = []
    for t in range(T):
        n = len(st.episode_rewards)
        st.update(r[t], d[t])
        steps.extend([t] * (len(st.episode_rewards) - n))
    rec = {"return": np.array(st.episode_rewards, np.float64), "length": np.array(st.episode_lengths, np.int32),
           "env": np.array(st.episode_envs, np.int32), "step": np.array(steps, np.int32)}
    return rec, st.ret.numpy().copy(), st.length.numpy().copy()


@functools.lru_cache(maxsize=None)
def case(T, B, density):
    reward, done = make_segment(T, B, density)
    return (reward, done) + per_step_reference(reward, done)


GUARD = 5  # elements past `capacity`, which the call must leave as they are


def device_update(reward, done, capacity, ret=None, length=None, exact=True, null_records=False, handle=None):
    """One wab_episode_stats_update call: (count [2], records dict of the arrays' first
    `capacity` elements, the guard elements past them, ret, length)."""
    T, B = reward.shape
    L = _lib.load()
    r = torch.as_tensor(np.ascontiguousarray(reward), device=DEV)
    d = torch.as_tensor(np.ascontiguousarray(done).view(np.uint8), device=DEV)  # (nonzero bytes as they are)
    ret = torch.zeros(B, dtype=torch.float64, device=DEV) if ret is None else torch.as_tensor(ret, device=DEV)
    length = torch.zeros(B, dtype=torch.int64, device=DEV) if length is None else torch.as_tensor(length, device=DEV)
    nbytes = int(L.wab_episode_stats_workspace(T, B))
    assert nbytes >= 0
    ws = torch.empty(nbytes // 8 + 1, dtype=torch.int64, device=DEV)
    ep_ret = torch.full((capacity + GUARD,), -7.0, dtype=torch.float64, device=DEV)
    ep_i32 = torch.full((3, capacity + GUARD), -7, dtype=torch.int32, device=DEV)
    count = torch.full((2,), -1, dtype=torch.int64, device=DEV)
    ptrs = [None] * 4 if null_records else [ep_ret.data_ptr()] + [ep_i32[k].data_ptr() for k in range(3)]
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    if handle is None and exact:
        handle = handle_env()._h
    _lib.check(L.wab_episode_stats_update(handle, r.data_ptr() if T else None,
                                          d.data_ptr() if T else None, T, B, ret.data_ptr(), length.data_ptr(),
                                          *ptrs, capacity, count.data_ptr(), ws.data_ptr(), stream),
               "wab_episode_stats_update")
    i32 = ep_i32.cpu().numpy()
    rec = {"return": ep_ret.cpu().numpy()[:capacity], "length": i32[0, :capacity], "env": i32[1, :capacity],
           "step": i32[2, :capacity]}
    guard = np.concatenate([ep_ret.cpu().numpy()[capacity:], i32[:, capacity:].ravel().astype(np.float64)])
    return count.cpu().numpy(), rec, guard, ret.cpu().numpy(), length.cpu().numpy()


def assert_records(got, want, n=None):
    for k in ("step", "env", "length"):
        assert np.array_equal(got[k][:n], want[k][:n]), k
    assert np.array_equal(got["return"][:n].view(np.uint64), want["return"][:n].view(np.uint64))


def assert_state(ret, length, want_ret, want_length):
    assert np.array_equal(ret.view(np.uint64), want_ret.view(np.uint64))
    assert np.array_equal(length, want_length)


# ------------------------------------------------------------------ 1. accounting
@pytest.mark.parametrize("density", DENSITIES)
@pytest.mark.parametrize("T,B", SHAPES)
def test_accounting_equals_the_per_step_updates(T, B, density):
    reward, done, want, want_ret, want_len = case(T, B, density)
    finished = len(want["step"])
    assert finished == int(done.sum())  # (all done: T * B records, the capacity exactly met)
    count, rec, guard, ret, length = device_update(reward, done, finished)
    assert count.tolist() == [finished, finished]
    assert_records(rec, want)
    assert (guard == -7).all()
    assert_state(ret, length, want_ret, want_len)


def test_accounting_with_more_tiles_than_one_scan_pass():
    T, B = MANY_TILES
    assert -(-(T * -(-B // 64)) // 256) > 256
    reward, done = make_segment(T, B, 0.03)
    want, want_ret, want_len = per_step_reference(reward, done)
    finished = len(want["step"])
    count, rec, guard, ret, length = device_update(reward, done, finished)
    assert count.tolist() == [finished, finished]
    assert_records(rec, want)
    assert (guard == -7).all()
    assert_state(ret, length, want_ret, want_len)


@pytest.mark.parametrize("name", [n for n, _, _ in rc.OPTION_SETS])
def test_accounting_with_every_reward_table_size(name):
    """The walk kernel has one instance per number of inexact table entries (0 to 4, and 8 for 5
    to 8), as the returns scan: tests/returns_cases.py's option sets select each, and its
    segments hold the set's rewards, arbitrary floats, -0.0 and done bytes 1, 0x80 and 0xFF."""
    options = dict(default_game_options)
    options.update(rc.options_of(name))
    env = BatchedWolvesAndBushesEnv(options, num_envs=64, seed=1, device=DEV)
    values = [f for f, _ in reward_table(options)]
    inexact = sum(1 for f, d in reward_table(options) if f != d)
    assert inexact == rc.INEXACT[name]
    reward, done, _ = rc.make_case(40, 100, (values * 8)[:8], bootstrap=False)
    want, want_ret, want_len = per_step_reference(reward, done, options=options)
    finished = len(want["step"])
    assert finished == int((done != 0).sum()) > 300
    count, rec, guard, ret, length = device_update(reward, done, finished, handle=env._h)
    assert count.tolist() == [finished, finished]
    assert_records(rec, want)
    assert (guard == -7).all()
    assert_state(ret, length, want_ret, want_len)


def test_an_empty_segment_counts_nothing_and_keeps_the_state():
    ret0, len0 = np.array([0.5, -2.0, 0.0]), np.array([3, 0, 9], np.int64)
    count, _, guard, ret, length = device_update(np.zeros((0, 3), np.float32), np.zeros((0, 3), bool), 4, ret0, len0)
    assert count.tolist() == [0, 0] and (guard == -7).all()
    assert_state(ret, length, ret0, len0)


# ------------------------------------------------------------------ 2. carried state
def test_two_calls_equal_one_call_and_the_per_step_path():
    T, B, cut = 50, 130, 23
    reward, done = make_segment(T, B, 0.08, seed=7)
    done[cut - 4:cut + 4, 0] = False          # env 0's episode spans the split
    done[cut + 4, 0] = True
    want, want_ret, want_len = per_step_reference(reward, done)
    n = len(want["step"])
    count, one, _, ret1, len1 = device_update(reward, done, n)
    assert count.tolist() == [n, n]
    ca, a, _, ret_a, len_a = device_update(reward[:cut], done[:cut], n)
    assert len_a[0] >= 4
    cb, b, _, ret_b, len_b = device_update(reward[cut:], done[cut:], n, ret_a, len_a)
    na, nb = int(ca[0]), int(cb[0])
    assert na + nb == n and ca[1] == na and cb[1] == nb
    two = {k: np.concatenate([a[k][:na], b[k][:nb] + (cut if k == "step" else 0)]) for k in a}
    for got in (one, two):
        assert_records(got, want)
    first = np.nonzero((want["env"] == 0) & (want["step"] == cut + 4))[0]
    assert len(first) == 1 and want["length"][first[0]] >= 9
    for r, l in ((ret1, len1), (ret_b, len_b)):
        assert_state(r, l, want_ret, want_len)


# ------------------------------------------------------------------ 3. capacity
def test_capacity_bounds_what_is_written():
    T, B, density = 64, 257, 0.03
    reward, done, want, want_ret, want_len = case(T, B, density)
    finished = len(want["step"])
    cap = finished - 3
    assert cap > 100
    count, rec, guard, ret, length = device_update(reward, done, cap)
    assert count.tolist() == [finished, cap]
    assert_records(rec, want, cap)
    assert (guard == -7).all()
    assert_state(ret, length, want_ret, want_len)
    # NULL arrays with capacity 0 only count
    count, _, _, ret, length = device_update(reward, done, 0, null_records=True)
    assert count.tolist() == [finished, 0]
    assert_state(ret, length, want_ret, want_len)
    # the Python surface: the overflow is reported by flush(), after the first max_episodes
    st = EpisodeStats(default_game_options, B, DEV, handle=handle_env()._h)
    st.update_rollout(torch.as_tensor(reward, device=DEV), torch.as_tensor(done, device=DEV), max_episodes=cap)
    with pytest.raises(RuntimeError, match="%d episodes finished.*holds %d" % (finished, cap)):
        st.flush()
    assert st.episode_lengths == want["length"][:cap].tolist()
    st.flush()  # (nothing left)
    assert len(st.episode_lengths) == cap


# ------------------------------------------------------------------ 4. exact doubles on a real env
def test_rollout_episode_sums_are_sums_of_the_reference_doubles():
    """Default options, 256 envs, 100 steps as two env.rollout launches under EpisodeMonitor,
    the C oracle stepping beside it: every episode's return is the sum, as Python floats from
    the int 0 in step order (gym's stats recorder), of the double rewards the reference's step()
    returns, which reward_table recovers from the float32 ones (-0.9f, -0.8999999761581421, stands
    for 0 + 0.1 + -1, the double nearest -0.9)."""
    from oracle.oracle import OracleBatch

    B, seed = 256, 0x5EED
    mon = EpisodeMonitor(BatchedWolvesAndBushesEnv(num_envs=B, seed=seed, device=DEV))
    orc = OracleBatch(None, B, seed, 0)
    mon.reset()
    orc.reset()
    rng = np.random.RandomState(3)
    rewards, dones = [], []
    for T in (64, 36):
        acts = rng.randint(5, size=(T, B))
        _, _, rew, done = mon.rollout(torch.as_tensor(acts))
        for t in range(T):
            orc.step(acts[t])
            assert np.array_equal(rew[t].cpu().numpy(), orc.reward) and np.array_equal(done[t].cpu().numpy(), orc.done)
        rewards.append(rew.cpu().numpy())
        dones.append(done.cpu().numpy())
    reward32, done = np.concatenate(rewards), np.concatenate(dones)
    assert (reward32 == np.float32(-0.9)).any()
    table = dict(reward_table(default_game_options))
    assert table[float(np.float32(-0.9))] == 0 + 0.1 + -1.0 != float(np.float32(-0.9))
    acc, steps, want = [0] * B, [0] * B, []
    for t in range(reward32.shape[0]):
        for e in range(B):
            acc[e] += table[float(reward32[t, e])]
            steps[e] += 1
            if done[t, e]:
                want.append((float(acc[e]), steps[e], e))
                acc[e], steps[e] = 0, 0
    got = list(zip(mon.get_episode_rewards(), mon.get_episode_lengths(), mon.stats.episode_envs))
    assert len(want) > B and got == want  # float == float: bit for bit
    assert mon.get_total_steps() == 100 * B
    # without the handle the float32 rewards are summed as given: some sum differs
    count, rec, _, _, _ = device_update(reward32, done, len(want), exact=False)
    assert count[0] == len(want) and np.array_equal(rec["length"], [w[1] for w in want])
    assert (rec["return"] != np.array([w[0] for w in want])).any()


# ------------------------------------------------------------------ 5. Monitor wiring
def _lists(mon):
    return mon.get_episode_rewards(), mon.get_episode_lengths(), list(mon.stats.episode_envs)


def test_monitor_over_the_wrapper_mixes_steps_and_rollouts(tmp_path):
    """EpisodeMonitor(PragmaticObsWrapper(env)), the reference's nesting: one env monitored
    through step() only, its twin through step(), rollout() and rollout_policy(), whose sampled
    actions are replayed into the first."""
    B = 192
    mons, envs = [], []
    for k in range(2):
        env = BatchedWolvesAndBushesEnv(dict(pc.OPTS_REF), num_envs=B, seed=pc.SEED, device=DEV)
        envs.append(env)
        mons.append(EpisodeMonitor(PragmaticObsWrapper(env), directory=str(tmp_path / str(k)), video_callable=False,
                                   flush_every=5))
        mons[k].reset()
    stepper, mixed = mons
    pol = policy.DevicePolicy(pc.weights("ref"), envs[1])
    rng = np.random.RandomState(11)

    def steps(n):
        for _ in range(n):
            a = torch.as_tensor(rng.randint(5, size=B), device=DEV)
            stepper.step(a)
            mixed.step(a)

    steps(3)
    acts = torch.as_tensor(rng.randint(5, size=(9, B)), device=DEV)
    out = mixed.rollout(acts)
    assert isinstance(out, tuple) and len(out) == 4 and out[1].shape == (9, B) and out[2].dtype == torch.bool
    for t in range(9):
        stepper.step(acts[t])
    steps(2)
    for T, kw in ((7, {}), (6, {"fused": False, "normalize": True})):
        out = mixed.rollout_policy(pol, T, **kw)
        assert out["actions"].shape == (T, B) and ("normalized" in out) == bool(kw)
        for t in range(T):
            _, r, d, _ = stepper.step(out["actions"][t])
            assert torch.equal(r, out["reward"][t]) and torch.equal(d.view(torch.uint8), out["done"][t])
    steps(4)
    assert len(_lists(stepper)[0]) > B  # (max_turns = 5: every env has finished episodes)
    assert _lists(mixed) == _lists(stepper)
    assert mixed.get_total_steps() == stepper.get_total_steps() == 31 * B
    assert mixed.close() is not None


def test_monitor_over_the_plain_env_and_video(tmp_path):
    B = 100
    mons = [EpisodeMonitor(BatchedWolvesAndBushesEnv(dict(pc.OPTS_REF), num_envs=B, seed=7, device=DEV), flush_every=4)
            for _ in range(2)]
    for m in mons:
        m.reset()
    rng = np.random.RandomState(12)
    acts = torch.as_tensor(rng.randint(5, size=(20, B)), device=DEV)
    for t in range(20):
        mons[0].step(acts[t])
    mons[1].step(acts[0])
    planes, scal, rew, done = mons[1].rollout(acts[1:12])
    assert planes.shape[:2] == (11, B) and done.dtype == torch.uint8
    out = mons[1].rollout_features(acts[12:19])
    assert out["features"].shape[:2] == (7, B)
    mons[1].step(acts[19])
    assert len(_lists(mons[0])[0]) > B and _lists(mons[1]) == _lists(mons[0])
    # video on: rollouts are refused, nothing is stepped
    filmed = EpisodeMonitor(BatchedWolvesAndBushesEnv(dict(pc.OPTS_REF), num_envs=8, seed=7, device=DEV),
                            directory=str(tmp_path))
    with pytest.raises(NotImplementedError, match="video_callable=False"):
        filmed.rollout(acts[:3, :8])
    assert filmed.get_total_steps() == 0


# ------------------------------------------------------------------ 6. normalisation
def restated_normalise(x, done, eps):
    """The contract, sequentially in float64 (Python floats): per column, segments end at each
    done and at the last step; mean = sum / n, var = sum((x - mean)^2) / (n - 1), out =
    float32((x - mean) / (sqrt(var) + eps)); a one-step segment is 0 / 0 = NaN."""
    T, B = x.shape
    out = np.empty((T, B), np.float32)
    xs, ds = x.astype(np.float64).T.tolist(), done.T.tolist()
    for b in range(B):
        col, dn, s = xs[b], ds[b], 0
        while s < T:
            e = s
            while e < T - 1 and not dn[e]:
                e += 1
            n = e - s + 1
            total = 0.0
            for t in range(s, e + 1):
                total += col[t]
            mean = total / n
            ss = 0.0
            for t in range(s, e + 1):
                dev = col[t] - mean
                ss += dev * dev
            denom = math.sqrt(ss / (n - 1)) + eps if n > 1 else math.nan
            for t in range(s, e + 1):
                out[t, b] = np.float32((col[t] - mean) / denom)
            s = e + 1
    return out


def ulp_distance(a, b):
    """float32 steps between a and b (NaN positions must be equal and count 0)"""
    assert np.array_equal(np.isnan(a), np.isnan(b))
    ia, ib = (np.where(np.isnan(v), np.float32(0), v).view(np.int32).astype(np.int64) for v in (a, b))
    ia, ib = (np.where(i < 0, np.int64(-2 ** 31) - i, i) for i in (ia, ib))
    return np.abs(ia - ib)


EPS = 1.1920928955078125e-07


@pytest.mark.parametrize("density", DENSITIES)
@pytest.mark.parametrize("T,B", SHAPES)
def test_normalisation_equals_the_sequential_float64_restatement(T, B, density):
    """Bit for bit, NaN positions equal.  The contract allows one float32 ulp (the float64
    quotient could differ from the host's by a few float64 ulps in divide and sqrt, which the
    rounding to float32 turns into at most one float32 step); on the MI355X the device's float64
    divide and sqrt round as the host's do and every case is equal, so equality is what is asserted
    (the distance is printed first)."""
    reward, done = make_segment(T, B, density)
    x = discounted_returns(torch.as_tensor(reward, device=DEV), torch.as_tensor(done, device=DEV), 0.99)
    got = normalized_returns(x, torch.as_tensor(done, device=DEV)).cpu().numpy()
    want = restated_normalise(x.cpu().numpy(), done, EPS)
    dist = ulp_distance(got, want)
    print("normalisation %dx%d density %g: max %d ulp, %d of %d differ, %d NaN"
          % (T, B, density, dist.max(), (dist > 0).sum(), dist.size, np.isnan(want).sum()))
    assert dist.max() == 0
    if density >= 1.0 or T == 1:
        assert np.isnan(got).all()          # one-step segments only
    elif density == 0.0:
        assert not np.isnan(got).any()      # one open segment per column
    # in place, and another eps
    done_d = torch.as_tensor(done, device=DEV)
    y = x.clone()
    assert normalized_returns(y, done_d, out=y) is y
    assert np.array_equal(y.cpu().numpy().view(np.uint32), got.view(np.uint32))
    other = normalized_returns(x, done_d.to(torch.uint8), eps=0.5).cpu().numpy()
    assert ulp_distance(other, restated_normalise(x.cpu().numpy(), done, 0.5)).max() == 0


@pytest.mark.parametrize("T,density", [(128, 0.02), (128, 0.5), (97, 0.02)])
def test_normalisation_at_the_longest_segment_kept_in_lds(T, density):
    """T = 128 is the last length of the LDS kernel (129, above, the first of the other one); with
    T > 64 the dones of a column fill both words of its mask, and at 97 the last load chunk and the
    second word are partial."""
    B = 70
    reward, done = make_segment(T, B, density, seed=3)
    done[:, 5] = False
    done[70, 5] = True            # a segment that ends in the second word, and an open one after it
    x = discounted_returns(torch.as_tensor(reward, device=DEV), torch.as_tensor(done, device=DEV), 0.99)
    got = normalized_returns(x, torch.as_tensor(done, device=DEV)).cpu().numpy()
    assert ulp_distance(got, restated_normalise(x.cpu().numpy(), done, EPS)).max() == 0
    assert not np.isnan(got[:, 5]).any()


def test_normalisation_matches_reference_finish_episode():
    """tests/golden/returns.npz: the reference's own normalised float32 values, the episodes laid
    out in 61 columns as in test_discounted_returns_exact_match_reference_finish_episode, whole
    episodes only, at the project's tolerance for them (rtol 1e-5, atol 1e-5)."""
    z = np.load(gr.GOLDEN_DIR + "/returns.npz")
    n, cols = len(z["done"]), 61
    starts = np.concatenate([[0], np.nonzero(z["done"])[0][:-1] + 1])
    idx = (starts[(29 * np.arange(cols)) % len(starts)][None, :] + np.arange(n)[:, None]) % n
    done = torch.as_tensor(z["done"][idx]).to(DEV)
    returns = torch.as_tensor(z["returns64"].astype(np.float32)[idx]).to(DEV)
    norm = normalized_returns(returns, done).cpu().numpy()
    for c in range(cols):
        last_done = np.nonzero(z["done"][idx[:, c]])[0][-1]
        np.testing.assert_allclose(norm[:last_done + 1, c], z["normalised32"][idx[:last_done + 1, c]],
                                   rtol=1e-5, atol=1e-5, equal_nan=True)


@pytest.mark.parametrize("fused", [None, False])
def test_rollout_policy_normalize_is_normalized_returns_of_its_own_returns(fused):
    env = BatchedWolvesAndBushesEnv(dict(pc.OPTS_REF), num_envs=68, seed=pc.SEED, device=DEV)
    w = PragmaticObsWrapper(env)
    w.reset()
    pol = policy.DevicePolicy(pc.weights("ref"), env)
    out = w.rollout_policy(pol, 12, fused=fused, normalize=True)
    assert out["done"].any() and out["normalized"].shape == (12, 68)
    want = normalized_returns(out["returns"], out["done"])
    assert torch.equal(out["normalized"].view(torch.int32), want.view(torch.int32))
    assert "normalized" not in w.rollout_policy(pol, 3, fused=fused)
    assert w.rollout_policy(pol, 0, normalize=True)["normalized"].shape == (0, 68)
