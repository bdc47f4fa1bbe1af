"""Every instance of wab_returns_kernel<VEC, NE> against the C oracle's scan in double
(oracle.discounted_returns, with exact_values where a reward table is in play), bit for bit
(np.array_equal), on the segments of tests/returns_cases.py.  Each case first asserts the
instance the launch takes, through wab_debug_returns_plan (the host function the launch itself
calls), so a moved threshold fails here instead of silently dropping an instance.

Which case launches which instance (VEC, NE):
  test_vec_dispatch          (4, 3) (2, 3) (1, 3): B = 262144 aligned; reward / done 8 / 2 bytes
                             off, B = 262146, B = 131072; returns 4 bytes or done 1 byte off,
                             B = 262145, B = 131068 -- with the default options' table
  test_reward_table_sizes    (1, n) at B = 1000, (2, n) at B = 131072, (4, n) at B = 262144 for
                             n = 0, 1, 2, 3, 4, 8 (8 twice: six inexact entries padded, and eight)
  test_chunk_edges           (1, 0) the plain call and (1, 3) the defaults, T = 1 .. 65
  test_gamma_zero_and_one    (1, 0) and (1, 3)
test_case_lists_cover_every_instance asserts that these lists name all 18.

The scan inside the rollout launch (T <= 128, wab_step_small's tail) runs on the same option sets
in test_in_launch_scan_*; T = 129 is the first length handed to wab_returns_kernel."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import returns_cases as rc
from oracle import oracle as orc
from test_featurizer_oracle import step_reward_values
from wab_gym_amd import _lib
from wab_gym_amd.env import BatchedWolvesAndBushesEnv
from wab_gym_amd.wrappers import discounted_returns

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GAMMA = 0.99


@functools.lru_cache(maxsize=None)
def table_env(name):
    """A 64-env handle of the option set: it only supplies the reward table (the call takes its own B)."""
    return BatchedWolvesAndBushesEnv(rc.options_of(name), num_envs=64, seed=1, device=DEV)


def plan_of(env, reward, done, out):
    got = (ctypes.c_int32 * 2)(-1, -1)
    _lib.check(_lib.load().wab_debug_returns_plan(None if env is None else env._h, reward.data_ptr(), done.data_ptr(),
                                                  out.data_ptr(), reward.shape[1], got), "wab_debug_returns_plan")
    return got[0], got[1]


@functools.lru_cache(maxsize=2)
def case(T, B, name, bootstrap, table=True):
    """(reward, done, bootstrap, the oracle's returns) on the host, shared by the cases that
    differ only in where the device copies lie."""
    values = step_reward_values(rc.options_of(name))
    reward, done, boot = rc.make_case(T, B, values, bootstrap=bootstrap)
    want = orc.discounted_returns(reward, done, GAMMA, boot, exact_values=values if table else None)
    return reward, done, boot, want


def device_view(host, offset):
    """`host` on the device, `offset` elements into a larger (256-byte aligned) buffer."""
    buf = torch.empty(host.size + 8, dtype=torch.from_numpy(host[:0]).dtype, device=DEV)
    assert buf.data_ptr() % 16 == 0
    view = buf[offset:offset + host.size].view(host.shape)
    view.copy_(torch.from_numpy(host))
    return view


def run(env, host_case, want_plan, offsets=(0, 0, 0), gamma=GAMMA):
    reward, done, boot, want = host_case
    r, d = device_view(reward, offsets[0]), device_view(done, offsets[1])
    out = device_view(np.zeros(reward.shape, np.float32), offsets[2])
    assert plan_of(env, r, d, out) == want_plan
    got = discounted_returns(r, d, gamma, None if boot is None else torch.as_tensor(boot, device=DEV), out=out, env=env)
    assert got is out
    got = got.cpu().numpy()
    bad = np.argwhere(got != want)
    assert np.array_equal(got, want), "%d differ, first at (t, b) = %s" % (len(bad), bad[:1].tolist())


# (B, (reward, done, returns) offsets in elements, planned VEC)
DISPATCH = [
    (262144, (0, 0, 0), 4),
    (262144, (2, 0, 0), 2),   # reward 8 bytes in
    (262144, (0, 0, 1), 1),   # returns 4 bytes in
    (262144, (0, 2, 0), 2),   # done 2 bytes in
    (262144, (0, 1, 0), 1),   # done 1 byte in
    (262146, (0, 0, 0), 2),   # B % 4 != 0
    (262145, (0, 0, 0), 1),   # B odd
    (131072, (0, 0, 0), 2),   # the smallest batch of VEC 2: B / 4 < 65536
    (131068, (0, 0, 0), 1),   # B / 2 < 65536
]
NE_BATCHES = ((1000, 1), (131072, 2), (262144, 4))
EDGE_T = (1, 31, 32, 33, 64, 65)
EDGE_B = (1, 63, 64, 65, 1000)


def test_case_lists_cover_every_instance():
    planned = {(vec, 3) for _, _, vec in DISPATCH}
    planned |= {(vec, ne) for _, _, ne in rc.OPTION_SETS for _, vec in NE_BATCHES}
    planned |= {(1, 0), (1, 3)}
    assert planned == {(vec, ne) for vec in (1, 2, 4) for ne in (0, 1, 2, 3, 4, 8)}


@pytest.mark.parametrize("T,B,offsets,vec", [(T, B, o, v) for T in (33, 65) for B, o, v in DISPATCH])
def test_vec_dispatch(T, B, offsets, vec):
    """The float2 / float4 rows, the 16- and 32-bit done loads and their byte select, at the
    smallest batches that reach them; T = 33 and 65: two and three chunks with a one-step last
    chunk (T = 33 with a bootstrap, T = 65 without)."""
    run(table_env("defaults"), case(T, B, "defaults", T == 33), (vec, 3), offsets)


@pytest.mark.parametrize("B,vec", NE_BATCHES)
@pytest.mark.parametrize("name,ne", [(n, ne) for n, _, ne in rc.OPTION_SETS])
def test_reward_table_sizes(name, ne, B, vec):
    run(table_env(name), case(33, B, name, True), (vec, ne))


@pytest.mark.parametrize("T", EDGE_T)
def test_chunk_edges(T):
    """The 32-step chunks' edges at VEC 1: one chunk short, exact and one step over, two chunks
    exact and one step over (where a chunk is short its loads past the segment's start re-read
    step 0, unused); one thread, a wave short, exact and one over, several workgroups; the plain
    call and the default table, with a bootstrap and without."""
    for B in EDGE_B:
        for bootstrap in (True, False):
            run(None, case(T, B, "defaults", bootstrap, False), (1, 0))
            run(table_env("defaults"), case(T, B, "defaults", bootstrap), (1, 3))


@pytest.mark.parametrize("gamma", [0.0, 1.0])
def test_gamma_zero_and_one(gamma):
    values = step_reward_values()
    reward, done, boot = rc.make_case(65, 1000, values, seed=1)
    run(None, (reward, done, boot, orc.discounted_returns(reward, done, gamma, boot)), (1, 0), gamma=gamma)
    want = orc.discounted_returns(reward, done, gamma, boot, exact_values=values)
    run(table_env("defaults"), (reward, done, boot, want), (1, 3), gamma=gamma)


# ------------------------------------------------------------------ the scan inside the rollout launch
def in_launch_case(name, T, B=68):
    """rollout_features' returns of T steps against the oracle's scan of the reward and done
    the same launch returned (max_turns = 5: episodes end inside the segment)."""
    opts = dict(rc.options_of(name), max_turns=5)
    env = BatchedWolvesAndBushesEnv(opts, num_envs=B, seed=7, device=DEV, validate_actions=False)
    env.reset()
    rng = np.random.RandomState(T)
    boot = rng.standard_normal(B).astype(np.float32)
    r = env.rollout_features(torch.as_tensor(rng.randint(env.n_actions, size=(T, B))), gamma=GAMMA, bootstrap=boot)
    assert env.counters()["rollout_launches"] == 1  # the steps ran as one launch
    reward, done = r["reward"].cpu().numpy(), r["done"].cpu().numpy()
    assert done.sum() > 0
    values = step_reward_values(opts)
    assert set(np.unique(reward).tolist()) <= set(np.asarray(values, np.float64).astype(np.float32).tolist())
    want = orc.discounted_returns(reward, done, GAMMA, boot, exact_values=values)
    assert np.array_equal(r["returns"].cpu().numpy(), want)
    return reward


@pytest.mark.parametrize("name", [n for n, _, _ in rc.OPTION_SETS])
def test_in_launch_scan_at_every_option_set(name):
    in_launch_case(name, 7)


@pytest.mark.parametrize("T", [128, 129])
def test_in_launch_scan_last_length_and_first_of_the_kernel(T):
    """T = 128 = kMaxFusedReturnSteps is the last length scanned in the launch, T = 129 the first
    handed to wab_returns_kernel after it."""
    reward = in_launch_case("defaults", T)
    assert len(np.unique(reward)) > 2
