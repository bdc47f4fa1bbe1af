"""Episode statistics of whole rollout segments, the parts that need no GPU: EpisodeStats.
update_rollout's CPU path against the per-step update() loop, EpisodeMonitor's rollout methods
over a scripted stand-in env, argument checks, the C-ABI declarations and their ctypes mirror,
and normalized_returns on CPU tensors."""
import os
import re

import numpy as np
import pytest
import torch

from wab_gym_amd import _lib
from wab_gym_amd.monitor import EpisodeMonitor, EpisodeStats
from wab_gym_amd.options import default_game_options
from wab_gym_amd.wrappers import normalize_episode_returns, normalized_returns

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "wab.h")

REWARDS = np.array([0.0, 0.1, 1.0, 1.1, -0.9, -1.0, 0.25], dtype=np.float32)
NEW_FUNCTIONS = ("wab_episode_stats_workspace", "wab_episode_stats_update", "wab_normalize_episode_returns")


def segment(T, B, density, seed):
    rng = np.random.RandomState(seed)
    return (torch.as_tensor(REWARDS[rng.randint(len(REWARDS), size=(T, B))]),
            torch.as_tensor(rng.random_sample((T, B)) < density))


def lists(st):
    st.flush()
    return st.episode_rewards, st.episode_lengths, st.episode_envs


def test_update_rollout_on_cpu_equals_the_update_loop():
    T, B = 37, 23
    reward, done = segment(T, B, 0.15, 1)
    a = EpisodeStats(default_game_options, B, "cpu", flush_every=5)
    b = EpisodeStats(default_game_options, B, "cpu", flush_every=5)
    for t in range(T):
        a.update(reward[t], done[t])
    b.update(reward[0], done[0])                    # per-step entries stay ahead of the rollout's
    b.update_rollout(reward[1:20], done[1:20])
    b.update_rollout(reward[20:20], done[20:20])    # T = 0
    b.update_rollout(reward[20:], done[20:].to(torch.uint8))
    assert len(lists(a)[0]) > 20
    assert lists(a) == lists(b)
    assert a.total_steps == b.total_steps == T * B
    assert torch.equal(a.ret, b.ret) and torch.equal(a.length, b.length)
    assert len(b.timestamps) == len(b.episode_rewards) == len(b.episode_types)


def test_update_rollout_rejects_wrong_shapes_and_dtypes():
    B = 6
    st = EpisodeStats(default_game_options, B, "cpu")
    reward, done = segment(4, B, 0.5, 2)
    for r, d in ((reward[0], done[0]),                        # one step: [B], not [T, B]
                 (reward[:, :5], done[:, :5]),                # another batch
                 (reward, done[:3]),                          # done of another shape
                 (reward.to(torch.int32), done),              # integer rewards
                 (reward, done.to(torch.float32)),            # float dones
                 (reward, done.to(torch.int64))):
        with pytest.raises(ValueError):
            st.update_rollout(r, d)
    with pytest.raises(ValueError):
        st.update_rollout(reward, done, max_episodes=-1)
    assert lists(st) == ([], [], []) and st.total_steps == 0


class ScriptedEnv:
    """a CPU stand-in that plays back rewards and dones, per step() and through the three
    multi-step methods in the forms the env and the wrapper return"""

    def __init__(self, reward, done, wrapper_form=False):
        self.reward_seq, self.done_seq, self.t = reward, done, 0
        self.game_options = dict(default_game_options)
        self.num_envs = reward.shape[1]
        self.device = torch.device("cpu")
        self.wrapper_form = wrapper_form

    def reset(self, mask=None):
        return None

    def _take(self, T):
        t, self.t = self.t, self.t + T
        return self.reward_seq[t:t + T], self.done_seq[t:t + T]

    def step(self, actions):
        r, d = self._take(1)
        return None, r[0], d[0], {}

    def rollout(self, actions):
        r, d = self._take(len(actions))
        if self.wrapper_form:   # (features, reward, done, returns)
            return torch.zeros(len(actions), self.num_envs, 3), r, d, torch.zeros_like(r)
        return (torch.zeros(len(actions), self.num_envs, 3, dtype=torch.uint8),
                torch.zeros(len(actions), 3, self.num_envs, dtype=torch.uint8), r, d.to(torch.uint8))

    def rollout_features(self, actions, gamma=0.99):
        r, d = self._take(len(actions))
        return {"features": None, "reward": r, "done": d.to(torch.uint8), "returns": None}

    def rollout_policy(self, policy, T, normalize=False):
        r, d = self._take(T)
        return {"actions": None, "reward": r, "done": d.to(torch.uint8)}

    def close(self):
        pass


@pytest.mark.parametrize("wrapper_form", [False, True])
def test_monitor_accounts_every_multi_step_method(wrapper_form, tmp_path):
    T, B = 60, 9
    reward, done = segment(T, B, 0.1, 3)
    per_step = EpisodeMonitor(ScriptedEnv(reward, done), flush_every=7)
    per_step.reset()
    for t in range(T):
        per_step.step(None)
    mixed = EpisodeMonitor(ScriptedEnv(reward, done, wrapper_form), directory=str(tmp_path), video_callable=False,
                           flush_every=7)
    mixed.reset()
    for _ in range(3):
        mixed.step(None)
    out = mixed.rollout(torch.zeros(17, B))
    assert isinstance(out, tuple) and len(out) == 4
    mixed.step(None)
    out = mixed.rollout_features(torch.zeros(11, B), gamma=0.9)
    assert set(out) == {"features", "reward", "done", "returns"}
    for _ in range(8):
        mixed.step(None)
    out = mixed.rollout_policy(None, 20)
    assert set(out) == {"actions", "reward", "done"}
    assert len(per_step.get_episode_rewards()) > 20
    assert mixed.get_episode_rewards() == per_step.get_episode_rewards()
    assert mixed.get_episode_lengths() == per_step.get_episode_lengths()
    assert mixed.stats.episode_envs == per_step.stats.episode_envs
    assert mixed.get_total_steps() == per_step.get_total_steps() == T * B
    path = mixed.close()
    assert path is not None and len(mixed.stats.timestamps) == len(mixed.stats.episode_rewards)


def test_monitor_rollouts_raise_while_video_is_on(tmp_path):
    reward, done = segment(8, 4, 0.3, 4)
    env = ScriptedEnv(reward, done)
    env.render = lambda **kw: np.zeros((1, 2, 2, 3), np.uint8)
    mon = EpisodeMonitor(env, directory=str(tmp_path))
    for call in (lambda: mon.rollout(torch.zeros(2, 4)), lambda: mon.rollout_features(torch.zeros(2, 4)),
                 lambda: mon.rollout_policy(None, 2)):
        with pytest.raises(NotImplementedError, match="video_callable=False"):
            call()
    assert env.t == 0  # nothing was stepped


def test_header_and_mirror_declare_the_episode_functions():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in NEW_FUNCTIONS:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _lib.EXPORTED
    m = re.search(r"int64_t\s+wab_episode_stats_workspace\s*\(\s*int32_t\s+T\s*,\s*int64_t\s+B\s*\)", text)
    assert m, "wab_episode_stats_workspace(int32_t T, int64_t B) returns bytes as int64_t"
    version = int(re.search(r"#define\s+WAB_ABI_VERSION\s+(\d+)", open(HEADER).read()).group(1))
    assert version == _lib.ABI_VERSION and version >= 10


def test_normalized_returns_on_cpu_is_normalize_episode_returns():
    rng = np.random.RandomState(5)
    x = torch.as_tensor(rng.standard_normal((40, 13)).astype(np.float32))
    done = torch.as_tensor(rng.random_sample((40, 13)) < 0.1)
    want = normalize_episode_returns(x, done)
    got = normalized_returns(x, done)
    assert got.dtype == torch.float32 and torch.equal(torch.isnan(got), torch.isnan(want))
    assert torch.equal(torch.nan_to_num(got), torch.nan_to_num(want))
    out = torch.empty_like(x)
    assert normalized_returns(x, done, out=out) is out and torch.equal(torch.nan_to_num(out), torch.nan_to_num(want))
    assert torch.equal(torch.nan_to_num(normalized_returns(x, done, eps=1e-3)),
                       torch.nan_to_num(normalize_episode_returns(x, done, eps=1e-3)))
    with pytest.raises(ValueError):
        normalized_returns(x, done[:5])
    with pytest.raises(ValueError):
        normalized_returns(x, done, out=torch.empty(40, 13, dtype=torch.float64))
