"""Monitor-style episode statistics for a batched env.

The reference wraps its env in gym 0.17's `gym.wrappers.Monitor` (actor_critic.py:46,
wab_env.py:1013), whose stats recorder sums each episode's rewards as Python floats in step
order (starting from the int 0) and counts its steps, and on close writes
`openaigym.episode_batch.<infix>.stats.json` with `initial_reset_timestamp`, `timestamps`,
`episode_lengths`, `episode_rewards` and `episode_types`.  gym is not installed here, so the
file layout is a restatement of gym 0.17's stats recorder (parity unpinned); the episode sums
themselves are pinned bit for bit against sums of the reference's own double rewards in the
golden vectors (tests/test_monitor.py).

Videos follow gym 0.17's Monitor for one env of the batch (`video_env`, default 0): episode
k of that env is recorded when `video_callable(k)` (default: gym's capped cubic schedule, k
in 0, 1, 8, 27, ... 729, then every 1000th), one frame after its reset and one after every
step, the terminal observation included (when the env was made with return_terminal=True;
the autoreset env's obs on a done step is already the next episode's).  Frames come from
`env.render(envs=(video_env, 1))` on device.  There is no ffmpeg or imageio in this image, so
a video is an animated GIF (PIL) at the env's `video.frames_per_second` instead of gym's
mp4, with gym's `<base>.meta.json` beside it.  The monitor reads that env's done flag on the
host (one synchronisation per step) only while the env's current or a soon-starting episode
is scheduled; otherwise episodes are counted on device and read at the stats flushes.

The device reward is the reference's double reward rounded to float32 (include/wab.h).  Each
step's double is recovered exactly from the few values a step can produce, `r_x` or
`r_eat + r_x` for r_x in (per turn, finishing, starving, killed) (wab_env.py:299-340), then
summed in float64 on device.  Finished episodes are gathered every `flush_every` steps (one
host synchronisation), so the per-step path stays asynchronous.

The multi-step launches (`rollout`, `rollout_features`, `rollout_policy`) are accounted a whole
[T, B] segment at a time: `EpisodeStats.update_rollout` is one call of wab_episode_stats_update
(include/wab.h), the same adds in the same order as T `update` calls, its finished episodes
compacted on device in (step, env) order and gathered at the next flush.  The episodes of one such
call share one timestamp (the call's), and rollouts record no video.
"""
from __future__ import annotations

import ctypes
import json
import os
import time

import numpy as np

_REWARD_KEYS = ("reward_per_turn", "reward_for_finishing", "reward_for_starving", "reward_for_being_killed")


def reward_table(game_options):
    """[(float32 value, exact double)] of every reward a step can return (wab_env.py:299-340):
    `0 + r_x` without an eat, `0 + r_eat + r_x` with one."""
    r_eat = game_options["reward_for_eating"]
    pairs = {}
    for k in _REWARD_KEYS:
        rx = game_options[k]
        for d in (0 + rx, 0 + r_eat + rx):
            d = float(d)
            f = float(np.float32(d))
            if f in pairs and pairs[f] != d:
                raise ValueError("rewards %r and %r round to the same float32: the double sum is "
                                 "not recoverable from the device reward" % (pairs[f], d))
            pairs[f] = d
    return sorted(pairs.items())


class EpisodeStats:
    """Per-env episode return (float64) and length on device; finished episodes are gathered
    into host lists in (step, env) order by flush()."""

    MAX_QUEUED = 4  # rollout segments held on device before update_rollout flushes on its own

    def __init__(self, game_options, num_envs, device, flush_every=32, handle=None):
        import torch

        self._torch = torch
        self.num_envs = int(num_envs)
        self.device = torch.device(device)
        self.flush_every = int(flush_every)
        self._game_options = game_options
        self._handle = handle  # the env's wab_handle (its exact reward table), for update_rollout
        self._own_handle = None
        self._queue = []  # pending segments in finishing order: ("steps", ...) or ("rollout", ...)
        tab = reward_table(game_options)
        self._f32 = torch.tensor([f for f, _ in tab], dtype=torch.float32, device=self.device)
        self._f64 = torch.tensor([d for _, d in tab], dtype=torch.float64, device=self.device)
        B, K = self.num_envs, self.flush_every
        self.ret = torch.zeros(B, dtype=torch.float64, device=self.device)
        self.length = torch.zeros(B, dtype=torch.int64, device=self.device)
        self._buf_ret = torch.zeros((K, B), dtype=torch.float64, device=self.device)
        self._buf_len = torch.zeros((K, B), dtype=torch.int64, device=self.device)
        self._times = []
        self.episode_rewards, self.episode_lengths, self.episode_envs = [], [], []
        self.timestamps, self.episode_types = [], []
        self.total_steps = 0

    def restart(self, mask=None):
        """Start new episodes (all envs, or those with mask[i]); unfinished ones are dropped."""
        if mask is None:
            self.ret.zero_()
            self.length.zero_()
        else:
            m = self._torch.as_tensor(mask, device=self.device).bool()
            self.ret.masked_fill_(m, 0.0)
            self.length.masked_fill_(m, 0)

    def decode(self, reward):
        """float32 device rewards -> the reference's doubles."""
        r = reward.to(self._torch.float32)
        hit = r.unsqueeze(1) == self._f32.unsqueeze(0)  # [B, n_values]
        exact = (hit.to(self._torch.float64) * self._f64.unsqueeze(0)).sum(1)
        return self._torch.where(hit.any(1), exact, r.to(self._torch.float64))

    def update(self, reward, done):
        """One step of every env: add the step's reward, count it, close the done episodes."""
        t = self._torch
        d = t.as_tensor(done, device=self.device).bool()
        self.ret += self.decode(t.as_tensor(reward, device=self.device))
        self.length += 1
        k = len(self._times)
        self._buf_ret[k].copy_(self.ret)
        self._buf_len[k].copy_(t.where(d, self.length, t.zeros_like(self.length)))
        self._times.append(time.time())
        self.ret.masked_fill_(d, 0.0)
        self.length.masked_fill_(d, 0)
        self.total_steps += self.num_envs
        if len(self._times) == self.flush_every:
            self.flush()

    def _rollout_handle(self):
        """The wab_handle whose reward table update_rollout uses: the env's, or one of this
        object's own (one env, made from the game options) when it was built without."""
        if self._handle is not None:
            return self._handle
        if self._own_handle is None:
            from . import _lib
            from .options import make_config

            cfg, self._own_keep = make_config(self._game_options)
            dev = self.device.index if self.device.index is not None else self._torch.cuda.current_device()
            h = ctypes.c_void_p()
            _lib.check(_lib.load().wab_create(ctypes.addressof(cfg), 1, 0, 0, dev, ctypes.byref(h)), "wab_create")
            self._own_handle = h
        return self._own_handle

    def __del__(self):
        h, self._own_handle = getattr(self, "_own_handle", None), None
        if h is not None:
            try:
                from . import _lib

                _lib.load().wab_destroy(h)
            except Exception:
                pass

    def _queue_steps(self):
        """Move the per-step entries not yet gathered into the queue (device copies, no
        synchronisation), so that what is recorded after them is gathered after them."""
        k = len(self._times)
        if k:
            self._queue.append(("steps", self._buf_ret[:k].clone(), self._buf_len[:k].clone(), self._times))
            self._times = []

    def update_rollout(self, reward, done, max_episodes=None):
        """T steps of every env at once: `reward` and `done` [T, B] of a multi-step launch, the same
        statistics as T update() calls (the same double adds in the same order).  On a HIP device it
        is one wab_episode_stats_update call on the current stream, without host synchronisation: the
        finished episodes stay on device, compacted in (step, env) order, until flush(); after
        MAX_QUEUED such segments the next call flushes first.  max_episodes bounds the episodes one
        call can record (device buffers of that many records, 20 bytes each); None means T * B, which
        cannot overflow; when more finish than a smaller bound holds, flush() raises RuntimeError
        naming both numbers, after recording the first max_episodes.  All episodes of one call get
        the call's timestamp.  CPU tensors take the update() loop."""
        t = self._torch
        reward, done = t.as_tensor(reward), t.as_tensor(done)
        if reward.dim() != 2 or reward.shape[1] != self.num_envs:
            raise ValueError("reward must have shape [T, %d], not %s" % (self.num_envs, tuple(reward.shape)))
        if tuple(done.shape) != tuple(reward.shape):
            raise ValueError("done must have the shape of reward %s, not %s" % (tuple(reward.shape), tuple(done.shape)))
        if not reward.dtype.is_floating_point:
            raise ValueError("reward must be a floating-point tensor, not %s" % reward.dtype)
        if done.dtype not in (t.bool, t.uint8):
            raise ValueError("done must be a bool or uint8 tensor, not %s" % done.dtype)
        if reward.device != done.device:
            raise ValueError("reward is on %s, done on %s" % (reward.device, done.device))
        T, B = reward.shape
        if max_episodes is not None and int(max_episodes) < 0:
            raise ValueError("max_episodes must be >= 0")
        if reward.device.type != "cuda" or self.device.type != "cuda":
            for k in range(T):
                self.update(reward[k], done[k])
            return
        if reward.device != self.device and self.device.index is not None:
            raise ValueError("reward is on %s, the statistics on %s" % (reward.device, self.device))
        from . import _lib

        L = _lib.load()
        if len(self._queue) >= self.MAX_QUEUED:
            self.flush()
        self._queue_steps()
        dev = reward.device
        r = reward.to(t.float32).contiguous()
        d = (done.view(t.uint8) if done.dtype == t.bool else done).contiguous()
        cap = T * B if max_episodes is None else min(int(max_episodes), T * B)
        ws_bytes = int(L.wab_episode_stats_workspace(T, B))
        if ws_bytes < 0:
            _lib.check(ws_bytes, "wab_episode_stats_workspace")
        ws = t.empty(ws_bytes // 8 + 1, dtype=t.int64, device=dev)
        ep_ret = t.empty(cap, dtype=t.float64, device=dev)
        ep_i32 = t.empty((3, cap), dtype=t.int32, device=dev)  # length, env, step
        count = t.empty(2, dtype=t.int64, device=dev)
        ptr = (lambda x: x.data_ptr()) if cap > 0 else (lambda x: None)
        stream = ctypes.c_void_p(t.cuda.current_stream(dev).cuda_stream)
        _lib.check(L.wab_episode_stats_update(self._rollout_handle(), r.data_ptr(), d.data_ptr(), T, B,
                                              self.ret.data_ptr(), self.length.data_ptr(), ptr(ep_ret),
                                              ptr(ep_i32[0]), ptr(ep_i32[1]), ptr(ep_i32[2]), cap, count.data_ptr(),
                                              ws.data_ptr(), stream), "wab_episode_stats_update")
        self._queue.append(("rollout", ep_ret, ep_i32, count, cap, time.time()))
        self.total_steps += T * B

    def _record(self, rets, lens, envs, times):
        self.episode_rewards.extend(float(x) for x in rets)
        self.episode_lengths.extend(int(x) for x in lens)
        self.episode_envs.extend(int(x) for x in envs)
        self.timestamps.extend(times)
        self.episode_types.extend("t" for _ in envs)

    def _record_steps(self, buf_ret, buf_len, times):
        lens = buf_len.cpu().numpy()
        rets = buf_ret.cpu().numpy()
        steps, envs = np.nonzero(lens)
        self._record(rets[steps, envs], lens[steps, envs], envs, [times[s] for s in steps])

    def flush(self):
        """Gather the episodes finished since the last flush, in finishing order (synchronises)."""
        while self._queue:
            item = self._queue.pop(0)
            if item[0] == "steps":
                self._record_steps(*item[1:])
                continue
            _, ep_ret, ep_i32, count, cap, stamp = item
            finished, written = (int(x) for x in count.cpu())
            i32 = ep_i32[:, :written].cpu().numpy()
            self._record(ep_ret[:written].cpu().numpy(), i32[0], i32[1], [stamp] * written)
            if finished > cap:
                raise RuntimeError("update_rollout: %d episodes finished in one call, max_episodes holds %d; "
                                   "the first %d were recorded, the rest are lost" % (finished, cap, cap))
        k = len(self._times)
        if k:
            self._record_steps(self._buf_ret[:k], self._buf_len[:k], self._times)
            self._times = []


def capped_cubic_video_schedule(episode_id):
    """gym 0.17 monitor.capped_cubic_video_schedule: episodes 0, 1, 8, 27, ..., 729, then
    every 1000th."""
    if episode_id < 1000:
        return int(round(episode_id ** (1.0 / 3))) ** 3 == episode_id
    return episode_id % 1000 == 0


class GifRecorder:
    """gym's VideoRecorder for rgb_array frames, as an animated GIF (no ffmpeg here):
    `<base>.gif` and `<base>.meta.json`; an episode closed with no frames writes only the
    metadata, marked empty."""

    def __init__(self, base_path, metadata, fps, enabled=True):
        self.path = base_path + ".gif"
        self.metadata_path = base_path + ".meta.json"
        self.metadata = dict(metadata)
        self.fps = fps
        self.enabled = enabled
        self.frames = []

    def capture_frame(self, frame):
        if self.enabled:
            self.frames.append(np.asarray(frame, dtype=np.uint8))

    @property
    def functional(self):
        return self.enabled and bool(self.frames)

    def close(self):
        if not self.enabled:
            return
        if self.frames:
            from PIL import Image

            ims = [Image.fromarray(f) for f in self.frames]
            ims[0].save(self.path, save_all=True, append_images=ims[1:], duration=int(round(1000.0 / self.fps)),
                        loop=0)
            import PIL

            self.metadata.update(content_type="image/gif", encoder_version={"backend": "PIL", "version": PIL.__version__},
                                 frames=len(self.frames))
        else:
            self.metadata["empty"] = True
        with open(self.metadata_path, "w") as f:
            json.dump(self.metadata, f)


class EpisodeMonitor:
    """`gym.wrappers.Monitor(env, directory, video_callable, force)` for a batched env: episode
    statistics of every env, video of env `video_env`'s scheduled episodes (module
    docstring).  video_callable=False records none.  rollout(), rollout_features() and
    rollout_policy() call the wrapped object's method and account its [T, B] reward and done in
    one device call (EpisodeStats.update_rollout); they record no video and raise
    NotImplementedError while video is enabled.  Other attributes of the wrapped env pass
    through, except snapshot() and restore(): the running episode sums and the video recorder
    are not part of an EnvSnapshot, so after a restore the statistics would describe episodes
    that were never played; both raise NotImplementedError here."""

    def __init__(self, env, directory=None, force=False, flush_every=32, monitor_id=0, video_callable=None,
                 video_env=0, video_scale=32):
        self.env = env
        self.stats = EpisodeStats(env.game_options, env.num_envs, env.device, flush_every,
                                  handle=getattr(env, "_h", None))
        self.directory = directory
        self.initial_reset_timestamp = None
        self._infix = "%d.%d" % (monitor_id, os.getpid())
        self.video_callable = capped_cubic_video_schedule if video_callable is None else video_callable
        self.video_env = int(video_env)
        self.video_scale = int(video_scale)
        self._video_on = (directory is not None and self.video_callable is not False
                          and hasattr(env, "render") and 0 <= self.video_env < env.num_envs)
        self.episode_id = 0  # episodes of video_env started (gym's Monitor.episode_id)
        self.videos = []
        self._rec = None
        self._ep_dev = None  # video_env's episode ends since the last count (device, unarmed)
        self._unsynced = 0
        if directory is not None:
            os.makedirs(directory, exist_ok=True)
            if force:
                for f in os.listdir(directory):
                    if f.startswith("openaigym."):
                        os.remove(os.path.join(directory, f))

    def __getattr__(self, name):
        return getattr(self.env, name)

    def snapshot(self, envs=None):
        raise NotImplementedError("EpisodeMonitor does not snapshot: its episode statistics are not part "
                                  "of an EnvSnapshot")

    def restore(self, snap, mask=None):
        raise NotImplementedError("EpisodeMonitor does not restore: its running episode sums would be "
                                  "wrong afterwards")

    def reset(self, mask=None):
        obs = self.env.reset(mask)
        if self.initial_reset_timestamp is None:
            self.initial_reset_timestamp = time.time()
        self.stats.restart(mask)
        if self._video_on and (mask is None or bool(np.asarray(self._host(mask))[self.video_env])):
            self._sync_episode_count()
            self._new_episode()
        return obs

    def step(self, actions):
        obs, reward, done, info = self.env.step(actions)
        if self._video_on:
            self._video_step(done)
        self.stats.update(reward, done)
        return obs, reward, done, info

    # ------------------------------------------------------------------ multi-step launches
    def _account_rollout(self, name, result):
        """Feed a rollout's reward and done [T, B] to the statistics; the forms are the env's
        (planes, scalars, reward, done), the wrapper's (features, reward, done, returns) and the
        dicts of rollout_features / rollout_policy."""
        if isinstance(result, dict):
            reward, done = result["reward"], result["done"]
        elif isinstance(result, tuple) and len(result) == 4:
            wrapper_form = result[1].dtype.is_floating_point
            reward, done = (result[1], result[2]) if wrapper_form else (result[2], result[3])
        else:
            raise TypeError("%s() of %s returned neither a 4-tuple nor a dict" % (name, type(self.env).__name__))
        self.stats.update_rollout(reward, done)
        return result

    def _rollout_call(self, name, args, kwargs):
        if self._video_on:
            raise NotImplementedError("EpisodeMonitor.%s() records no video: pass video_callable=False (or no "
                                      "directory), or step() the episodes to be filmed" % name)
        return self._account_rollout(name, getattr(self.env, name)(*args, **kwargs))

    def rollout(self, *args, **kwargs):
        """The wrapped env's or wrapper's rollout(), its episodes accounted; the result unchanged."""
        return self._rollout_call("rollout", args, kwargs)

    def rollout_features(self, *args, **kwargs):
        """The wrapped env's rollout_features(), its episodes accounted; the result unchanged."""
        return self._rollout_call("rollout_features", args, kwargs)

    def rollout_policy(self, *args, **kwargs):
        """The wrapped PragmaticObsWrapper's rollout_policy(), its episodes accounted; the result
        unchanged."""
        return self._rollout_call("rollout_policy", args, kwargs)

    # ------------------------------------------------------------------ video
    def _host(self, x):
        return x.cpu().numpy() if hasattr(x, "cpu") else x

    def _frame(self, obs=None):
        img = self.env.render(scale=self.video_scale, obs=obs, envs=(self.video_env, 1))
        return self._host(img[0])

    def _armed(self):
        """True when video_env's done flag must be read every step: its current episode is
        being recorded, or one of the next flush_every + 1 may be (an episode lasts >= 1 step,
        and the device count is read every flush_every unarmed steps)."""
        if self._rec is not None and self._rec.enabled:
            return True
        return any(self.video_callable(self.episode_id + k) for k in range(self.stats.flush_every + 1))

    def _sync_episode_count(self):
        """Fold the device-counted episode ends (unarmed steps) into episode_id."""
        if self._ep_dev is not None:
            n = int(self._ep_dev.item())
            self._ep_dev = None
            self._unsynced = 0
            for _ in range(n):  # (each ended episode started the next one, unrecorded)
                self._close_recorder()
                self.episode_id += 1

    def _new_episode(self):
        """gym's reset_video_recorder + episode_id bump: a recorder for the episode that
        starts now, its first frame captured."""
        self._close_recorder()
        base = os.path.join(self.directory, "openaigym.video.%s.video%06d" % (self._infix, self.episode_id))
        fps = getattr(self.env, "metadata", {}).get("video.frames_per_second", 30)
        self._rec = GifRecorder(base, {"episode_id": self.episode_id}, fps,
                                enabled=bool(self.video_callable(self.episode_id)))
        if self._rec.enabled:
            self._rec.capture_frame(self._frame())
        self.episode_id += 1

    def _close_recorder(self):
        if self._rec is not None:
            self._rec.close()
            if self._rec.functional:
                self.videos.append((self._rec.path, self._rec.metadata_path))
            self._rec = None

    def _video_step(self, done):
        t = self.stats._torch
        d_e = t.as_tensor(done, device=self.stats.device)[self.video_env]
        if not self._armed():
            if self._ep_dev is None:
                self._ep_dev = t.zeros((), dtype=t.int64, device=self.stats.device)
            self._ep_dev += d_e.to(t.int64)
            self._unsynced += 1
            if self._unsynced == self.stats.flush_every:  # (with the stats' own flush, normally)
                self._sync_episode_count()
            return
        self._sync_episode_count()
        if bool(d_e):
            if self._rec is not None and self._rec.enabled:
                term = getattr(self.env, "terminal_observation", None)
                if term is not None:
                    self._rec.capture_frame(self._frame(obs=term))
            self._new_episode()  # (the autoreset obs is the new episode's first)
        elif self._rec is not None and self._rec.enabled:
            self._rec.capture_frame(self._frame())

    def get_episode_rewards(self):
        self.stats.flush()
        return list(self.stats.episode_rewards)

    def get_episode_lengths(self):
        self.stats.flush()
        return list(self.stats.episode_lengths)

    def get_total_steps(self):
        return self.stats.total_steps

    def write_stats(self):
        """The stats file of gym 0.17's stats recorder (+ a manifest naming it)."""
        self.stats.flush()
        if self.directory is None:
            return None
        s = self.stats
        path = os.path.join(self.directory, "openaigym.episode_batch.%s.stats.json" % self._infix)
        with open(path, "w") as f:
            json.dump({"initial_reset_timestamp": self.initial_reset_timestamp,
                       "timestamps": s.timestamps, "episode_lengths": s.episode_lengths,
                       "episode_rewards": s.episode_rewards, "episode_types": s.episode_types}, f)
        spec = getattr(self.env, "spec", None)
        with open(os.path.join(self.directory, "openaigym.manifest.%s.manifest.json" % self._infix), "w") as f:
            json.dump({"stats": os.path.basename(path),
                       "videos": [(os.path.basename(v), os.path.basename(m)) for v, m in self.videos],
                       "env_info": {"env_id": getattr(spec, "id", None), "gym_version": "0.17.2 (restated)"}}, f)
        return path

    def close(self):
        self._close_recorder()
        path = self.write_stats()
        self.env.close()
        return path
