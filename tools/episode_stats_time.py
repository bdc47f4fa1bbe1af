"""Time the episode statistics and the per-episode normalisation of one rollout segment.

    python tools/episode_stats_time.py [--envs 65536] [--steps 64] [--reps 10] [--batches 7]

One env of B envs with the default options is warmed up for 40 steps, then one env.rollout of T
steps gives the reward and done [T, B] (and discounted_returns their returns) that every variant
works on:
    (a) update      T calls of EpisodeStats.update, the per-step path,
    (b) rollout     one EpisodeStats.update_rollout (wab_episode_stats_update),
    (c) returns     discounted_returns(env=...) (wab_discounted_returns_exact): the yardstick, one
                    pass over the same 5 bytes per env-step,
    (d) normalize   normalize_episode_returns, the torch scatter_add version,
    (e) normalized  normalized_returns (wab_normalize_episode_returns).
Each variant is first run eagerly, as a caller runs it: `reps` calls between two hipEvents on the
stream, ending in a synchronise, the variants alternating once per batch after a warm-up batch.
That time holds the host's work per launch.  (b), (c) and (e) are then also captured as a graph of
10 x `reps` calls of their C entry point on preallocated buffers and replayed the same way: the time
of the kernels alone, from which the ratios (b)/(c) and (e)/(c) are taken.  The gather of the
finished episodes (flush(), a host synchronisation) is timed in neither (a) nor (b): (a)'s
pending entries and (b)'s queued segment are dropped after every call.
Prints every batch's time per call, medians and spreads, then one JSON line; exits non-zero unless
(b) < (a) and (e) < (d).
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    import numpy as np
    import torch

    from wab_gym_amd import _lib
    from wab_gym_amd.env import BatchedWolvesAndBushesEnv
    from wab_gym_amd.monitor import EpisodeStats
    from wab_gym_amd.wrappers import discounted_returns, normalize_episode_returns, normalized_returns

    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--batches", type=int, default=7)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("episode_stats_time needs a GPU: a time measured anywhere else says nothing")

    dev = torch.device("cuda:0")
    B, T, reps = args.envs, args.steps, args.reps
    env = BatchedWolvesAndBushesEnv(num_envs=B, device=dev)
    env.reset()
    rng = np.random.RandomState(0)
    for _ in range(40):
        env.step(torch.as_tensor(rng.randint(env.n_actions, size=B)))
    _, _, reward, done = env.rollout(torch.as_tensor(rng.randint(env.n_actions, size=(T, B)).astype(np.int8)))
    reward, done = reward.clone(), done.clone()  # (the planes of the rollout are released)
    returns = discounted_returns(reward, done, env=env)
    done_bool = done.view(torch.bool)
    episodes = int(done.sum())

    L = _lib.load()
    per_step = EpisodeStats(env.game_options, B, dev, flush_every=T + 1)
    whole = EpisodeStats(env.game_options, B, dev, handle=env._h)
    ret_out, norm_out = torch.empty_like(returns), torch.empty_like(returns)

    def update(i):
        for t in range(T):
            per_step.update(reward[t], done_bool[t])
        per_step._times = []  # (dropped, not gathered)

    def rollout(i):
        whole.update_rollout(reward, done)
        whole._queue.clear()

    def returns_scan(i):
        discounted_returns(reward, done, out=ret_out, env=env)

    def normalize(i):
        normalize_episode_returns(returns, done)

    def normalized(i):
        normalized_returns(returns, done, out=norm_out)

    # the C entry points on preallocated buffers, for the graphs
    cap = T * B
    ws = torch.empty(int(L.wab_episode_stats_workspace(T, B)) // 8 + 1, dtype=torch.int64, device=dev)
    g_ret = torch.zeros(B, dtype=torch.float64, device=dev)
    g_len = torch.zeros(B, dtype=torch.int64, device=dev)
    ep_ret = torch.empty(cap, dtype=torch.float64, device=dev)
    ep_i32 = torch.empty((3, cap), dtype=torch.int32, device=dev)
    count = torch.zeros(2, dtype=torch.int64, device=dev)

    def c_rollout(i):
        _lib.check(L.wab_episode_stats_update(env._h, reward.data_ptr(), done.data_ptr(), T, B, g_ret.data_ptr(),
                                              g_len.data_ptr(), ep_ret.data_ptr(), ep_i32[0].data_ptr(),
                                              ep_i32[1].data_ptr(), ep_i32[2].data_ptr(), cap, count.data_ptr(),
                                              ws.data_ptr(), env._stream()), "wab_episode_stats_update")

    def c_returns(i):
        _lib.check(L.wab_discounted_returns_exact(env._h, reward.data_ptr(), done.data_ptr(), T, B, 0.99, None,
                                                  ret_out.data_ptr(), env._stream()), "wab_discounted_returns_exact")

    def c_normalized(i):
        _lib.check(L.wab_normalize_episode_returns(returns.data_ptr(), done.data_ptr(), T, B,
                                                   1.1920928955078125e-07, norm_out.data_ptr(), env._stream()),
                   "wab_normalize_episode_returns")

    eager = {"update": update, "rollout": rollout, "returns": returns_scan, "normalize": normalize,
             "normalized": normalized}
    captured = {"rollout": c_rollout, "returns": c_returns, "normalized": c_normalized}
    stream = torch.cuda.current_stream(dev)
    for fn in list(eager.values()) + list(captured.values()):
        for i in range(2):  # first calls: code objects loaded, the allocator's blocks made
            fn(i)
    torch.cuda.synchronize(dev)
    assert int(count[0]) == episodes and int(count[1]) == episodes, (count, episodes)
    graphs = {}
    for name, fn in captured.items():
        g = torch.cuda.CUDAGraph()
        side = torch.cuda.Stream(dev)
        side.wait_stream(stream)
        with torch.cuda.stream(side):
            with torch.cuda.graph(g, stream=side):
                for i in range(10 * reps):
                    fn(i)
        stream.wait_stream(side)
        graphs[name] = g

    def timed(run, calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        run()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / calls  # us per call

    def eager_batch(name):
        def run():
            for i in range(reps):
                eager[name](i)
        return timed(run, reps)

    runs = [("eager", k, lambda k=k: eager_batch(k)) for k in eager]
    runs += [("graph", k, lambda k=k: timed(graphs[k].replay, 10 * reps)) for k in graphs]
    times = {(mode, k): [] for mode, k, _ in runs}
    for b in range(args.batches + 1):
        for mode, k, fn in runs:
            us = fn()
            if b > 0:  # (batch 0 warms up)
                times[(mode, k)].append(us)
    med = {key: statistics.median(v) for key, v in times.items()}
    for (mode, k), v in times.items():
        print("%-5s %-10s us per call, by batch: %s   median %.1f  (min %.1f, max %.1f)"
              % (mode, k, " ".join("%.1f" % x for x in v), med[(mode, k)], min(v), max(v)))
    a, b_, d, e = (med[("eager", k)] for k in ("update", "rollout", "normalize", "normalized"))
    gb, gc, ge = (med[("graph", k)] for k in ("rollout", "returns", "normalized"))
    print("segment %d x %d, %d episodes finished; (a)/(b) %.1f, (d)/(e) %.1f eager; kernels alone (b)/(c) %.2f, "
          "(e)/(c) %.2f" % (T, B, episodes, a / b_, d / e, gb / gc, ge / gc))
    print(json.dumps({"envs": B, "steps": T, "reps": reps, "batches": args.batches, "episodes": episodes,
                      "eager_us": {k: round(med[("eager", k)], 2) for k in eager},
                      "graph_us": {k: round(med[("graph", k)], 2) for k in graphs},
                      "spread_us": {"%s_%s" % key: [round(min(v), 2), round(max(v), 2)] for key, v in times.items()},
                      "rollout_over_returns": round(gb / gc, 2), "normalized_over_returns": round(ge / gc, 2),
                      "update_over_rollout": round(a / b_, 2), "normalize_over_normalized": round(d / e, 2)}))
    if not (b_ < a and e < d):
        raise SystemExit("gate failed: (b) %.1f us must be below (a) %.1f us, (e) %.1f us below (d) %.1f us"
                         % (b_, a, e, d))


if __name__ == "__main__":
    main()
