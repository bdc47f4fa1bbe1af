"""Time the device policy (wab_policy_act) against its floor and against the stock-torch policy.

    python tools/policy_rate.py [--envs 65536] [--reps 20] [--batches 7]

One env of B envs with the default options (449 features) and the reference's 449-128-150-128-5
network.  Four variants, each captured as a graph of `reps` calls and replayed, alternating, once
per batch between two hipEvents on the stream, after a warm-up replay of each:
    act     (a) wab_policy_act alone (probs and value written too),
    loop    (b) the closed-loop step: wab_policy_act, then wab_step_features without planes,
    read    (c) a plain device read of the same [B, 449] float32 array (torch.sum): the floor of (a),
    torch   (d) the stock-torch act() of bench.py's make_policy (imported, not copied).
(a), (c) and (d) read a ring of four feature buffers (4 x 118 MB at B = 65536, more than the
256 MB Infinity Cache), so that a call's features come from HBM as they do behind a step; (b)
reads what its own step just wrote.  Prints every batch's per-call time, the median and the
spread of each variant, the ratios (a)/(c) and (d)/(a), and one JSON line.
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

    import bench
    from wab_gym_amd.env import BatchedWolvesAndBushesEnv
    from wab_gym_amd.policy import DevicePolicy
    from wab_gym_amd.wrappers import PragmaticObsWrapper

    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--batches", type=int, default=7)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("policy_rate needs a GPU: a time measured anywhere else says nothing")

    dev = torch.device("cuda:0")
    B, reps = args.envs, args.reps
    env = BatchedWolvesAndBushesEnv(num_envs=B, device=dev)
    w = PragmaticObsWrapper(env)
    w.reset()
    rng = np.random.RandomState(0)
    for _ in range(10):
        w.step(torch.as_tensor(rng.randint(env.n_actions, size=B)))
    F = w.feature_dim
    stock = bench.make_policy(F, env.n_actions, dev)
    pol = DevicePolicy(stock, env)  # the same weights
    ring = [w.features.clone() for _ in range(4)]
    actions = torch.zeros(B, dtype=torch.int8, device=dev)
    probs = torch.empty((B, env.n_actions), device=dev)
    value = torch.empty(B, device=dev)
    total = torch.zeros((), device=dev)
    loop_feats = w.features.clone()

    def act(i):
        pol.act(ring[i % 4], out=actions, probs=probs, value=value)

    def loop(i):
        pol.act(loop_feats, out=actions, probs=probs, value=value)
        env.step_features(actions, loop_feats, store_planes=False)

    def read(i):
        torch.sum(ring[i % 4].view(-1), (0,), out=total)

    def stock_act(i):
        stock.act(ring[i % 4], actions)

    env.validate_actions = False  # (the policy's actions are in range; no per-step host check)
    variants = {"act": act, "loop": loop, "read": read, "torch": stock_act}
    stream = torch.cuda.current_stream(dev)
    graphs = {}
    for name, fn in variants.items():
        for i in range(2):  # eager first: code objects loaded, libraries' algorithms picked
            fn(i)
        torch.cuda.synchronize(dev)
        g = torch.cuda.CUDAGraph()
        side = torch.cuda.Stream(dev)
        side.wait_stream(stream)
        with torch.cuda.stream(side):
            with torch.cuda.graph(g, stream=side):
                for i in range(reps):
                    fn(i)
        stream.wait_stream(side)
        graphs[name] = g

    def batch(g):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        g.replay()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / reps  # us per call

    for g in graphs.values():
        batch(g)
    times = {k: [] for k in graphs}
    for _ in range(args.batches):
        for k, g in graphs.items():
            times[k].append(batch(g))
    c = env.counters()
    assert c["bad_actions"] == 0 and c["handoff_timeouts"] == 0, c

    med = {k: statistics.median(v) for k, v in times.items()}
    for k, v in times.items():
        print("%-6s us per call, by batch: %s   median %.1f  (min %.1f, max %.1f)"
              % (k, " ".join("%.1f" % x for x in v), med[k], min(v), max(v)))
    nbytes = B * F * 4
    print("features: %d bytes per call; read %.0f GB/s, act %.0f GB/s" % (nbytes, nbytes / med["read"] / 1e3,
                                                                        nbytes / med["act"] / 1e3))
    print(json.dumps({"envs": B, "features": F, "reps": reps, "batches": args.batches, "kernel": env.step_kernel,
                      "act_us": round(med["act"], 2), "loop_us": round(med["loop"], 2),
                      "read_us": round(med["read"], 2), "torch_us": round(med["torch"], 2),
                      "spread_us": {k: [round(min(v), 2), round(max(v), 2)] for k, v in times.items()},
                      "act_over_read": round(med["act"] / med["read"], 2),
                      "torch_over_act": round(med["torch"] / med["act"], 2)}))


if __name__ == "__main__":
    main()
