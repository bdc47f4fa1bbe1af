"""Time the device policy (wab_policy_act) against its floor and against the stock-torch policy.

    python tools/policy_rate.py [--envs 65536] [--reps 20] [--batches 7] [--steps 64]

One env of B envs with the default options (449 features) and the reference's 449-128-150-128-5
network.  Eight variants, each captured as a graph of `reps` calls and replayed, alternating, once
per batch between two hipEvents on the stream, after a warm-up replay of each:
    act     (a) wab_policy_act alone (probs and value written too),
    loop    (b) the closed-loop step: wab_policy_act, then wab_step_features without planes,
    read    (c) a plain device read of the same [B, 449] float32 array (torch.sum): the floor of (a),
    torch   (d) the stock-torch act() of bench.py's make_policy (imported, not copied),
    fusedS  (e) the fused closed loop, wab_rollout_policy as one launch of --steps steps with the
                feature rows stored ([T, B, 449] float32),
    fusedN  (f) the same with features = NULL (no intermediate row leaves the chip),
    fusedP  the same with the rows stored packed, 1 bit per feature (wab_rollout_policy_packed:
            [T, B, 16] uint32, 64 bytes per row instead of 1796; the call's wab_features_pack
            launch for slice 0 is part of the time),
    roll    the floor of (e): wab_rollout_features, the same launch with pre-chosen actions and no
            policy (the env steps and the feature stores that (e) contains).
(e), (f), fusedP and roll are reported per step (a call's time / --steps), so they compare with (b).
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
    ap.add_argument("--steps", type=int, default=64, help="T of the multi-step variants")
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

    # the multi-step variants, through the C entry points on preallocated buffers
    import ctypes

    from wab_gym_amd import _lib

    L = _lib.load()
    T = args.steps
    if L.wab_rollout_policy_fused(env._h, pol._p) != 1:
        raise SystemExit("wab_rollout_policy is not one launch here: " + L.wab_last_error().decode())
    seq = torch.empty((T, B, F), device=dev)
    seq_actions = torch.as_tensor(rng.randint(env.n_actions, size=(T, B)).astype(np.int8), device=dev)
    pol_actions = torch.empty((T, B), dtype=torch.int8, device=dev)
    seq_value = torch.empty((T, B), device=dev)
    seq_probs = torch.empty((T, B, env.n_actions), device=dev)  # (written as (b) writes its probs)
    seq_reward = torch.empty((T, B), device=dev)
    seq_done = torch.empty((T, B), dtype=torch.uint8, device=dev)
    seq_scal = torch.empty((3, T, B), dtype=torch.uint8, device=dev)
    seq_obs = _lib.WabObs(None, seq_scal[0].data_ptr(), seq_scal[1].data_ptr(), seq_scal[2].data_ptr())
    fused_feats = w.features.clone()  # features0 and features_last of every call: a continuing rollout

    def fused(features):
        _lib.check(L.wab_rollout_policy(env._h, pol._p, fused_feats.data_ptr(), T, ctypes.addressof(seq_obs),
                                        pol_actions.data_ptr(), seq_value.data_ptr(), seq_probs.data_ptr(),
                                        seq_reward.data_ptr(),
                                        seq_done.data_ptr(), features, fused_feats.data_ptr(), 0.99, None, None,
                                        env._stream()), "wab_rollout_policy")

    def fused_stored(i):
        fused(seq.data_ptr())

    def fused_null(i):
        fused(None)

    seq_bits = torch.empty((T, B, L.wab_feature_bits_pitch(F)), dtype=torch.int32, device=dev)

    def fused_packed(i):
        _lib.check(L.wab_rollout_policy_packed(env._h, pol._p, fused_feats.data_ptr(), T, ctypes.addressof(seq_obs),
                                               pol_actions.data_ptr(), seq_value.data_ptr(), seq_probs.data_ptr(),
                                               seq_reward.data_ptr(), seq_done.data_ptr(), seq_bits.data_ptr(),
                                               fused_feats.data_ptr(), 0.99, None, None, env._stream()),
                   "wab_rollout_policy_packed")

    def roll(i):
        _lib.check(L.wab_rollout_features(env._h, seq_actions.data_ptr(), T, ctypes.addressof(seq_obs),
                                          seq_reward.data_ptr(), seq_done.data_ptr(), seq.data_ptr(), 0.99, None, None,
                                          env._stream()), "wab_rollout_features")

    per_call = {"fusedS": T, "fusedN": T, "fusedP": T, "roll": T}  # steps per call
    env.validate_actions = False  # (the policy's actions are in range; no per-step host check)
    variants = {"act": act, "loop": loop, "read": read, "torch": stock_act, "fusedS": fused_stored,
                "fusedN": fused_null, "fusedP": fused_packed, "roll": roll}
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
                for i in range(reps if name not in per_call else max(1, reps // 4)):
                    fn(i)
        stream.wait_stream(side)
        graphs[name] = g

    def batch(name):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        graphs[name].replay()
        e1.record(stream)
        e1.synchronize()
        if name in per_call:  # us per step
            return e0.elapsed_time(e1) * 1e3 / (max(1, reps // 4) * per_call[name])
        return e0.elapsed_time(e1) * 1e3 / reps  # us per call

    for k in graphs:
        batch(k)
    times = {k: [] for k in graphs}
    for _ in range(args.batches):
        for k in graphs:
            times[k].append(batch(k))
    c = env.counters()
    assert c["bad_actions"] == 0 and c["handoff_timeouts"] == 0, c

    med = {k: statistics.median(v) for k, v in times.items()}
    for k, v in times.items():
        print("%-6s us per call (fusedS, fusedN, fusedP, roll: per step), by batch: %s   median %.1f  (min %.1f, max %.1f)"
              % (k, " ".join("%.1f" % x for x in v), med[k], min(v), max(v)))
    nbytes = B * F * 4
    print("features: %d bytes per call; read %.0f GB/s, act %.0f GB/s" % (nbytes, nbytes / med["read"] / 1e3,
                                                                        nbytes / med["act"] / 1e3))
    print(json.dumps({"envs": B, "features": F, "reps": reps, "batches": args.batches, "kernel": env.step_kernel,
                      "act_us": round(med["act"], 2), "loop_us": round(med["loop"], 2),
                      "read_us": round(med["read"], 2), "torch_us": round(med["torch"], 2), "steps": T,
                      "fused_stored_us": round(med["fusedS"], 2), "fused_null_us": round(med["fusedN"], 2),
                      "fused_packed_us": round(med["fusedP"], 2), "roll_features_us": round(med["roll"], 2),
                      "spread_us": {k: [round(min(v), 2), round(max(v), 2)] for k, v in times.items()},
                      "act_over_read": round(med["act"] / med["read"], 2),
                      "torch_over_act": round(med["torch"] / med["act"], 2)}))


if __name__ == "__main__":
    main()
