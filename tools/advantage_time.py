"""Time the advantages of one closed-loop rollout segment and their whitening.

    python tools/advantage_time.py [--envs 65536] [--steps 64] [--reps 10] [--batches 7]

One env of B envs with the default options and the reference's network (random init) is warmed up
by one rollout_policy of 40 steps, then one rollout_policy of T steps with bootstrap_value=True
gives the reward, done, value [T, B] and last_value [B] that the variants work on:
    (a) gae_torch   GAE as the T-step reverse loop in stock torch (float32, as a trainer writes it),
    (b) gae         gae(env=...) (wab_gae),
    (c) returns     discounted_returns(env=...) (wab_discounted_returns_exact): the yardstick, 9
                    bytes per env-step where (b) moves 17,
    (d) whiten_torch  (x - x.mean()) / (x.std() + eps) in torch,
    (e) whitened    whitened(x) (wab_whiten),
    (f) rollout, rollout_gae   rollout_policy(T) without and with bootstrap_value=True,
                    gae_lambda=0.95, whiten=True.
Each variant is first run eagerly, as a caller runs it: `reps` calls between two hipEvents on the
stream, ending in a synchronise, the variants alternating once per batch after a warm-up batch.
(b), (c) and (e) are then also captured as a graph of 10 x `reps` calls of their C entry point on
preallocated buffers and replayed the same way: the time of the kernels alone, from which (b)/(c)
is taken.  Prints every batch's time per call, medians and spreads, then one JSON line; exits
non-zero unless (b) < (a).
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    import torch

    from wab_gym_amd import _lib
    from wab_gym_amd.env import BatchedWolvesAndBushesEnv
    from wab_gym_amd.policy import DevicePolicy
    from wab_gym_amd.wrappers import PragmaticObsWrapper, discounted_returns, gae, whitened

    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--batches", type=int, default=7)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("advantage_time needs a GPU: a time measured anywhere else says nothing")

    dev = torch.device("cuda:0")
    B, T, reps = args.envs, args.steps, args.reps
    gamma, lam, eps = 0.99, 0.95, 1.1920928955078125e-07
    env = BatchedWolvesAndBushesEnv(num_envs=B, device=dev)
    w = PragmaticObsWrapper(env)
    w.reset()
    torch.manual_seed(0)
    F, A = w.feature_dim, env.n_actions
    sd = {}
    for name, (n_out, n_in) in (("affine1", (128, F)), ("affine2", (150, 128)), ("affine3", (128, 150)),
                                ("action_head", (A, 128)), ("value_head", (1, 128))):
        layer = torch.nn.Linear(n_in, n_out)
        sd[name + ".weight"], sd[name + ".bias"] = layer.weight.detach(), layer.bias.detach()
    pol = DevicePolicy(sd, env)
    w.rollout_policy(pol, 40, store_features=False)
    seg = w.rollout_policy(pol, T, gamma=gamma, store_features=False, bootstrap_value=True)
    reward, done, value, last = seg["reward"], seg["done"], seg["value"], seg["last_value"]
    episodes = int(done.sum())
    adv0, _ = gae(reward, done, value, last, gamma, lam, env=env)

    L = _lib.load()
    adv, tgt, ret_out, white = (torch.empty_like(reward) for _ in range(4))
    notdone = (done == 0).to(torch.float32)

    def gae_torch(i):
        a = torch.zeros(B, device=dev)
        vnext = last
        out = torch.empty_like(reward)
        for t in range(T - 1, -1, -1):
            delta = reward[t] + gamma * vnext * notdone[t] - value[t]
            a = delta + gamma * lam * notdone[t] * a
            out[t] = a
            vnext = value[t]
        return out, out + value

    def gae_hip(i):
        gae(reward, done, value, last, gamma, lam, env=env, advantage=adv, target=tgt)

    def returns_scan(i):
        discounted_returns(reward, done, gamma, bootstrap=last, out=ret_out, env=env)

    def whiten_torch(i):
        return (adv0 - adv0.mean()) / (adv0.std() + eps)

    def whiten_hip(i):
        whitened(adv0, eps, out=white)

    def rollout(i):
        w.rollout_policy(pol, T, gamma=gamma, store_features=False)

    def rollout_gae(i):
        w.rollout_policy(pol, T, gamma=gamma, store_features=False, bootstrap_value=True, gae_lambda=lam, whiten=True)

    ws = torch.empty(int(L.wab_whiten_workspace(T * B)) // 8, dtype=torch.float64, device=dev)

    def c_gae(i):
        _lib.check(L.wab_gae(env._h, reward.data_ptr(), done.data_ptr(), value.data_ptr(), last.data_ptr(), T, B, gamma,
                             lam, adv.data_ptr(), tgt.data_ptr(), env._stream()), "wab_gae")

    def c_returns(i):
        _lib.check(L.wab_discounted_returns_exact(env._h, reward.data_ptr(), done.data_ptr(), T, B, gamma,
                                                  last.data_ptr(), ret_out.data_ptr(), env._stream()),
                   "wab_discounted_returns_exact")

    def c_whiten(i):
        _lib.check(L.wab_whiten(adv0.data_ptr(), T * B, eps, white.data_ptr(), ws.data_ptr(), env._stream()),
                   "wab_whiten")

    eager = {"gae_torch": gae_torch, "gae": gae_hip, "returns": returns_scan, "whiten_torch": whiten_torch,
             "whitened": whiten_hip, "rollout": rollout, "rollout_gae": rollout_gae}
    captured = {"gae": c_gae, "returns": c_returns, "whitened": c_whiten}
    stream = torch.cuda.current_stream(dev)
    for fn in list(eager.values()) + list(captured.values()):
        for i in range(2):  # first calls: code objects loaded, the allocator's blocks made
            fn(i)
    torch.cuda.synchronize(dev)
    # the stock loop computes the same thing in float32
    ref = gae_torch(0)[0]
    err = float((ref - adv0).abs().max())
    assert err < 1e-3 * max(1.0, float(adv0.abs().max())), err
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
        print("%-5s %-12s us per call, by batch: %s   median %.1f  (min %.1f, max %.1f)"
              % (mode, k, " ".join("%.1f" % x for x in v), med[(mode, k)], min(v), max(v)))
    a, b_, d, e = (med[("eager", k)] for k in ("gae_torch", "gae", "whiten_torch", "whitened"))
    f0, f1 = med[("eager", "rollout")], med[("eager", "rollout_gae")]
    gb, gc, ge = (med[("graph", k)] for k in ("gae", "returns", "whitened"))
    print("segment %d x %d, %d episodes finished; eager (a)/(b) %.1f, (e)/(d) %.2f; kernels alone (b)/(c) %.2f; "
          "rollout_policy %.1f -> %.1f us (+%.1f)" % (T, B, episodes, a / b_, e / d, gb / gc, f0, f1, f1 - f0))
    print(json.dumps({"envs": B, "steps": T, "reps": reps, "batches": args.batches, "episodes": episodes,
                      "eager_us": {k: round(med[("eager", k)], 2) for k in eager},
                      "graph_us": {k: round(med[("graph", k)], 2) for k in graphs},
                      "spread_us": {"%s_%s" % key: [round(min(v), 2), round(max(v), 2)] for key, v in times.items()},
                      "gae_over_returns": round(gb / gc, 2), "whitened_over_torch": round(e / d, 2),
                      "gae_torch_over_gae": round(a / b_, 2), "rollout_gae_minus_rollout_us": round(f1 - f0, 2)}))
    if not b_ < a:
        raise SystemExit("gate failed: (b) %.1f us must be below (a) %.1f us" % (b_, a))


if __name__ == "__main__":
    main()
