"""Time PPO's clipped loss and the evaluate pass against loss_and_grad on one rollout segment.

    python tools/ppo_time.py [--envs 65536] [--steps 64] [--batches 7]

tools/policy_grad_time.py's segment: B envs with the default options and the reference's network
(torch's default init), warmed up by one rollout_policy of 40 steps; one rollout_policy of T steps
with bootstrap_value=True, gae_lambda=0.95, whiten=True gives features [T, B, F], actions,
advantage, target and value.  old_logp is evaluate's, shifted by a fixed pattern so that rows of
every kind take part (the time does not depend on it: the head has no divergent work to speak of).
    loss_and_grad       DevicePolicy.loss_and_grad(into=model)                (wab_policy_grad)
    ppo_loss_and_grad   DevicePolicy.ppo_loss_and_grad(into=model), value clip on  (wab_policy_grad_ppo)
    evaluate            DevicePolicy.evaluate(features, actions)              (wab_policy_evaluate)
Each call is timed between two hipEvents on the stream and ends in a synchronise; the variants
alternate once per batch after a warm-up batch; medians of `batches` with min and max.  Prints one
JSON line.  On a tree whose DevicePolicy has no ppo_loss_and_grad (an earlier revision, for an
A/B of loss_and_grad in the same visit) it times loss_and_grad alone.  Exits non-zero when
ppo_loss_and_grad's median exceeds loss_and_grad's by more than loss_and_grad's own spread
(max - min), or when evaluate's median is not below loss_and_grad's.
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

    from wab_gym_amd.env import BatchedWolvesAndBushesEnv
    from wab_gym_amd.policy import DevicePolicy
    from wab_gym_amd.wrappers import PragmaticObsWrapper

    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--batches", type=int, default=7)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ppo_time needs a GPU: a time measured anywhere else says nothing")

    dev = torch.device("cuda:0")
    B, T = args.envs, args.steps
    env = BatchedWolvesAndBushesEnv(num_envs=B, device=dev)
    w = PragmaticObsWrapper(env)
    w.reset()
    torch.manual_seed(0)
    F, A = w.feature_dim, env.n_actions

    class Policy(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.affine1 = torch.nn.Linear(F, 128)
            self.affine2 = torch.nn.Linear(128, 150)
            self.affine3 = torch.nn.Linear(150, 128)
            self.action_head = torch.nn.Linear(128, A)
            self.value_head = torch.nn.Linear(128, 1)

    model = Policy().to(dev)
    pol = DevicePolicy(model, env)
    w.rollout_policy(pol, 40)
    r = w.rollout_policy(pol, T, bootstrap_value=True, gae_lambda=0.95, whiten=True)
    N = T * B
    feats, acts, adv, tgt, val = r["features"], r["actions"], r["advantage"], r["target"], r["value"]

    variants = {"loss_and_grad": lambda: pol.loss_and_grad(feats, acts, adv, tgt, into=model, reduction="mean")}
    res = {"envs": B, "steps": T, "rows": N, "batches": args.batches}
    if hasattr(pol, "ppo_loss_and_grad"):
        rows = torch.arange(N, device=dev).view(T, B)
        old_logp = (pol.evaluate(feats, acts)["logp"] + ((rows % 5) - 2).float() * 0.125).contiguous()
        old_value = (val + ((rows % 4).float() - 1.5) * 0.2).contiguous()
        out = pol.ppo_loss_and_grad(feats, acts, adv, tgt, old_logp, clip=0.2, old_value=old_value, value_clip=0.2,
                                    into=model, reduction="mean")
        pol.check()
        res["diagnostics"] = {k: float(out[k]) for k in ("clip_fraction", "approx_kl", "value_clip_fraction",
                                                         "ratio_mean")}
        variants["ppo_loss_and_grad"] = lambda: pol.ppo_loss_and_grad(
            feats, acts, adv, tgt, old_logp, clip=0.2, old_value=old_value, value_clip=0.2, into=model,
            reduction="mean")
        variants["evaluate"] = lambda: pol.evaluate(feats, acts)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    times = {k: [] for k in variants}
    for batch in range(args.batches + 1):
        for k, fn in variants.items():
            ms = timed(fn)
            if batch > 0:  # (batch 0 warms up)
                times[k].append(ms)
    for k, v in times.items():
        res[k + "_ms"] = {"median": statistics.median(v), "min": min(v), "max": max(v)}
        print("%-18s median %9.3f ms  (min %9.3f, max %9.3f)" % (k, statistics.median(v), min(v), max(v)))
    pol.check()
    print(json.dumps(res))
    if "ppo_loss_and_grad" in variants:
        base = res["loss_and_grad_ms"]
        if res["ppo_loss_and_grad_ms"]["median"] > base["median"] + (base["max"] - base["min"]):
            raise SystemExit("ppo_loss_and_grad is slower than loss_and_grad by more than its spread")
        if not res["evaluate_ms"]["median"] < base["median"]:
            raise SystemExit("evaluate is not faster than loss_and_grad")


if __name__ == "__main__":
    main()
