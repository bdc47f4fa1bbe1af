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

    python tools/ppo_time.py --gather [--parent parent.json] [--out new.json]

times one minibatch of T B / 4 rows of the same segment instead, the variants alternating in the
same way:
    a   ppo_loss_and_grad on the contiguous quarter features[t0:t1]
    b   ppo_loss_and_grad(rows=perm[:n]), perm a random permutation of all T B rows
    c   what a caller without rows= has to do, all of it inside the timed span: index_select of the
        features and of the five per-row arrays into preallocated buffers, then the contiguous call
    d   b with rows = arange(n): the index's own cost, without the scattered rows
    eval_a, eval_b, eval_d   the same three for evaluate
On a tree without rows= it times a, c and eval_a alone (the parent's side of an A/B; --out keeps
its JSON line for --parent).  Exits non-zero when b's median is not below c's, or, with --parent,
when a's median exceeds the parent's a by more than the parent's own spread (max - min).
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
    ap.add_argument("--gather", action="store_true", help="one minibatch of T B / 4 rows: contiguous, by index, by copies")
    ap.add_argument("--parent", help="--gather: the JSON line of the parent's run (its --out)")
    ap.add_argument("--out", help="write the JSON line to this file too")
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
    if args.gather:
        import inspect

        variants = gather_variants(torch, pol, model, r, T, B,
                                   "rows" in inspect.signature(pol.ppo_loss_and_grad).parameters)
        res["minibatch_rows"] = N // 4
    elif hasattr(pol, "ppo_loss_and_grad"):
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
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res) + "\n")
    if args.gather:
        med = {k: res[k + "_ms"]["median"] for k in variants}
        if "b" in med:
            for pair in (("b", "a"), ("d", "a"), ("eval_b", "eval_a"), ("eval_d", "eval_a"), ("b", "c")):
                print("%s / %s = %.4f" % (pair + (med[pair[0]] / med[pair[1]],)))
            if not med["b"] < med["c"]:
                raise SystemExit("rows= (b) is not faster than index_select copies and the contiguous call (c)")
        if args.parent:
            base = json.loads(open(args.parent).read().strip().splitlines()[-1])["a_ms"]
            print("a: %.3f ms, the parent's %.3f (min %.3f, max %.3f)" % (med["a"], base["median"], base["min"], base["max"]))
            if med["a"] > base["median"] + (base["max"] - base["min"]):
                raise SystemExit("the contiguous call (a) is slower than the parent's by more than the parent's spread")
        return
    if "ppo_loss_and_grad" in variants:
        base = res["loss_and_grad_ms"]
        if res["ppo_loss_and_grad_ms"]["median"] > base["median"] + (base["max"] - base["min"]):
            raise SystemExit("ppo_loss_and_grad is slower than loss_and_grad by more than its spread")
        if not res["evaluate_ms"]["median"] < base["median"]:
            raise SystemExit("evaluate is not faster than loss_and_grad")


def gather_variants(torch, pol, model, r, T, B, has_rows):
    """The --gather variants over one minibatch of T B / 4 rows of the segment r."""
    feats, acts, adv, tgt, val = r["features"], r["actions"], r["advantage"], r["target"], r["value"]
    dev, N = feats.device, T * B
    n, t1 = N // 4, T // 4
    i = torch.arange(N, device=dev).view(T, B)
    old_logp = (pol.evaluate(feats, acts)["logp"] + ((i % 5) - 2).float() * 0.125).contiguous()
    old_value = (val + ((i % 4).float() - 1.5) * 0.2).contiguous()
    kw = dict(clip=0.2, value_clip=0.2, into=model, reduction="mean")
    per_row = (acts, adv, tgt, old_logp, old_value)

    def contiguous():
        return pol.ppo_loss_and_grad(feats[:t1], acts[:t1], adv[:t1], tgt[:t1], old_logp[:t1], old_value=old_value[:t1],
                                     **kw)

    torch.manual_seed(1)
    perm = torch.randperm(N, device=dev, dtype=torch.int32)
    idx64 = perm[:n].long()  # (index_select's index type; made once, outside the timed span)
    bufs = [torch.empty((n,) + tuple(x.shape[2:]), dtype=x.dtype, device=dev) for x in (feats,) + per_row]

    def copies():
        torch.index_select(feats.view(N, -1), 0, idx64, out=bufs[0])
        for x, b in zip(per_row, bufs[1:]):
            torch.index_select(x.view(N), 0, idx64, out=b)
        return pol.ppo_loss_and_grad(bufs[0], bufs[1], bufs[2], bufs[3], bufs[4], old_value=bufs[5], **kw)

    variants = {"a": contiguous, "c": copies, "eval_a": lambda: pol.evaluate(feats[:t1], acts[:t1])}
    if has_rows:
        ident = torch.arange(n, device=dev, dtype=torch.int32)

        def by_index(rows):
            return lambda: pol.ppo_loss_and_grad(feats, acts, adv, tgt, old_logp, old_value=old_value, rows=rows, **kw)

        variants = {"a": contiguous, "b": by_index(perm[:n]), "c": copies, "d": by_index(ident),
                    "eval_a": variants["eval_a"], "eval_b": lambda: pol.evaluate(feats, acts, rows=perm[:n]),
                    "eval_d": lambda: pol.evaluate(feats, acts, rows=ident)}
        # b and c compute the same thing
        want, got = copies(), variants["b"]()
        assert all(torch.equal(want[k], got[k]) for k in ("loss", "ppo_sums")), "rows= differs from the copies"
    return variants


if __name__ == "__main__":
    main()
