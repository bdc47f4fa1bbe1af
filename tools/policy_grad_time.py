"""Time the actor-critic update's loss and backward pass on one closed-loop rollout segment.

    python tools/policy_grad_time.py [--envs 65536] [--steps 64] [--batches 7]

One env of B envs with the default options and the reference's network (torch's default init) is
warmed up by one rollout_policy of 40 steps; one rollout_policy of T steps with
bootstrap_value=True, gae_lambda=0.95, whiten=True then gives the features [T, B, F], actions,
advantage and target that every variant works on:
    (a) torch_fp32   stock torch: fp32 forward over the T B rows, the same loss, backward(),
    (b) loss_and_grad, eager   DevicePolicy.loss_and_grad(into=model) (wab_policy_grad),
    (b) loss_and_grad, graph   the same call captured once and replayed,
    (c) torch_bf16   (a) under torch.autocast(bfloat16): for information only,
    (d) evaluate, loss_and_grad and ppo_loss_and_grad, eager, on the float rows and on the same
        rows packed to 1 bit per feature (wab_gym_amd.features; the *_packed lines), each over the
        contiguous rows and through rows= (a permutation of the T B rows; the *_rows lines).
Each call is timed between two hipEvents on the stream and ends in a synchronise; the variants
alternate once per batch after a warm-up batch; medians of `batches` with min and max.  (b) is
also set against the bytes it must move (the features twice, the bf16 workspace once out and once
in) at the 6.3 TB/s a streaming copy achieves.  Prints one JSON line; exits non-zero unless
(b) eager < (a).
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
    import torch.nn.functional as Fn

    from wab_gym_amd.env import BatchedWolvesAndBushesEnv
    from wab_gym_amd.policy import LAYERS, DevicePolicy
    from wab_gym_amd.wrappers import PragmaticObsWrapper

    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--batches", type=int, default=7)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("policy_grad_time needs a GPU: a time measured anywhere else says nothing")

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

        def forward(self, x):
            x = Fn.leaky_relu(self.affine1(x))
            x = Fn.leaky_relu(self.affine2(x))
            x = torch.clamp(Fn.leaky_relu(self.affine3(x)), -4, 4)
            return Fn.log_softmax(self.action_head(x), dim=-1), self.value_head(x)[:, 0]

    model = Policy().to(dev)
    pol = DevicePolicy(model, env)
    w.rollout_policy(pol, 40)
    r = w.rollout_policy(pol, T, bootstrap_value=True, gae_lambda=0.95, whiten=True)
    N = T * B
    feats, acts = r["features"], r["actions"]
    adv, tgt = r["advantage"], r["target"]
    x2, a2 = feats.view(N, F), acts.view(N).long()
    adv1, tgt1 = adv.view(N), tgt.view(N)

    def torch_update(autocast):
        for p in model.parameters():
            p.grad = None
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
            logp_all, v = model(x2)
        logp = logp_all.float().gather(1, a2[:, None])[:, 0]
        loss = (-(adv1 * logp).sum() + Fn.smooth_l1_loss(v.float(), tgt1, reduction="sum")) / N
        loss.backward()
        return loss

    def device_update():
        return pol.loss_and_grad(feats, acts, adv, tgt, into=model, reduction="mean")["loss"]

    # the two agree on what they compute (bf16 operands against fp32: a loose check, printed)
    l_t = float(torch_update(False))
    g_t = model.affine2.weight.grad.clone()
    l_d = float(device_update())
    g_d = model.affine2.weight.grad
    print("loss: torch fp32 %.6f, loss_and_grad %.6f; affine2.weight.grad max |diff| %.3e of max %.3e"
          % (l_t, l_d, float((g_t - g_d).abs().max()), float(g_t.abs().max())))
    pol.check()
    assert abs(l_t - l_d) <= 0.02 * max(abs(l_t), 1e-3), (l_t, l_d)

    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph):
        device_update()

    # (d): the float rows and the same rows packed, contiguous and through an index
    from wab_gym_amd.features import pack_features

    bits = pack_features(feats)
    perm = torch.randperm(N, device=dev, dtype=torch.int32)
    old_logp = pol.evaluate(feats, acts)["logp"]

    def family(name, rows_of):
        def ev(x, rows):
            return lambda: pol.evaluate(x, acts, rows=rows)

        def lg(x, rows):
            return lambda: pol.loss_and_grad(x, acts, adv, tgt, into=model, reduction="mean", rows=rows)

        def ppo(x, rows):
            return lambda: pol.ppo_loss_and_grad(x, acts, adv, tgt, old_logp, clip=0.2, old_value=r["value"],
                                                 value_clip=0.2, into=model, reduction="mean", rows=rows)

        make = {"evaluate": ev, "loss_and_grad": lg, "ppo_loss_and_grad": ppo}[name]
        return {name + sfx: make(x, rows_of(tag)) for sfx, x, tag in
                (("", feats, 0), ("_packed", bits, 0), ("_rows", feats, 1), ("_rows_packed", bits, 1))}

    extra = {}
    for name in ("evaluate", "loss_and_grad", "ppo_loss_and_grad"):
        extra.update(family(name, lambda tag: perm if tag else None))
    extra.pop("loss_and_grad")  # (loss_and_grad_eager above)

    variants = {
        "torch_fp32": lambda: torch_update(False),
        "loss_and_grad_eager": device_update,
        "loss_and_grad_graph": graph.replay,
        "torch_bf16_autocast": lambda: torch_update(True),
    }
    variants.update(extra)

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
    res = {"envs": B, "steps": T, "rows": N, "batches": args.batches}
    for k, v in times.items():
        res[k + "_ms"] = {"median": statistics.median(v), "min": min(v), "max": max(v)}
        print("%-22s median %9.3f ms  (min %9.3f, max %9.3f)" % (k, statistics.median(v), min(v), max(v)))
    units = 2 * (128 + 160 + 128) + 16  # X_1..3, D_1..3 padded to the tile, D_4: bf16 per row
    must = 2 * N * F * 4 + 2 * N * units * 2
    floor_ms = must / 6.3e12 * 1e3
    res["feature_bytes"] = {"float": N * F * 4, "packed": bits.numel() * 4}
    res["bytes_must_move"] = must
    res["floor_ms_at_6.3TBps"] = floor_ms
    res["eager_over_floor"] = res["loss_and_grad_eager_ms"]["median"] / floor_ms
    res["graph_over_floor"] = res["loss_and_grad_graph_ms"]["median"] / floor_ms
    res["speedup_vs_torch_fp32"] = res["torch_fp32_ms"]["median"] / res["loss_and_grad_eager_ms"]["median"]
    print(json.dumps(res))
    if not res["loss_and_grad_eager_ms"]["median"] < res["torch_fp32_ms"]["median"]:
        raise SystemExit("loss_and_grad is not faster than stock torch fp32")


if __name__ == "__main__":
    main()
