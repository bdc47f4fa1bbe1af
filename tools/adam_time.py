"""Time the tail of the actor-critic update at the reference net: the optimizer step and the
re-pack of the policy's weights.

    python tools/adam_time.py [--iters 200] [--runs 3]

Two variants on the same model (449-128-150-128-{5, 1}, torch's default init) and the same fixed
gradients (seeded normal, so every step does real work):
    (a) torch   torch.optim.Adam.step() followed by DevicePolicy.load(model),
    (b) device  DeviceAdam.step() (wab_policy_adam_step: the step and the re-pack),
    (b) graph   the same captured once and replayed (for information).
A run is `iters` back-to-back calls between two events on the stream, ending in a synchronise; the
variants alternate, run by run, after a warm-up run of each; per variant the per-call time of each
run is reported (microseconds).  The launch counts come from torch's profiler over ten calls, in
a pass of its own after the timing.  Prints one JSON line; exits non-zero if (b)'s slowest run is
slower than (a)'s fastest.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    import torch

    from wab_gym_amd.env import BatchedWolvesAndBushesEnv
    from wab_gym_amd.policy import DeviceAdam, DevicePolicy

    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--runs", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("adam_time needs a GPU: a time measured anywhere else says nothing")
    dev = torch.device("cuda:0")
    env = BatchedWolvesAndBushesEnv(num_envs=256, device=dev)
    env.reset()

    def make():
        torch.manual_seed(0)
        model = torch.nn.Module()
        for name, (i, o) in (("affine1", (449, 128)), ("affine2", (128, 150)), ("affine3", (150, 128)),
                             ("action_head", (128, env.n_actions)), ("value_head", (128, 1))):
            model.add_module(name, torch.nn.Linear(i, o))
        model = model.to(dev)
        g = torch.Generator(device=dev).manual_seed(1)
        for p in model.parameters():
            p.grad = torch.randn(p.shape, generator=g, device=dev) * 1e-2
        return model, DevicePolicy(model, env)

    model_t, pol_t = make()
    opt_t = torch.optim.Adam(model_t.parameters(), lr=3e-4)
    model_d, pol_d = make()
    opt_d = DeviceAdam(pol_d, model_d, lr=3e-4)
    model_g, pol_g = make()
    opt_g = DeviceAdam(pol_g, model_g, lr=3e-4)

    def torch_tail():
        opt_t.step()
        pol_t.load(model_t)

    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph):
        opt_g.step()
    variants = {"torch": torch_tail, "device": opt_d.step, "device_graph": graph.replay}

    def run(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / args.iters

    times = {k: [] for k in variants}
    for r in range(args.runs + 1):
        for k, fn in variants.items():
            us = run(fn)
            if r > 0:  # (run 0 warms up)
                times[k].append(us)
    # the three end in the same place up to the rounding order of torch's step
    diff = max(float((a.detach() - b.detach()).abs().max()) for a, b in zip(model_t.parameters(), model_d.parameters()))
    res = {"iters": args.iters, "runs": args.runs, "max_abs_diff_torch_vs_device": diff}
    for k, v in times.items():
        res[k + "_us"] = [round(x, 2) for x in v]
        print("%-13s per call: %s us" % (k, "  ".join("%8.2f" % x for x in v)))

    from torch.profiler import ProfilerActivity, profile

    for k, fn in (("torch", torch_tail), ("device", opt_d.step)):
        try:
            with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
                for _ in range(10):
                    fn()
                torch.cuda.synchronize()
            kernels = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
            res[k + "_launches_per_call"] = len(kernels) / 10.0
            print("%-13s %.1f device launches per call" % (k, len(kernels) / 10.0))
        except Exception as e:  # (a profiler that cannot trace here: the times above stand)
            res[k + "_launches_per_call"] = None
            print("%-13s launches not measured: %s" % (k, e))
    print(json.dumps(res))
    if diff > 1e-4:
        raise SystemExit("the two optimizers ended %.3e apart" % diff)
    if max(times["device"]) > min(times["torch"]):
        raise SystemExit("DeviceAdam.step() is not faster than torch's Adam.step() + load")


if __name__ == "__main__":
    main()
