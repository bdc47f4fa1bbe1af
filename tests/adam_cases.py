"""Inputs shared by tests/test_adam_host.py (CPU) and tests/test_gpu_adam.py: the nets, seeded
fp32 parameters and gradients in the optimizer's flat order, and the reference run over several
steps.  Everything here runs on the CPU."""
from __future__ import annotations

import functools

import numpy as np

import policy_cases as pc
from wab_gym_amd import policy

NET_TINY = (1, 1, 1, 1, 2)            # twelve parameters: one segment, most of it padding (no handle has 2 actions)
NET_TWO_LEVEL = (5000, 256, 8, 8, 5)  # 1 282 438 parameters: 1253 first-level partials, the two-level tree
NETS = {"ref": pc.NET_REF, "odd": pc.NET_ODD, "wide": pc.NET_WIDE, "tiny": NET_TINY, "two_level": NET_TWO_LEVEL}
NAMES = policy.ADAM_TENSORS


def shapes(net):
    F, h1, h2, h3, A = net
    return [(h1, F), (h1,), (h2, h1), (h2,), (h3, h2), (h3,), (A, h3), (A,), (1, h3), (1,)]


def count(net):
    return sum(int(np.prod(s)) for s in shapes(net))


@functools.lru_cache(maxsize=None)
def params(which):
    """The ten float32 parameter arrays of NETS[which], uniform in +-1/sqrt(fan_in) like a default
    Linear init."""
    net = NETS[which]
    rng = np.random.RandomState(1000 + sum(net))
    out = []
    for s in shapes(net):
        bound = 1.0 / np.sqrt(s[-1] if len(s) == 2 else max(1, out[-1].shape[1]))
        out.append(((rng.random_sample(s) * 2 - 1) * bound).astype(np.float32))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def grads(which, k=0, scale=1.0):
    """Gradients of step k: normal, of very different magnitudes from tensor to tensor, a few exact
    zeros and one denormal-squared entry (1e-30) per weight tensor."""
    net = NETS[which]
    rng = np.random.RandomState(2000 + sum(net) + 101 * k)
    out = []
    for i, s in enumerate(shapes(net)):
        g = (rng.standard_normal(s) * 10.0 ** (-(i % 4))).astype(np.float32)
        flat = g.reshape(-1)
        if flat.size >= 50:  # (never a small tensor's every element: a zero gradient tests nothing)
            flat[rng.randint(flat.size, size=flat.size // 50)] = 0.0
        if len(s) == 2:
            flat[flat.size // 2] = np.float32(1e-30)
        out.append((g * np.float32(scale)).astype(np.float32))
    return tuple(out)


def zeros(which):
    return [np.zeros(s, np.float32) for s in shapes(NETS[which])]


def reference_run(which, steps, start=None, grad_scale=1.0, **hyper):
    """`steps` reference_adam_step calls on grads(which, 0), grads(which, 1), ...: the list of
    (params, exp_avg, exp_avg_sq, state) after each.  start: such a tuple to continue from."""
    cur = (list(params(which)), zeros(which), zeros(which), policy.adam_fresh_state()) if start is None else start
    out = []
    for _ in range(steps):
        k = int(cur[3]["step"]) + int(cur[3]["skipped"])
        cur = policy.reference_adam_step(cur[0], grads(which, k, grad_scale), cur[1], cur[2], cur[3], **hyper)
        out.append(cur)
    return out


@functools.lru_cache(maxsize=None)
def reference_five(which):
    """Five default-hyperparameter steps (shared by the tests that need them; not to be modified)."""
    return tuple(reference_run(which, 5))


def make_model(which, order=("affine1", "affine2", "affine3", "action_head", "value_head")):
    """A torch module with the five Linears of NETS[which], registered in `order`, holding
    params(which)."""
    import torch

    F, h1, h2, h3, A = NETS[which]
    dims = {"affine1": (F, h1), "affine2": (h1, h2), "affine3": (h2, h3), "action_head": (h3, A), "value_head": (h3, 1)}
    model = torch.nn.Module()
    for name in order:
        model.add_module(name, torch.nn.Linear(*dims[name]))
    by_name = dict(model.named_parameters())
    with torch.no_grad():
        for name, p in zip(NAMES, params(which)):
            by_name[name].copy_(torch.from_numpy(p))
    return model
