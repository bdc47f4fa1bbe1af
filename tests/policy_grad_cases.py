"""Inputs shared by tests/test_policy_grad_host.py (CPU) and tests/test_gpu_policy_grad.py: the
nets, the rows, the actions / weights / targets, and the stock fp32 autograd that E_grad is
measured against.  Everything here runs on the CPU."""
from __future__ import annotations

import functools

import numpy as np

import policy_cases as pc

EXACT_NETS = ((1, 1, 1, 1, 5), (17, 33, 33, 33, 5), (449, 128, 150, 128, 5), (449, 129, 150, 128, 6))
RANDOM_NETS = ("ref", "odd", "wide")
NETS = tuple(EXACT_NETS) + RANDOM_NETS
ROWS = (1, 127, 128, 129, 257)
GRAD_NAMES = tuple("%s.%s" % (n, p) for n in ("affine1", "affine2", "affine3", "action_head", "value_head")
                   for p in ("weight", "bias"))


def net_shape(net):
    return net if isinstance(net, tuple) else {"ref": pc.NET_REF, "odd": pc.NET_ODD, "wide": pc.NET_WIDE}[net]


@functools.lru_cache(maxsize=None)
def state_dict(net):
    return pc.exact_net(net) if isinstance(net, tuple) else pc.weights(net)


def _pool(net, n):
    if net == "ref":
        return pc.ref_features(n)
    return pc.odd_features(n, net_shape(net)[0])


def kink_margins(sd, features):
    """Per row: min over the hidden units of |distance to the nearest kink| - bound, the bound
    K * 2^-23 * (sum |terms| + |bias|) of the unit's fp32 sum (K the layer's input width: the
    worst-case error of a K-term fp32 sum, times 2), computed from the contract alone.  The kinks
    are z = 0 in every hidden layer and leaky_relu(z_3) = -4, 4."""
    import torch

    from wab_gym_amd.policy import LAYERS, reference_forward

    def bf(x):
        return torch.as_tensor(x).to(torch.float32).to(torch.bfloat16).to(torch.float64)

    hidden = []
    reference_forward(sd, features, hidden=hidden)
    x = bf(features)
    worst = torch.full((x.shape[0],), float("inf"), dtype=torch.float64)
    slope = float(np.float32(0.01))
    for i, name in enumerate(LAYERS[:3]):
        w = bf(sd[name + ".weight"])
        b = sd[name + ".bias"].to(torch.float64)
        bound = w.shape[1] * 2.0 ** -23 * (x.abs() @ w.abs().T + b.abs()[None, :])
        z = hidden[i][0]
        room = z.abs() - bound
        if i == 2:
            y = torch.where(z >= 0, z, z * slope)
            room = torch.minimum(room, torch.minimum((y - 4.0).abs(), (y + 4.0).abs()) - bound)
        worst = torch.minimum(worst, room.min(dim=1).values)
        x = hidden[i][1]
    return worst.numpy()


@functools.lru_cache(maxsize=None)
def features(net, n):
    """[n, F] rows.  Exact nets: pc.exact_features.  Random-weight nets: the first n rows of a
    pool of 2 n whose every hidden pre-activation stays clear of its kinks (kink_margins)."""
    if isinstance(net, tuple):
        return pc.exact_features(n, net[0])
    pool = np.asarray(_pool(net, 2 * n), dtype=np.float32)
    keep = np.nonzero(kink_margins(state_dict(net), pool) > 0)[0]
    assert len(keep) >= n, "the pool of %d rows has %d clear of the kinks, %d wanted" % (2 * n, len(keep), n)
    return np.ascontiguousarray(pool[keep[:n]])


@functools.lru_cache(maxsize=None)
def rows(net, n):
    """(actions int8 [n], weight float32 [n], target float32 [n]) from a fixed RandomState: weights
    of both signs, about a fifth zeros; targets dyadic with |v - target| on both sides of 1."""
    from wab_gym_amd.policy import reference_forward

    shape = net_shape(net)
    rng = np.random.RandomState(900 + n + 13 * shape[0] + shape[1])
    a = rng.randint(shape[4], size=n).astype(np.int8)
    w = (rng.randint(-12, 13, size=n) / 4.0).astype(np.float32)
    w[rng.rand(n) < 0.2] = 0.0
    _, v = reference_forward(state_dict(net), features(net, n))
    delta = rng.choice((-1.75, -0.25, 0.5, 1.5), size=n)
    t = (np.floor(v.numpy() * 4.0) / 4.0 + delta).astype(np.float32)
    return a, w, t


def fp32_loss_and_grad(sd, feats, actions, weight, target, value_coef=1.0, entropy_coef=0.0, value_loss="smooth_l1",
                       scale=1.0):
    """Stock torch fp32 on the CPU, weights not rounded: pc.fp32_forward, the same loss, autograd.
    The layout of reference_loss_and_grad's result."""
    import torch
    import torch.nn.functional as Fn

    p = {k: v.detach().clone().float().requires_grad_(True) for k, v in sd.items()}
    probs, v = pc.fp32_forward(p, feats)
    a = torch.as_tensor(actions).long()
    w = torch.as_tensor(weight).float()
    t = torch.as_tensor(target).float()
    logp_all = torch.log(probs)
    logp = logp_all.gather(1, a[:, None])[:, 0]
    H = -(probs * logp_all).sum(dim=-1)
    lp = -(w * logp).sum()
    lv = Fn.smooth_l1_loss(v, t, reduction="sum") if value_loss == "smooth_l1" else 0.5 * ((v - t) ** 2).sum()
    le = H.sum()
    total = scale * (lp + value_coef * lv - entropy_coef * le)
    total.backward()
    return {"loss": tuple(x.detach().double() for x in (lp, lv, le, total)), "logp": logp.detach().double(),
            "value": v.detach().double(), "entropy": H.detach().double(),
            "grads": {k: p[k].grad.double() for k in GRAD_NAMES}}


def contract_and_cost(net, n, value_coef=1.0, entropy_coef=0.0, value_loss="smooth_l1", scale=1.0):
    """(contract, E): reference_loss_and_grad of the case, and E = max |contract - stock fp32
    autograd| per gradient tensor, per loss part ("loss_policy", ...) and per row output."""
    return _contract_and_cost(net, n, float(value_coef), float(entropy_coef), value_loss, float(scale))


@functools.lru_cache(maxsize=None)
def _contract_and_cost(net, n, value_coef, entropy_coef, value_loss, scale):
    from wab_gym_amd.policy import reference_loss_and_grad

    sd, x = state_dict(net), features(net, n)
    a, w, t = rows(net, n)
    ref = reference_loss_and_grad(sd, x, a, w, t, value_coef, entropy_coef, value_loss, scale)
    f32 = fp32_loss_and_grad(sd, x, a, w, t, value_coef, entropy_coef, value_loss, scale)
    return ref, cost_of(ref, f32)


def cost_of(ref, f32):
    E = {k: float((ref["grads"][k] - f32["grads"][k]).abs().max()) for k in GRAD_NAMES}
    for i, k in enumerate(("loss_policy", "loss_value", "entropy", "loss")):
        E[k] = float((ref["loss"][i] - f32["loss"][i]).abs())
    for k in ("logp", "value"):
        E[k] = float((ref[k] - f32[k]).abs().max())
    E["entropy_rows"] = float((ref["entropy"] - f32["entropy"]).abs().max())
    return E
