"""Inputs shared by tests/test_ppo_host.py (CPU) and tests/test_gpu_ppo.py: tests/policy_grad_cases.py's
nets, rows, actions, weights (as advantages) and targets, plus old_logp = logp_ref + delta and
old_value = v_ref + eps, the rows kept clear of the clipped loss's own kinks, and the stock fp32
autograd of the textbook PPO loss that E is measured against.  Everything here runs on the CPU."""
from __future__ import annotations

import functools

import numpy as np

import policy_cases as pc
import policy_grad_cases as pgc

CLIP = 0.25
VALUE_CLIP = 0.25
DELTAS = (0.0, 0.0625, -0.0625, 0.5, -0.5)
EPSILONS = (0.0625, -0.0625, 1.0, -1.0)
ROWS = (1, 128, 129, 257)
LO, HI = float(np.float32(1.0) - np.float32(CLIP)), float(np.float32(1.0) + np.float32(CLIP))


def _loss(d, value_loss):
    return 0.5 * d * d if value_loss == "mse" else np.where(np.abs(d) < 1.0, 0.5 * d * d, np.abs(d) - 0.5)


@functools.lru_cache(maxsize=None)
def case(net, n):
    """The first n rows of a pool of 2 n (pgc's rows of the net) that clear every kink the clipped
    loss adds by 8 E (16 E for l2 = l1), E the pool's own cost for logp and value (pgc.cost_of).
    Returns a dict of float32 / int8 arrays: x, a, adv, t, old_logp, old_value.

    A value-clipped row's loss, l(old_value +- c - target), does not depend on the network.  In a
    case made of such rows alone (one row can be) loss_value is a constant of the inputs: the bf16
    contract costs it nothing, E = |contract - stock fp32| is then one float32 rounding of that
    constant or 0, and no float32 result, the stock one included, lies within half of it.  E is a
    yardstick only where the network enters the sum, so a case keeps at least one row that is not
    value-clipped under either value loss: where the first n clear rows have none, the last of
    them takes the small eps of its sign (0.0625 for 1), which leaves it inside the value clip
    and as clear of |u| = c as before (asserted).  This is worked out here from the contract
    alone; of the cases in use only a single row can need it (net "odd" at n = 1), and every case
    of 128 rows and more is the plain draw."""
    from wab_gym_amd.policy import reference_loss_and_grad

    m = 2 * n
    sd, x = pgc.state_dict(net), pgc.features(net, m)
    a, w, t = pgc.rows(net, m)
    ref = reference_loss_and_grad(sd, x, a, w, t)
    E = pgc.cost_of(ref, pgc.fp32_loss_and_grad(sd, x, a, w, t))
    rng = np.random.RandomState(4100 + n + 7 * pgc.net_shape(net)[0] + pgc.net_shape(net)[1])
    logp, v = ref["logp"].numpy(), ref["value"].numpy()
    old_logp = (logp + rng.choice(DELTAS, size=m)).astype(np.float32)
    eps = rng.choice(EPSILONS, size=m)
    old_value = (v + eps).astype(np.float32)
    d = logp - old_logp.astype(np.float64)
    u = v - old_value.astype(np.float64)
    c = float(np.float32(VALUE_CLIP))
    t64 = t.astype(np.float64)
    vc = old_value.astype(np.float64) + np.where(u > 0, c, -c)
    outside = ~(np.abs(u) <= c)
    El, Ev = E["logp"], E["value"]
    ok = (np.abs(d - np.log(HI)) > 8 * El) & (np.abs(d - np.log(LO)) > 8 * El) & (np.abs(np.abs(u) - c) > 8 * Ev)
    for value_loss in ("smooth_l1", "mse"):
        gap = np.abs(_loss(vc - t64, value_loss) - _loss(v - t64, value_loss))
        ok &= ~outside | (gap > 16 * Ev)
    ok &= ~outside | (np.abs(np.abs(vc - t64) - 1.0) > 8 * Ev)
    keep = np.nonzero(ok)[0]
    assert len(keep) >= n, "the pool of %d rows has %d clear of the PPO kinks, %d wanted" % (m, len(keep), n)
    vclipped = np.zeros(m, bool)  # (under either value loss)
    for value_loss in ("smooth_l1", "mse"):
        vclipped |= outside & (_loss(vc - t64, value_loss) > _loss(v - t64, value_loss))
    keep = keep[:n]
    if vclipped[keep].all():
        i = keep[-1]
        old_value[i] = np.float32(v[i] + np.sign(eps[i]) * min(np.abs(EPSILONS)))
        assert abs(abs(v[i] - float(old_value[i])) - c) > 8 * Ev and abs(v[i] - float(old_value[i])) <= c
    return {"x": np.ascontiguousarray(x[keep]), "a": a[keep].copy(), "adv": w[keep].copy(), "t": t[keep].copy(),
            "old_logp": old_logp[keep].copy(), "old_value": old_value[keep].copy(), "kept_of_pool": (len(np.nonzero(ok)[0]), m)}


def fp32_ppo_loss_and_grad(sd, feats, actions, adv, target, old_logp, clip, old_value=None, value_clip=None,
                           value_coef=1.0, entropy_coef=0.0, value_loss="smooth_l1", scale=1.0):
    """Stock torch fp32 on the CPU, weights not rounded: pc.fp32_forward, the textbook clipped
    loss, autograd.  reference_ppo_loss_and_grad's layout ("ppo": k3 and ratio sums in fp32)."""
    import torch

    p = {k: v.detach().clone().float().requires_grad_(True) for k, v in sd.items()}
    probs, v = pc.fp32_forward(p, feats)
    a = torch.as_tensor(actions).long()
    A, t, olp = torch.as_tensor(adv).float(), torch.as_tensor(target).float(), torch.as_tensor(old_logp).float()
    logp_all = torch.log(probs)
    logp = logp_all.gather(1, a[:, None])[:, 0]
    H = -(probs * logp_all).sum(dim=-1)
    d = logp - olp
    r = torch.exp(d)
    lo, hi = float(np.float32(1.0) - np.float32(clip)), float(np.float32(1.0) + np.float32(clip))
    lp = -torch.min(r * A, torch.clamp(r, lo, hi) * A).sum()

    def l(e):
        return 0.5 * e * e if value_loss == "mse" else torch.where(e.abs() < 1, 0.5 * e * e, e.abs() - 0.5)

    lv = l(v - t)
    if value_clip is not None and value_clip > 0:
        ov = torch.as_tensor(old_value).float()
        lv = torch.max(lv, l(ov + torch.clamp(v - ov, -float(value_clip), float(value_clip)) - t))
    lv, le = lv.sum(), H.sum()
    total = scale * (lp + value_coef * lv - entropy_coef * le)
    total.backward()
    dd = d.detach().double()
    return {"loss": tuple(x.detach().double() for x in (lp, lv, le, total)), "logp": logp.detach().double(),
            "value": v.detach().double(), "entropy": H.detach().double(), "ratio": r.detach().double(),
            "ppo": (None, (torch.expm1(dd) - dd).sum(), None, r.detach().double().sum()),
            "grads": {k: p[k].grad.double() for k in pgc.GRAD_NAMES}}


def cost_of(ref, f32):
    """pgc.cost_of, and E for the ratio rows, the k3 sum and the ratio sum."""
    E = pgc.cost_of(ref, f32)
    E["ratio"] = float((ref["ratio"] - f32["ratio"]).abs().max())
    E["k3_sum"] = abs(float(ref["ppo"][1]) - float(f32["ppo"][1]))
    E["ratio_sum"] = abs(float(ref["ppo"][3]) - float(f32["ppo"][3]))
    return E


@functools.lru_cache(maxsize=None)
def contract_and_cost(net, n, value_coef, entropy_coef, value_loss, value_clip_on=True):
    """(contract, E) of case(net, n): reference_ppo_loss_and_grad and max |contract - stock fp32
    autograd of the textbook formula| per output."""
    from wab_gym_amd.policy import reference_ppo_loss_and_grad

    c, sd = case(net, n), pgc.state_dict(net)
    vclip = VALUE_CLIP if value_clip_on else None
    args = (sd, c["x"], c["a"], c["adv"], c["t"], c["old_logp"], CLIP, c["old_value"], vclip, value_coef,
            entropy_coef, value_loss)
    ref = reference_ppo_loss_and_grad(*args)
    return ref, cost_of(ref, fp32_ppo_loss_and_grad(*args))
