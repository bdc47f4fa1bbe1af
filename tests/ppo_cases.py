"""Inputs shared by tests/test_ppo_host.py (CPU) and tests/test_gpu_ppo.py: tests/policy_grad_cases.py's
nets, rows, actions, weights (as advantages) and targets, plus old_logp = logp_ref + delta and
old_value = v_ref + eps, the rows kept clear of the clipped loss's own kinks, and the stock fp32
autograd of the textbook PPO loss that E is measured against; and for
tests/test_gpu_ppo_edges.py the head in numpy float32 (predict_head) and the builders that put rows
on the head's ties from float32 logp and value bits.  Everything here runs on the CPU."""
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


# ------------------------------------------------------------------ the head in float32, and rows on its ties
# (tests/test_gpu_ppo_edges.py; tests/test_ppo_host.py holds all of it to the contract on the CPU)
F32 = np.float32


def ordered(x):
    """float32 -> int64 that rises with the value (one step per unit in the last place)."""
    a = np.asarray(x, dtype=np.float32)
    i = a.reshape(-1).view(np.int32).astype(np.int64).reshape(a.shape)
    return np.where(i >= 0, i, -(i & 0x7FFFFFFF))


def move_units(x, k):
    """The float32 array x moved k units in the last place (k an int or an int array)."""
    o = ordered(x) + np.asarray(k, np.int64)
    return np.where(o >= 0, o, (-o) | 0x80000000).astype(np.uint32).view(np.float32).reshape(np.shape(x))


def units_apart(a, b):
    """How many float32 values lie between two float32 results, as a count of steps."""
    return np.abs(ordered(F32(a)) - ordered(F32(b)))


def value_loss32(dl, value_loss):
    """(l(dl), l'(dl)) in float32 as grad_value_loss forms them: 0.5f * dl * dl is two multiplies."""
    ad = np.abs(dl)
    quad = np.full(dl.shape, True) if value_loss == "mse" else ad < F32(1.0)
    dv = np.where(quad, dl, np.where(dl > F32(0.0), F32(1.0), F32(-1.0)))
    return np.where(quad, (F32(0.5) * dl) * dl, ad - F32(0.5)), dv


def predict_head(logp, value, ratio, adv, target, old_logp, old_value, clip, value_clip, value_loss):
    """The head of wab_policy_grad_ppo (include/wab.h) in numpy float32, one operation per contract
    operation, from the float32 logp, value and ratio a run returned: every decision the kernel
    makes is a float32 function of those bits and of the inputs, so this predicts it exactly, on
    the ties too.  d = clamp(fl32(logp - old_logp)) by comparisons (a NaN stays a NaN); lo, hi =
    float32(1) -+ float32(clip); clipped from the given ratio; w_eff = fl32(ratio A).  value_clip
    None or <= 0: no value clipping (old_value is not read).
    Returns the rows "d", "clipped", "lpol", "w_eff", "outside", "l1", "l2", "value_clipped", "lv",
    "dv" (l'(v - t), 0 where value_clipped; not yet times value_coef) and "k3" (float64), the counts
    "n_clipped" and "n_value_clipped", and "sums": float64 sums of lpol, lv, ratio and k3."""
    logp, value, ratio = (np.asarray(x) for x in (logp, value, ratio))
    assert logp.dtype == value.dtype == ratio.dtype == np.float32, "the head is predicted from float32 bits"
    A, t, olp = (np.ascontiguousarray(x, dtype=np.float32) for x in (adv, target, old_logp))
    with np.errstate(invalid="ignore", over="ignore"):
        d = logp - olp
        d = np.where(d < F32(-30.0), F32(-30.0), np.where(d > F32(30.0), F32(30.0), d))
        lo, hi = F32(1.0) - F32(clip), F32(1.0) + F32(clip)
        clipped = ((A > F32(0.0)) & (ratio > hi)) | ((A < F32(0.0)) & (ratio < lo))
        ra = ratio * A
        lpol = np.where(clipped, -(A * np.where(A > F32(0.0), hi, lo)), -ra)
        w_eff = np.where(clipped, F32(0.0), ra)
        l1, dv = value_loss32(value - t, value_loss)
        outside = np.zeros(len(A), bool)
        l2, vcl, lv = l1.copy(), np.zeros(len(A), bool), l1
        if value_clip is not None and float(value_clip) > 0:
            c, ov = F32(value_clip), np.ascontiguousarray(old_value, dtype=np.float32)
            u = value - ov
            outside = ~(np.abs(u) <= c)
            vc = ov + np.where(u > F32(0.0), c, -c)
            l2 = np.where(outside, value_loss32(vc - t, value_loss)[0], l1)
            vcl = outside & (l2 > l1)
            lv = np.where(vcl, l2, l1)
        dv = np.where(vcl, F32(0.0), dv)
        d64 = d.astype(np.float64)
        k3 = np.expm1(d64) - d64
    out = {"d": d, "clipped": clipped, "lpol": lpol, "w_eff": w_eff, "outside": outside, "l1": l1, "l2": l2,
           "value_clipped": vcl, "lv": lv, "dv": dv, "k3": k3, "lo": lo, "hi": hi}
    assert all(out[k].dtype == np.float32 for k in ("d", "lpol", "w_eff", "l1", "l2", "lv", "dv"))
    out["n_clipped"], out["n_value_clipped"] = int(clipped.sum()), int(vcl.sum())
    out["sums"] = {"lpol": float(lpol.astype(np.float64).sum()), "lv": float(lv.astype(np.float64).sum()),
                   "ratio": float(ratio.astype(np.float64).sum()), "k3": float(k3.sum())}
    return out


def tie_old_logp(logp, bound):
    """old_logp = fl32(logp - ln bound) moved k units, k cycling over -4 .. 4 by row: the ratios of
    these rows lie within a few units of `bound` (1.25, 0.75), several rows to a value."""
    logp = np.asarray(logp, np.float32)
    base = (logp.astype(np.float64) - np.log(bound)).astype(np.float32)
    return move_units(base, np.arange(len(logp)) % 9 - 4)


def tie_advantages(ratio):
    """Advantages for rows of the given ratios: in the order of (ratio, row) the signs cycle
    + - 0 + -, so two fifths are positive, two fifths negative, a fifth exactly 0, and any five
    rows that share a ratio hold all three; the magnitudes are dyadic, the first zero is -0.0."""
    ratio = np.asarray(ratio, np.float32)
    order = np.lexsort((np.arange(len(ratio)), ratio))
    sign = np.array([1.0, -1.0, 0.0, 1.0, -1.0], np.float32)
    adv = np.empty(len(ratio), np.float32)
    adv[order] = sign[np.arange(len(ratio)) % 5] * ((np.arange(len(ratio)) % 7 + 1) / 4.0).astype(np.float32)
    zeros = np.nonzero(adv == 0)[0]
    if len(zeros):
        adv[zeros[0]] = F32(-0.0)
    return adv


def clip_for_bound(bound, upper):
    """The float32 clip (as a Python float) with fl32(1.0f + clip) == bound (upper) or
    fl32(1.0f - clip) == bound, found within a few float32 steps of |bound - 1|."""
    bound = F32(bound)
    start = np.abs(bound - F32(1.0))
    for k in (0, 1, -1, 2, -2, 3, -3, 4, -4):
        clip = move_units(start, k)
        got = F32(1.0) + clip if upper else F32(1.0) - clip
        if got == bound and 0.0 < float(clip) < 1.0:
            return float(clip)
    raise AssertionError("no float32 clip gives the bound %r" % (bound,))


def tie_bound(ratio, adv, upper):
    """The median of the distinct ratios among the rows the bound can clip (A > 0: upper)."""
    r = np.unique(np.asarray(ratio)[(adv > 0) if upper else (adv < 0)])
    return F32(r[len(r) // 2])


def groups(x, bound):
    """(#x < bound, #x == bound, #x > bound)."""
    return int((x < bound).sum()), int((x == bound).sum()), int((x > bound).sum())


def tie_value_rows(value, target, value_clip, value_loss):
    """(old_value, target, info) with the value term's rows on its ties, from float32 `value` bits.
    old_value = fl32(value -+ c) moved -2 .. 2 units (every sixth row 3 c away), so |u| <, ==, > c
    all occur.  A row outside the clip gets for its target the float32 midpoint of value and vc
    moved some of -3 .. 3 units, two rows of three the first such move at which the float32 losses
    tie (l2 == l1), the third its own move whatever it gives.  Every fourth row (outside: of vc;
    inside: of value) has its target 1 away, moved -1, 0, 1 units: smooth_l1's kink.  info counts
    the rows per group."""
    value = np.asarray(value, np.float32)
    n, c = len(value), F32(value_clip)
    i = np.arange(n)
    sgn = np.where((i // 5) % 2 == 0, F32(1.0), F32(-1.0))
    far = i % 6 == 5
    old_value = move_units(value - sgn * np.where(far, F32(3.0) * c, c), i % 5 - 2)
    u = value - old_value
    outside = ~(np.abs(u) <= c)
    vc = old_value + np.where(u > F32(0.0), c, -c)
    t = np.asarray(target, np.float32).copy()
    mid = ((value.astype(np.float64) + vc.astype(np.float64)) / 2.0).astype(np.float32)
    kinks = 0
    for j, row in enumerate(np.nonzero(outside)[0]):
        if j % 4 == 3:
            t[row] = move_units(vc[row] + (F32(1.0) if j % 8 == 3 else F32(-1.0)), (j // 8) % 3 - 1)
            kinks += 1
            continue
        moves = [(row + m) % 7 - 3 for m in range(7 if j % 3 else 1)]
        for m in moves:
            cand = move_units(mid[row], m)
            la, lb = (value_loss32(np.array([x - cand], np.float32), value_loss)[0][0] for x in (value[row], vc[row]))
            if la == lb:
                break
        else:
            cand = move_units(mid[row], moves[0])
        t[row] = cand
    for j, row in enumerate(np.nonzero(~outside)[0]):
        if j % 4 == 3:
            t[row] = move_units(value[row] + (F32(1.0) if j % 8 == 3 else F32(-1.0)), (j // 8) % 3 - 1)
            kinks += 1
    au = np.abs(u)
    info = {"u": groups(au, c), "kink_rows": kinks}
    return old_value, t, info
