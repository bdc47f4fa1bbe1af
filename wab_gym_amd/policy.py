"""DevicePolicy — actor_critic.py's Policy (actor_critic.py:54-97) for inference on device, the
action sampled in the same launch (wab_policy_act, wab_gym_amd/csrc/wab_policy.hip).

    policy = DevicePolicy(model, env)            # model: the five Linears by the reference's names
    actions = policy.act(features)               # int8 [B]; probs=/value= tensors are filled too
    ...optimizer.step()...; policy.load(model)   # stream-ordered re-pack, no host sync
    policy.loss_and_grad(features, actions, weight, target, into=model)   # finish_episode's loss
                                                 # and loss.backward() (wab_policy_grad)
    old = policy.evaluate(features, actions)["logp"]                      # (wab_policy_evaluate)
    policy.ppo_loss_and_grad(features, actions, advantage, target, old, clip=0.2, into=model)
                                                 # PPO's clipped loss (wab_policy_grad_ppo)
    policy.ppo_loss_and_grad(..., rows=perm[a:b])  # the minibatch's rows picked from the whole segment
                                                 # by an int32 index, no copy (wab_policy_grad_ppo_gather)

    opt = DeviceAdam(policy, model, lr=3e-4)     # optimizer.step() and the re-pack in HIP
    opt.step()                                   # (wab_policy_adam_step): no policy.load after it

loss_and_grad fills each parameter's .grad; the caller steps with DeviceAdam, or with a torch
optimizer and reloads.

What the kernels compute is `reference_forward`, `reference_loss_and_grad` (the numeric
contracts, in torch on the CPU), `reference_adam_step` (in numpy) and `sample_reference` (the
sampling rule, in numpy) below; the tests check the kernels against them.
The reference's `+ U(0, 1) / 100` input noise (actor_critic.py:189) is not reproduced.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib

LAYERS = ("affine1", "affine2", "affine3", "action_head", "value_head")
SITE_POLICY = 11  # keyed-RNG site of the action draw (the first id free in oracle/keyed_rng.py)


def _state_dict(module_or_state_dict):
    sd = module_or_state_dict
    if hasattr(sd, "state_dict"):
        sd = sd.state_dict()
    out = {}
    for name in LAYERS:
        for part in ("weight", "bias"):
            key = "%s.%s" % (name, part)
            if key not in sd:
                raise ValueError("the policy needs %s (the five Linears of actor_critic.Policy: %s)"
                                 % (key, ", ".join(LAYERS)))
            out[key] = sd[key]
    return out


def shape_of(state_dict):
    """(in_features, h1, h2, h3, n_actions) of a state dict, its layers checked against each other."""
    sd = _state_dict(state_dict)
    w = [sd[n + ".weight"] for n in LAYERS]
    if any(x.dim() != 2 for x in w):
        raise ValueError("Linear weights must be 2-D [out, in]")
    h1, F = w[0].shape
    h2, h3, A = w[1].shape[0], w[2].shape[0], w[3].shape[0]
    want = {"affine2": (h2, h1), "affine3": (h3, h2), "action_head": (A, h3), "value_head": (1, h3)}
    for name, shp in want.items():
        if tuple(sd[name + ".weight"].shape) != shp:
            raise ValueError("%s.weight has shape %s, expected %s" % (name, tuple(sd[name + ".weight"].shape), shp))
    for name, n in zip(LAYERS, (h1, h2, h3, A, 1)):
        if tuple(sd[name + ".bias"].shape) != (n,):
            raise ValueError("%s.bias has shape %s, expected (%d,)" % (name, tuple(sd[name + ".bias"].shape), n))
    return int(F), int(h1), int(h2), int(h3), int(A)


def reference_forward(state_dict, features, hidden=None):
    """The kernel's numeric contract in torch on the CPU: every matmul operand (features, weights,
    hidden activations after bias, leaky_relu and clamp) rounded to bf16 (nearest even), everything
    else in float64 (the kernel: fp32 MFMA accumulation, fp32 bias / leaky_relu(0.01) / clamp(-4, 4)
    / max-subtracted softmax / value).  Returns (probs [B, A], value [B]) as float64 tensors.
    `hidden`, a list, receives each hidden layer's (pre-activation, bf16 output) pair."""
    import torch

    sd = {k: v.detach().to("cpu", torch.float32) for k, v in _state_dict(state_dict).items()}

    def bf(x):  # round to bf16, carried on in float64
        return x.to(torch.float32).to(torch.bfloat16).to(torch.float64)

    def linear(x, name):
        return x @ bf(sd[name + ".weight"]).T + sd[name + ".bias"].to(torch.float64)

    x = bf(torch.as_tensor(features).detach().to("cpu", torch.float32))
    for i, name in enumerate(LAYERS[:3]):
        z = linear(x, name)
        x = torch.where(z >= 0, z, z * float(np.float32(0.01)))
        if i == 2:
            x = x.clamp(-4.0, 4.0)
        x = bf(x)
        if hidden is not None:
            hidden.append((z, x))
    logits = linear(x, "action_head")
    e = torch.exp(logits - logits.max(dim=-1, keepdim=True).values)
    return e / e.sum(dim=-1, keepdim=True), linear(x, "value_head")[:, 0]


def _value_loss(d, value_loss):
    """(l(d), l'(d)) of the configured value loss, float64 tensors."""
    import torch

    if value_loss == "mse":
        return 0.5 * d * d, d
    return (torch.where(d.abs() < 1.0, 0.5 * d * d, d.abs() - 0.5), torch.where(d.abs() < 1.0, d, torch.sign(d)))


def _reference_head_and_backward(state_dict, features, actions, head, entropy_coef, scale, round_grads):
    """What reference_loss_and_grad and reference_ppo_loss_and_grad share: the forward, p, log p,
    H, then head(logp, v, ok) -> (w rows, g_v rows, loss_policy, loss_value, extras), then G_4 and
    the straight-through backward.  ok: the rows whose action is inside [0, A); the others are left
    out of every sum and gradient and have logp 0 (the kernels' bad-action rule).  Returns (loss
    parts, logp, v, H, grads, extras)."""
    import torch

    sd = {k: v.detach().to("cpu", torch.float32) for k, v in _state_dict(state_dict).items()}

    def bf(x):
        return x.to(torch.float32).to(torch.bfloat16).to(torch.float64)

    def rd(g):
        return bf(g) if round_grads else g

    x0 = bf(torch.as_tensor(features).detach().to("cpu", torch.float32))
    a = torch.as_tensor(actions).detach().to("cpu", torch.int64)
    hidden = []
    _, v = reference_forward(sd, features, hidden=hidden)
    xs = [x0] + [h[1] for h in hidden]
    wq = {n: bf(sd[n + ".weight"]) for n in LAYERS}
    logits = xs[3] @ wq["action_head"].T + sd["action_head.bias"].to(torch.float64)
    zc = logits - logits.max(dim=-1, keepdim=True).values
    logp_all = zc - torch.log(torch.exp(zc).sum(dim=-1, keepdim=True))
    p = torch.exp(logp_all)
    H = -(p * logp_all).sum(dim=-1)
    ok = (a >= 0) & (a < p.shape[1])
    onehot = torch.zeros_like(p)
    onehot[torch.arange(len(a)), torch.where(ok, a, torch.zeros_like(a))] = 1.0
    zero = torch.zeros_like(H)
    logp = torch.where(ok, (logp_all * onehot).sum(dim=-1), zero)
    w, gv, loss_policy, loss_value, extras = head(logp, v, ok)
    loss_entropy = torch.where(ok, H, zero).sum()

    Da = rd(w[:, None] * (p - onehot) + entropy_coef * p * (logp_all + H[:, None]))
    Da = torch.where(ok[:, None], Da, torch.zeros_like(Da))
    Dv = rd(torch.where(ok, gv, zero))[:, None]
    grads = {"action_head.weight": Da.T @ xs[3], "action_head.bias": Da.sum(dim=0),
             "value_head.weight": Dv.T @ xs[3], "value_head.bias": Dv.sum(dim=0)}
    dx = Da @ wq["action_head"] + Dv @ wq["value_head"]
    slope = float(np.float32(0.01))
    for i in (2, 1, 0):
        z = hidden[i][0]
        G = dx * torch.where(z >= 0, 1.0, slope)
        if i == 2:
            y = torch.where(z >= 0, z, z * slope)
            G = G * ((y >= -4.0) & (y <= 4.0)).to(torch.float64)
        D = rd(G)
        grads[LAYERS[i] + ".weight"] = D.T @ xs[i]
        grads[LAYERS[i] + ".bias"] = D.sum(dim=0)
        dx = D @ wq[LAYERS[i]]
    grads = {k: g * scale for k, g in grads.items()}
    return (loss_policy, loss_value, loss_entropy), logp, v, H, grads, extras


def _reference_gather(features, rows, actions, **per_row):
    """The host side of `rows=`: (features, actions, per-row arrays) of call rows 0 .. N - 1, row i
    from source row rows[i] of features [M, F] or [T, B, F] (M = T B).  An index outside [0, M) is
    clamped into it and its row given action -1: the bad-row rule is the bad-action rule."""
    import torch

    r = torch.as_tensor(rows).detach().to("cpu", torch.int64).reshape(-1)
    x = torch.as_tensor(features).detach().to("cpu")
    x = x.reshape(-1, x.shape[-1])
    M = x.shape[0]
    if M < 1:
        raise ValueError("rows= needs a source of at least one row")
    bad = (r < 0) | (r >= M)
    rc = r.clamp(0, M - 1)
    a = torch.as_tensor(actions).detach().to("cpu", torch.int64).reshape(-1)[rc]
    a = torch.where(bad, torch.full_like(a, -1), a)
    out = {k: None if v is None else torch.as_tensor(v).detach().to("cpu").reshape(-1)[rc] for k, v in per_row.items()}
    return x[rc], a, out


def reference_loss_and_grad(state_dict, features, actions, weight, target, value_coef=1.0, entropy_coef=0.0,
                            value_loss="smooth_l1", scale=1.0, round_grads=True, rows=None):
    """wab_policy_grad's numeric contract in torch on the CPU, float64, written out by hand (no
    autograd).  The forward is reference_forward.  Per row, p = softmax(logits), H = -sum p log p:

        loss_policy = -sum_i weight_i log p_i[a_i];  loss_value = sum_i l(v_i - target_i), l
        smooth_l1 (beta 1) or "mse" = d^2 / 2;  loss_entropy = sum_i H_i;
        total = scale (loss_policy + value_coef loss_value - entropy_coef loss_entropy)

    and the gradients of `total`, straight-through: every bf16 rounding has derivative 1.  With
    G_4 = [weight (p - onehot) + entropy_coef p (log p + H) | value_coef l'] and D_l = bf16(G_l)
    (G_l itself without round_grads): dW_l = D_l^T x_{l-1}, db_l = sum_i D_l[i], dx_{l-1} = D_l
    bf16(W_l), G_{l-1} = dx_{l-1} * (z >= 0 ? 1 : float32(0.01)) * (layer 3: -4 <= leaky_relu(z) <= 4).
    Returns {"loss": (policy, value, entropy, total), "logp", "value", "entropy": [N] rows,
    "grads": the ten tensors in torch Linear layout}, all float64.
    A row whose action is outside [0, A) takes no part in any sum or gradient and has logp 0.
    rows (int [N]): the call's row i is source row rows[i] of features and of every per-row array
    (wab_policy_grad_gather); an index outside the source is clamped into it and its row treated
    as a bad-action row."""
    import torch

    if value_loss not in ("smooth_l1", "mse"):
        raise ValueError("value_loss must be 'smooth_l1' or 'mse'")
    if rows is not None:
        features, actions, g = _reference_gather(features, rows, actions, weight=weight, target=target)
        weight, target = g["weight"], g["target"]
    w = torch.as_tensor(weight).detach().to("cpu", torch.float64)
    tg = torch.as_tensor(target).detach().to("cpu", torch.float64)

    def head(logp, v, ok):
        lv, dv = _value_loss(v - tg, value_loss)
        zero = torch.zeros_like(v)
        return w, value_coef * dv, torch.where(ok, -(w * logp), zero).sum(), torch.where(ok, lv, zero).sum(), None

    (lp, lvs, le), logp, v, H, grads, _ = _reference_head_and_backward(state_dict, features, actions, head,
                                                                       entropy_coef, scale, round_grads)
    total = scale * (lp + value_coef * lvs - entropy_coef * le)
    return {"loss": (lp, lvs, le, total), "logp": logp, "value": v, "entropy": H, "grads": grads}


def reference_ppo_loss_and_grad(state_dict, features, actions, advantage, target, old_logp, clip=0.2, old_value=None,
                                value_clip=None, value_coef=1.0, entropy_coef=0.0, value_loss="smooth_l1", scale=1.0,
                                round_grads=True, rows=None):
    """wab_policy_grad_ppo's numeric contract (include/wab.h) in torch on the CPU, float64, by
    hand: reference_loss_and_grad with the clipped surrogate's effective weight and the clipped
    value loss.  Per row, A the advantage, lo = float32(1) - float32(clip), hi = float32(1) +
    float32(clip) (the two float32 values the kernel forms):

        d = clamp(logp - old_logp, -30, 30);  r = exp(d)
        clipped = (A > 0 and r > hi) or (A < 0 and r < lo)
        loss_policy_i = -(A (hi if A > 0 else lo)) if clipped else -(r A);  w_eff = 0 if clipped else r A
        u = v - old_value;  |u| <= value_clip: the plain value loss and gradient;  otherwise
        vc = old_value + sign(u) value_clip, loss_value_i = max(l(v - t), l(vc - t)), and g_v = 0
        where l(vc - t) > l(v - t) (value_clipped)

    value_clip None or <= 0: no value clipping.  Returns reference_loss_and_grad's dict plus
    "ratio", "clipped", "value_clipped" rows and "ppo" = (clipped rows, sum of k3 = expm1(d) - d,
    value-clipped rows, sum of r).  Bad-action rows and `rows` as reference_loss_and_grad's (a row
    left out has ratio 0 and counts in none of the four)."""
    import torch

    if value_loss not in ("smooth_l1", "mse"):
        raise ValueError("value_loss must be 'smooth_l1' or 'mse'")
    if rows is not None:
        features, actions, g = _reference_gather(features, rows, actions, advantage=advantage, target=target,
                                                 old_logp=old_logp, old_value=old_value)
        advantage, target, old_logp, old_value = g["advantage"], g["target"], g["old_logp"], g["old_value"]
    A = torch.as_tensor(advantage).detach().to("cpu", torch.float64)
    tg = torch.as_tensor(target).detach().to("cpu", torch.float64)
    olp = torch.as_tensor(old_logp).detach().to("cpu", torch.float64)
    one, cl = np.float32(1.0), np.float32(clip)
    lo, hi = float(one - cl), float(one + cl)
    vclip_on = value_clip is not None and float(value_clip) > 0
    if vclip_on and old_value is None:
        raise ValueError("value_clip > 0 needs old_value")
    c = float(np.float32(value_clip)) if vclip_on else 0.0

    def head(logp, v, ok):
        zero = torch.zeros_like(v)
        d = (logp - olp).clamp(-30.0, 30.0)
        r = torch.where(ok, torch.exp(d), zero)
        clipped = ok & (((A > 0) & (r > hi)) | ((A < 0) & (r < lo)))
        bound = torch.where(A > 0, hi, lo)
        lpol = torch.where(clipped, -(A * bound), -(r * A))
        w_eff = torch.where(clipped, torch.zeros_like(A), r * A)
        l1, dv = _value_loss(v - tg, value_loss)
        lv, vcl = l1, torch.zeros_like(clipped)
        if vclip_on:
            ov = torch.as_tensor(old_value).detach().to("cpu", torch.float64)
            u = v - ov
            vc = ov + torch.where(u > 0, c, -c)
            l2, _ = _value_loss(vc - tg, value_loss)
            outside = ~(u.abs() <= c)
            vcl = ok & outside & (l2 > l1)
            lv = torch.where(vcl, l2, l1)
        gv = torch.where(vcl, torch.zeros_like(dv), value_coef * dv)
        ppo = (clipped.to(torch.float64).sum(), torch.where(ok, torch.expm1(d) - d, zero).sum(),
               vcl.to(torch.float64).sum(), r.sum())
        return (w_eff, gv, torch.where(ok, lpol, zero).sum(), torch.where(ok, lv, zero).sum(),
                {"ratio": r, "clipped": clipped, "value_clipped": vcl, "ppo": ppo})

    (lp, lvs, le), logp, v, H, grads, extra = _reference_head_and_backward(state_dict, features, actions, head,
                                                                           entropy_coef, scale, round_grads)
    total = scale * (lp + value_coef * lvs - entropy_coef * le)
    out = {"loss": (lp, lvs, le, total), "logp": logp, "value": v, "entropy": H, "grads": grads}
    out.update(extra)
    return out


def check_rows(shape, features, **rows):
    """features [N, F] or [T, B, F] float32 and the named per-row tensors (actions int8, every other
    float32) of the leading shape, all contiguous and on the features' device: returns N."""
    import torch

    F = shape[0]
    if not isinstance(features, torch.Tensor) or features.dtype != torch.float32 or features.dim() not in (2, 3) \
            or features.shape[-1] != F or not features.is_contiguous():
        raise ValueError("features must be a contiguous float32 tensor of shape [N, %d] or [T, B, %d]" % (F, F))
    lead = tuple(features.shape[:-1])
    for name, x in rows.items():
        dt = torch.int8 if name == "actions" else torch.float32
        if not isinstance(x, torch.Tensor) or x.dtype != dt or tuple(x.shape) != lead or not x.is_contiguous() \
                or x.device != features.device:
            raise ValueError("%s must be a contiguous %s tensor of shape %s on %s"
                             % (name, str(dt).replace("torch.", ""), lead, features.device))
    n = 1
    for k in lead:
        n *= int(k)
    if n >= 1 << 31:
        raise ValueError("loss_and_grad takes fewer than 2^31 rows")
    return n


def check_row_index(rows, device):
    """The checks of a `rows=` index that need no device: a 1-d contiguous int32 or int64 tensor
    (a slice such as perm[a:b] is one) on `device`, fewer than 2^31 entries.  Returns N, its
    length.  The values are checked on the device, by the kernels."""
    import torch

    if not isinstance(rows, torch.Tensor):
        raise ValueError("rows must be a torch tensor of int32 (or int64) source rows")
    if rows.dtype not in (torch.int32, torch.int64):
        raise ValueError("rows must be int32 (or int64, converted), not %s" % str(rows.dtype).replace("torch.", ""))
    if rows.dim() != 1:
        raise ValueError("rows must be 1-d [N], not of shape %s" % (tuple(rows.shape),))
    if not rows.is_contiguous():
        raise ValueError("rows must be contiguous (stride %s): take a slice of a contiguous index" % (rows.stride(),))
    if rows.device != torch.device(device):
        raise ValueError("rows must be on the features' device %s, not %s" % (device, rows.device))
    if rows.numel() >= 1 << 31:
        raise ValueError("rows must have fewer than 2^31 entries")
    return int(rows.numel())


def check_loss_args(shape, features, actions, weight, target, value_loss="smooth_l1", reduction="sum", into=None,
                    accumulate=False):
    """loss_and_grad's checks that need no device: returns N, the row count.  features [N, F] or
    [T, B, F] float32, actions int8, weight and target float32 of the leading shape, all
    contiguous and on one device."""
    n = check_rows(shape, features, actions=actions, weight=weight, target=target)
    if value_loss not in _lib.VALUE_LOSS:
        raise ValueError("value_loss must be 'smooth_l1' or 'mse', not %r" % (value_loss,))
    if reduction not in ("sum", "mean"):
        raise ValueError("reduction must be 'sum' or 'mean', not %r" % (reduction,))
    if accumulate and into is None:
        raise ValueError("accumulate=True needs into=: there is no earlier gradient to add to")
    return n


def check_ppo_args(shape, features, actions, advantage, target, old_logp, clip=0.2, old_value=None, value_clip=None,
                   value_loss="smooth_l1", reduction="sum", into=None, accumulate=False):
    """ppo_loss_and_grad's checks that need no device: check_loss_args', and old_logp (old_value
    where value_clip > 0) float32 of the leading shape, contiguous, on the features' device; clip
    inside (0, 1); value_clip None, or a number (<= 0: off).  Returns N."""
    n = check_loss_args(shape, features, actions, advantage, target, value_loss, reduction, into, accumulate)
    if not 0.0 < float(clip) < 1.0:
        raise ValueError("clip must be inside (0, 1), not %r" % (clip,))
    if value_clip is not None and float(value_clip) != float(value_clip):
        raise ValueError("value_clip is NaN")
    on = value_clip is not None and float(value_clip) > 0
    if on and old_value is None:
        raise ValueError("value_clip > 0 needs old_value")
    check_rows(shape, features, old_logp=old_logp, **({"old_value": old_value} if on else {}))
    return n


ADAM_TENSORS = tuple("%s.%s" % (n, part) for n in LAYERS for part in ("weight", "bias"))  # the flat order


def pair_tree_sum(q):
    """The adjacent-pair tree sum of a 1-D float64 array, zero-padded to the next power of two:
    x = x[0::2] + x[1::2] until one value is left (the order wab_policy_adam_step's norm is
    summed in)."""
    q = np.asarray(q, np.float64).ravel()
    n = 1
    while n < q.size:
        n *= 2
    x = np.zeros(n, np.float64)
    x[:q.size] = q
    with np.errstate(all="ignore"):
        while x.size > 1:
            x = x[0::2] + x[1::2]
    return x[0]


def check_adam_args(lr, betas, eps, weight_decay, max_grad_norm):
    """The argument checks of wab_policy_adam_step, on the host (ValueError)."""
    if not float(lr) >= 0.0:
        raise ValueError("lr must be >= 0, not %r" % (lr,))
    if len(betas) != 2 or not all(0.0 <= float(b) < 1.0 for b in betas):
        raise ValueError("betas must be two numbers in [0, 1), not %r" % (betas,))
    if not float(eps) > 0.0:
        raise ValueError("eps must be > 0, not %r" % (eps,))
    if not float(weight_decay) >= 0.0:
        raise ValueError("weight_decay must be >= 0, not %r" % (weight_decay,))
    if float(max_grad_norm) != float(max_grad_norm):
        raise ValueError("max_grad_norm is NaN")


def adam_beta_powers(step, betas):
    """beta1^step and beta2^step as the optimizer state keeps them: `step` sequential double
    multiplications each (0.0 for step 0, where they are not read)."""
    out = []
    for b in betas:
        p = 0.0
        for i in range(int(step)):
            p = (1.0 if i == 0 else p) * float(b)
        out.append(p)
    return tuple(out)


def adam_fresh_state():
    """wab_adam_state of a fresh optimizer (all-zero bytes), as a dict."""
    return {"step": 0, "skipped": 0, "beta1_pow": 0.0, "beta2_pow": 0.0, "grad_norm": np.float32(0.0),
            "clip_scale": np.float32(0.0)}


def reference_adam_step(params, grads, exp_avg, exp_avg_sq, state, lr=1e-3, betas=(0.9, 0.999), eps=1e-8,
                        weight_decay=0.0, decoupled=False, max_grad_norm=0.0):
    """wab_policy_adam_step's numeric contract (include/wab.h) in numpy: float32 arrays and
    scalars, float64 where the contract says so, the norm's sum by pair_tree_sum.  params, grads,
    exp_avg, exp_avg_sq: the ten arrays each in ADAM_TENSORS order; state: a dict as
    adam_fresh_state().  Nothing is modified; returns (params, exp_avg, exp_avg_sq, state), new."""
    check_adam_args(lr, betas, eps, weight_decay, max_grad_norm)
    f32 = np.float32

    def arrays(xs, what):
        xs = [np.array(x.detach().cpu().numpy() if hasattr(x, "detach") else x, copy=True) for x in xs]
        if len(xs) != len(ADAM_TENSORS) or any(x.dtype != np.float32 for x in xs):
            raise ValueError("%s must be ten float32 arrays" % what)
        return xs

    p, g, m, v = (arrays(x, n) for x, n in ((params, "params"), (grads, "grads"), (exp_avg, "exp_avg"),
                                            (exp_avg_sq, "exp_avg_sq")))
    st = dict(state)
    with np.errstate(all="ignore"):
        flat = np.concatenate([x.ravel() for x in g]).astype(np.float64)
        S = pair_tree_sum(flat * flat)
        norm = np.sqrt(np.float64(S))
        st["grad_norm"] = f32(norm)
        c = f32(1.0)
        if max_grad_norm > 0:
            r = np.float64(max_grad_norm) / (norm + np.float64(1e-6))
            c = f32(r if r < 1.0 else 1.0)
        st["clip_scale"] = c
        if not np.isfinite(S):
            st["skipped"] = int(st["skipped"]) + 1
            return p, m, v, st
        beta1, beta2 = float(betas[0]), float(betas[1])
        b1p = (1.0 if st["step"] == 0 else float(st["beta1_pow"])) * beta1
        b2p = (1.0 if st["step"] == 0 else float(st["beta2_pow"])) * beta2
        a = f32(float(lr) / (1.0 - b1p))
        r2 = np.sqrt(f32(1.0 - b2p))
        b1f, omb1, b2f, omb2 = f32(beta1), f32(1.0 - beta1), f32(beta2), f32(1.0 - beta2)
        epsf, wdf, decayf = f32(eps), f32(weight_decay), f32(1.0 - float(lr) * float(weight_decay))
        st["step"] = int(st["step"]) + 1
        st["beta1_pow"], st["beta2_pow"] = b1p, b2p
        for i in range(len(p)):
            gi = g[i] * c
            if weight_decay != 0 and not decoupled:
                gi = gi + wdf * p[i]
            if weight_decay != 0 and decoupled:
                p[i] = p[i] * decayf
            m[i] = b1f * m[i] + omb1 * gi
            v[i] = b2f * v[i] + (omb2 * gi) * gi
            den = np.sqrt(v[i]) / r2 + epsf
            p[i] = p[i] - a * (m[i] / den)
            assert p[i].dtype == np.float32 and m[i].dtype == np.float32 and v[i].dtype == np.float32
    return p, m, v, st


def adam_state_dict(step, exp_avg, exp_avg_sq, order, lr, betas, eps, weight_decay, decoupled, max_grad_norm):
    """An optimizer state in torch.optim.Adam's state_dict() layout: state[order[k]] = {"step",
    "exp_avg", "exp_avg_sq"} for tensor k of ADAM_TENSORS (order[k]: its index in
    model.parameters()), one param group with Adam's keys (AdamW's with `decoupled`) plus
    "max_grad_norm".  A fresh optimizer (step 0) has an empty state, as torch's."""
    import torch

    kind = torch.optim.AdamW if decoupled else torch.optim.Adam
    group = dict(kind([torch.zeros(1)]).defaults)  # every key this torch's step() reads
    group.update(lr=float(lr), betas=(float(betas[0]), float(betas[1])), eps=float(eps),
                 weight_decay=float(weight_decay), max_grad_norm=float(max_grad_norm),
                 params=list(range(len(order))))
    state = {}
    if int(step) > 0:
        for k, i in enumerate(order):
            state[int(i)] = {"step": torch.tensor(float(step), dtype=torch.float32),
                             "exp_avg": exp_avg[k].detach().clone(), "exp_avg_sq": exp_avg_sq[k].detach().clone()}
    return {"state": state, "param_groups": [group]}


def parse_adam_state_dict(sd, order, shapes):
    """What DeviceAdam.load_state_dict takes from a state_dict() of torch.optim.Adam / AdamW or of
    DeviceAdam over the same model: (step, exp_avg, exp_avg_sq, hyper), the moments in
    ADAM_TENSORS order (None for an empty state), hyper a dict of lr, betas, eps, weight_decay,
    decoupled and, where the dict has it, max_grad_norm.  ValueError for another layout: more than
    one param group, amsgrad or maximize, a state that covers some tensors only, steps that differ
    between tensors, or moments of another shape."""
    if not isinstance(sd, dict) or "state" not in sd or "param_groups" not in sd:
        raise ValueError("not an optimizer state_dict (state, param_groups)")
    if len(sd["param_groups"]) != 1:
        raise ValueError("DeviceAdam takes one param group, the state_dict has %d" % len(sd["param_groups"]))
    group = sd["param_groups"][0]
    if sorted(group["params"]) != sorted(int(i) for i in order):
        raise ValueError("the state_dict's param group does not hold the model's ten parameters")
    if group.get("amsgrad") or group.get("maximize"):
        raise ValueError("amsgrad and maximize are not supported")
    hyper = {"lr": float(group["lr"]), "betas": (float(group["betas"][0]), float(group["betas"][1])),
             "eps": float(group["eps"]), "weight_decay": float(group["weight_decay"]),
             "decoupled": bool(group.get("decoupled_weight_decay", False))}
    if "max_grad_norm" in group:
        hyper["max_grad_norm"] = float(group["max_grad_norm"])
    check_adam_args(hyper["lr"], hyper["betas"], hyper["eps"], hyper["weight_decay"], hyper.get("max_grad_norm", 0.0))
    state = sd["state"]
    if len(state) == 0:
        return 0, None, None, hyper
    if sorted(state.keys()) != sorted(int(i) for i in order):
        raise ValueError("the state_dict's state covers parameters %s, the model's are %s"
                         % (sorted(state.keys()), sorted(order)))
    steps = {float(state[int(i)]["step"]) for i in order}
    if len(steps) != 1:
        raise ValueError("the parameters' step counts differ: %s" % sorted(steps))
    step = steps.pop()
    if step != int(step) or step < 0:
        raise ValueError("step must be a non-negative integer, not %r" % step)
    m, v = [], []
    for k, i in enumerate(order):
        for key, dst in (("exp_avg", m), ("exp_avg_sq", v)):
            x = state[int(i)][key]
            if tuple(x.shape) != tuple(shapes[k]):
                raise ValueError("%s of %s has shape %s, expected %s" % (key, ADAM_TENSORS[k], tuple(x.shape),
                                                                        tuple(shapes[k])))
            dst.append(x)
    return int(step), m, v, hyper


def keyed_u(seed, env_ids, episode, turn):
    """The 53-bit keyed uniform of the action draw: (seed, global env id, episode, site 11, turn,
    tile (0, 0), k = 0) under the definition of oracle/keyed_rng.py, restated here so that the
    product does not import test infrastructure."""
    M64 = (1 << 64) - 1

    def mix64(z):
        z &= M64
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
        return z ^ (z >> 31)

    def fmix32(h):
        h ^= h >> 16
        h = (h * 0x85EBCA6B) & 0xFFFFFFFF
        h ^= h >> 13
        h = (h * 0xC2B2AE35) & 0xFFFFFFFF
        return h ^ (h >> 16)

    a = mix64((int(seed) + 0x9E3779B97F4A7C15) & M64)
    out = np.zeros(len(env_ids), np.float64)
    for i, (env, ep, t) in enumerate(zip(env_ids, episode, turn)):
        ek = mix64(mix64(a ^ (int(env) & M64)) ^ (int(ep) & M64))
        b0, b1 = ek & 0xFFFFFFFF, ek >> 32
        ts = SITE_POLICY | ((int(t) & 0xFFFFF) << 12)
        h1 = fmix32(b0)  # tile (0, 0)
        hi = fmix32(h1 ^ ts ^ b1)
        lo = fmix32(h1 ^ (((ts << 16) | (ts >> 16)) & 0xFFFFFFFF) ^ b0 ^ 0x9E3779B9)
        out[i] = float((hi << 21) | (lo >> 11)) * 2.0 ** -53
    return out


def sample_reference(probs_f32, seed, env_ids, episode, turn):
    """The sampling rule in numpy: action = #{k < A - 1 : c_k <= u}, c_k the running sum in double,
    k = 0, 1, ..., of the float32 probabilities, u = keyed_u(...).  int8 [B]."""
    p = np.asarray(probs_f32)
    if p.dtype != np.float32:
        raise ValueError("probs must be float32: the rule is defined on the values the kernel writes")
    c = np.cumsum(p.astype(np.float64), axis=1)  # sequential, in order k = 0, 1, ...
    u = keyed_u(seed, np.asarray(env_ids), np.asarray(episode), np.asarray(turn))
    return (c[:, :-1] <= u[:, None]).sum(axis=1).astype(np.int8)


class DevicePolicy:
    """The policy network on the env's device.  `module_or_state_dict` holds the five Linears by
    the reference's names (affine1, affine2, affine3, action_head, value_head); `env` is the
    BatchedWolvesAndBushesEnv (or a wrapper of it) whose envs it acts for: its episode and turn
    counters key the draw."""

    def __init__(self, module_or_state_dict, env):
        import torch

        self._torch = torch
        base = env
        while not hasattr(base, "_h") and hasattr(base, "env"):
            base = base.env
        self.env = base
        self.shape = shape_of(module_or_state_dict)
        F, h1, h2, h3, A = self.shape
        if A != base.n_actions:
            raise ValueError("the policy has %d actions, the env's options %d" % (A, base.n_actions))
        self.in_features, self.n_actions = F, A
        L = _lib.load()
        shp = _lib.WabPolicyShape(F, h1, h2, h3, A)
        p = ctypes.c_void_p()
        _lib.check(L.wab_policy_create(ctypes.addressof(shp), base.device.index, ctypes.byref(p)),
                   "wab_policy_create")
        self._p = p
        self._keep = None
        self._grad_ws = None  # loss_and_grad's workspace, allocated by its first call
        B = base.num_envs
        self.actions = torch.zeros(B, dtype=torch.int8, device=base.device)
        self.load(module_or_state_dict)

    def load(self, module_or_state_dict):
        """Re-pack the weights (bf16, padded) from the module's current parameters: one launch on
        the env's stream, no host synchronisation.  Parameters already float32, contiguous and on
        the env's device are read in place."""
        t = self._torch
        if shape_of(module_or_state_dict) != self.shape:
            raise ValueError("load(): the layers' shapes differ from the policy's %s" % (self.shape,))
        sd = _state_dict(module_or_state_dict)
        keep = [sd["%s.%s" % (n, part)].detach().to(self.env.device, t.float32).contiguous()
                for n in LAYERS for part in ("weight", "bias")]
        w = _lib.WabPolicyWeights(*[x.data_ptr() for x in keep])
        _lib.check(_lib.load().wab_policy_load(self._p, ctypes.addressof(w), self.env._stream()),
                   "wab_policy_load")
        self._keep = keep  # (alive until the next load: the launch reads them stream-ordered)

    def _check(self, x, shape, dtype, name):
        t = self._torch
        if (not isinstance(x, t.Tensor) or x.dtype != dtype or x.device != self.env.device
                or tuple(x.shape) != shape or not x.is_contiguous()):
            raise ValueError("%s must be a contiguous %s tensor of shape %s on %s"
                             % (name, str(dtype).replace("torch.", ""), shape, self.env.device))

    def act(self, features, out=None, probs=None, value=None):
        """Sampled actions int8 [B] of features [B, F] float32 (one launch on the env's stream).
        out, probs [B, A] float32 and value [B] float32 are written when given."""
        t = self._torch
        B = self.env.num_envs
        self._check(features, (B, self.in_features), t.float32, "features")
        dst = self.actions if out is None else out
        self._check(dst, (B,), t.int8, "out")
        if probs is not None:
            self._check(probs, (B, self.n_actions), t.float32, "probs")
        if value is not None:
            self._check(value, (B,), t.float32, "value")
        _lib.check(_lib.load().wab_policy_act(self.env._h, self._p, features.data_ptr(), dst.data_ptr(),
                                              None if probs is None else probs.data_ptr(),
                                              None if value is None else value.data_ptr(),
                                              self.env._stream()), "wab_policy_act")
        return dst

    def _grad_targets(self, into, accumulate):
        """The ten gradient tensors in LAYERS order (weight, bias): `into`'s .grad fields
        (allocated where missing), or fresh ones."""
        t = self._torch
        F, h1, h2, h3, A = self.shape
        shapes = [(h1, F), (h1,), (h2, h1), (h2,), (h3, h2), (h3,), (A, h3), (A,), (1, h3), (1,)]
        names = ["%s.%s" % (n, part) for n in LAYERS for part in ("weight", "bias")]
        if into is None:
            return {k: t.empty(shp, dtype=t.float32, device=self.env.device) for k, shp in zip(names, shapes)}
        out = {}
        for k, shp in zip(names, shapes):
            layer, part = k.split(".")
            prm = getattr(getattr(into, layer, None), part, None)
            if not isinstance(prm, t.Tensor) or tuple(prm.shape) != shp:
                raise ValueError("into.%s must be a tensor of shape %s" % (k, shp))
            if prm.dtype != t.float32 or prm.device != self.env.device:
                raise ValueError("into.%s must be float32 on %s" % (k, self.env.device))
            if prm.grad is None:
                prm.grad = t.zeros_like(prm, memory_format=t.contiguous_format)
            g = prm.grad
            if g.dtype != t.float32 or g.device != self.env.device or not g.is_contiguous() or tuple(g.shape) != shp:
                raise ValueError("into.%s.grad must be a contiguous float32 tensor of shape %s on %s"
                                 % (k, shp, self.env.device))
            out[k] = g
        return out

    def loss_and_grad(self, features, actions, weight, target, *, value_coef=1.0, entropy_coef=0.0,
                      value_loss="smooth_l1", reduction="sum", into=None, accumulate=False, return_rows=False,
                      chunk_rows=0, scale=None, rows=None):
        """finish_episode()'s loss and loss.backward() (actor_critic.py:148-165) on the env's stream,
        no host synchronisation: features [N, F] or [T, B, F] (viewed, not copied), actions int8,
        weight (the reference's R - value.item(), or an advantage; a constant) and target float32
        of the leading shape.  loss = scale (loss_policy + value_coef loss_value - entropy_coef
        entropy), scale 1 ("sum") or 1 / N ("mean") unless `scale` gives it; the three parts are
        returned unscaled.  chunk_rows: rows per pass through the workspace (0: the default).
        into=model writes (accumulate=True: adds to) each parameter's .grad; otherwise the result
        holds "grads", the ten tensors by name.  Returns 0-d device tensors "loss", "loss_policy",
        "loss_value", "entropy", and with return_rows "logp", "value", "entropy_rows" [N].
        Rows whose action is out of range are left out and counted: check() raises for them.
        rows (wab_policy_grad_gather): a 1-d contiguous int32 tensor [N] on the features' device (a
        slice such as perm[a:b] is one; int64 is converted with .to(torch.int32), one small launch,
        no synchronisation).  features and the per-row tensors are then the source ([M, F] or
        [T, B, F], M = T B) and row i of the call is source row rows[i]; an index may repeat.  No
        copy is made: the result is, bit for bit, that of the call on index_select copies.
        N = rows.numel() is what "mean" divides by, and the row outputs are [N].  An index outside
        [0, M) is never followed: its row is left out and counted, and check() raises for it."""
        t = self._torch
        n = check_loss_args(self.shape, features, actions, weight, target, value_loss, reduction, into, accumulate)
        if features.device != self.env.device:
            raise ValueError("features must be on %s" % (self.env.device,))
        n, gather = self._row_index(rows, n)
        grads = self._grad_targets(into, accumulate)
        L = _lib.load()
        cfg = _lib.WabPolicyLoss(float(value_coef), float(entropy_coef), _lib.VALUE_LOSS[value_loss],
                                 float(scale) if scale is not None else (1.0 / n if reduction == "mean" and n > 0
                                                                         else 1.0), 1 if accumulate else 0,
                                 int(chunk_rows))
        self._workspace(n, chunk_rows)
        loss = t.zeros(4, dtype=t.float32, device=self.env.device)
        rows = [t.empty(n, dtype=t.float32, device=self.env.device) for _ in range(3)] if return_rows else [None] * 3
        gw = _lib.WabPolicyWeights(*[grads["%s.%s" % (nm, part)].data_ptr() for nm in LAYERS
                                     for part in ("weight", "bias")])
        call = L.wab_policy_grad_gather if gather else L.wab_policy_grad
        _lib.check(call(self._p, features.data_ptr(), actions.data_ptr(), weight.data_ptr(),
                        target.data_ptr(), n, ctypes.addressof(cfg), ctypes.addressof(gw),
                        loss.data_ptr(), *[None if r is None else r.data_ptr() for r in rows],
                        self._grad_ws.data_ptr(), self._grad_ws.numel(), self.env._stream(), *gather),
                   "wab_policy_grad_gather" if gather else "wab_policy_grad")
        out = {"loss": loss[3], "loss_policy": loss[0], "loss_value": loss[1], "entropy": loss[2]}
        if into is None:
            out["grads"] = grads
        if return_rows:
            lead = (n,) if gather else tuple(features.shape[:-1])
            out["logp"], out["value"], out["entropy_rows"] = [r.view(lead) for r in rows]
        return out

    def _row_index(self, rows, m):
        """(N, the _gather calls' trailing arguments) of a call whose checked source has m rows:
        (m, ()) without an index; with one (rows.numel(), (its address, m)), an int64 index
        converted on the stream (the copy is kept until the next call, so nothing allocated before
        the launch can take its memory)."""
        if rows is None:
            return m, ()
        n = check_row_index(rows, self.env.device)
        if m < 1:
            raise ValueError("rows= needs a source of at least one row")
        if rows.dtype != self._torch.int32:
            rows = rows.to(self._torch.int32)
        self._rows_keep = rows
        return n, (rows.data_ptr() if n > 0 else None, m)

    def _workspace(self, n, chunk_rows):
        L = _lib.load()
        need = L.wab_policy_grad_workspace(self._p, n, int(chunk_rows))
        if need == 0:
            _lib.check(-1, "wab_policy_grad_workspace")
        if self._grad_ws is None or self._grad_ws.numel() < need:
            self._grad_ws = self._torch.empty(need, dtype=self._torch.uint8, device=self.env.device)
        return self._grad_ws

    def evaluate(self, features, actions=None, rows=None):
        """Forward and head alone (wab_policy_evaluate), one launch on the env's stream, no host
        synchronisation: {"value", "entropy"} float32 of features' leading shape ([N, F] or
        [T, B, F], viewed), and "logp" with `actions` (int8 of that shape).  The bits are those
        loss_and_grad(return_rows=True) returns, so under unchanged weights a PPO ratio built from
        this logp is exactly 1.  A row whose action is out of range has logp 0 and is counted:
        check() raises for it.  rows: as loss_and_grad's (wab_policy_evaluate_gather); the results
        are then [N], in the index's order."""
        t = self._torch
        n = check_rows(self.shape, features, **({} if actions is None else {"actions": actions}))
        if features.device != self.env.device:
            raise ValueError("features must be on %s" % (self.env.device,))
        n, gather = self._row_index(rows, n)
        if self._grad_ws is None:
            self._grad_ws = t.empty(256, dtype=t.uint8, device=self.env.device)
        names = (("logp",) if actions is not None else ()) + ("value", "entropy")
        rows = {k: t.empty(n, dtype=t.float32, device=self.env.device) for k in names}
        L = _lib.load()
        _lib.check((L.wab_policy_evaluate_gather if gather else L.wab_policy_evaluate)(
            self._p, features.data_ptr(), None if actions is None else actions.data_ptr(), n,
            *[rows[k].data_ptr() if k in rows else None for k in ("logp", "value", "entropy")],
            self._grad_ws.data_ptr(), self._grad_ws.numel(), self.env._stream(), *gather),
            "wab_policy_evaluate_gather" if gather else "wab_policy_evaluate")
        lead = (n,) if gather else tuple(features.shape[:-1])
        return {k: r.view(lead) for k, r in rows.items()}

    def ppo_loss_and_grad(self, features, actions, advantage, target, old_logp, *, clip=0.2, old_value=None,
                          value_clip=None, value_coef=1.0, entropy_coef=0.0, value_loss="smooth_l1", reduction="sum",
                          into=None, accumulate=False, return_rows=False, chunk_rows=0, scale=None, rows=None):
        """loss_and_grad with PPO's clipped surrogate (wab_policy_grad_ppo; the contract is
        reference_ppo_loss_and_grad): old_logp from evaluate() before the first step, float32 of
        the leading shape; value_clip > 0 clips the value loss around old_value (the rollout's
        value).  A minibatch is a contiguous row range, features[t0:t1] of a [T, B, F] segment (a
        view), or with rows= (as loss_and_grad's; wab_policy_grad_ppo_gather) any rows of the whole
        segment, such as a slice of a fresh permutation per epoch: every per-row tensor is then the
        segment's.  accumulate=True sums several minibatches into one step.  Returns loss_and_grad's keys
        and 0-d device tensors "clip_fraction", "approx_kl" (Schulman's k3), "value_clip_fraction"
        and "ratio_mean", each a sum over the rows divided by N on the device ("ppo_sums": the
        four sums themselves); with return_rows also "ratio"."""
        t = self._torch
        n = check_ppo_args(self.shape, features, actions, advantage, target, old_logp, clip, old_value, value_clip,
                           value_loss, reduction, into, accumulate)
        if features.device != self.env.device:
            raise ValueError("features must be on %s" % (self.env.device,))
        n, gather = self._row_index(rows, n)
        # (no rows: nothing to clip, and an empty old_value has no address to pass)
        vclip = float(value_clip) if value_clip is not None and float(value_clip) > 0 and n > 0 else 0.0
        grads = self._grad_targets(into, accumulate)
        cfg = _lib.WabPolicyLoss(float(value_coef), float(entropy_coef), _lib.VALUE_LOSS[value_loss],
                                 float(scale) if scale is not None else (1.0 / n if reduction == "mean" and n > 0
                                                                         else 1.0), 1 if accumulate else 0,
                                 int(chunk_rows))
        ppo = _lib.WabPpoConfig(float(clip), vclip)
        ws = self._workspace(n, chunk_rows)
        sums = t.zeros(8, dtype=t.float32, device=self.env.device)  # loss_out[4], ppo_out[4]
        rows = [t.empty(n, dtype=t.float32, device=self.env.device) for _ in range(4)] if return_rows else [None] * 4
        gw = _lib.WabPolicyWeights(*[grads["%s.%s" % (nm, part)].data_ptr() for nm in LAYERS
                                     for part in ("weight", "bias")])
        L = _lib.load()
        _lib.check((L.wab_policy_grad_ppo_gather if gather else L.wab_policy_grad_ppo)(
            self._p, features.data_ptr(), actions.data_ptr(), advantage.data_ptr(), target.data_ptr(),
            old_logp.data_ptr(), old_value.data_ptr() if vclip > 0 else None, n, ctypes.addressof(cfg),
            ctypes.addressof(ppo), ctypes.addressof(gw), sums.data_ptr(), sums[4:].data_ptr(),
            *[None if r is None else r.data_ptr() for r in rows], ws.data_ptr(), ws.numel(), self.env._stream(),
            *gather), "wab_policy_grad_ppo_gather" if gather else "wab_policy_grad_ppo")
        out = {"loss": sums[3], "loss_policy": sums[0], "loss_value": sums[1], "entropy": sums[2]}
        diag = sums[4:] / float(max(n, 1))
        out["clip_fraction"], out["approx_kl"], out["value_clip_fraction"], out["ratio_mean"] = diag.unbind(0)
        out["ppo_sums"] = sums[4:]
        if into is None:
            out["grads"] = grads
        if return_rows:
            lead = (n,) if gather else tuple(features.shape[:-1])
            out["logp"], out["value"], out["entropy_rows"], out["ratio"] = [r.view(lead) for r in rows]
        return out

    def check(self):
        """Synchronises; raises IndexError if the latest loss_and_grad left rows out because their
        action was outside [0, n_actions), or (rows=) their index outside the source's rows."""
        if self._grad_ws is None:
            return
        L = _lib.load()
        for call, name in ((L.wab_policy_grad_bad_actions, "wab_policy_grad_bad_actions"),
                           (L.wab_policy_grad_bad_rows, "wab_policy_grad_bad_rows")):
            bad = ctypes.c_uint64(0)
            rc = call(self._p, self._grad_ws.data_ptr(), self.env._stream(), ctypes.byref(bad))
            if bad.value:
                raise IndexError(L.wab_last_error().decode(errors="replace"))
            _lib.check(rc, name)

    def close(self):
        if getattr(self, "_p", None) is not None and self._p.value:
            _lib.load().wab_policy_destroy(self._p)
            self._p = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DeviceAdam:
    """torch.optim.Adam (AdamW with decoupled=True) for the ten parameters of a DevicePolicy's
    model, stepped on the device by wab_policy_adam_step: the global-norm clip (max_grad_norm > 0,
    torch's clip_grad_norm_ rule), no step at all on a non-finite gradient, the Adam update of the
    float32 parameters in place (model.state_dict() stays the truth) and the policy's bf16 image
    in the same launch, so no policy.load(model) follows a step().  What it computes is
    reference_adam_step.  Three launches on the env's stream, no host synchronisation: step() can
    be captured in a graph (which then keeps the lr of the capture).

        opt = DeviceAdam(policy, model, lr=3e-4, max_grad_norm=0.5)
        policy.loss_and_grad(..., into=model);  opt.step()

    The policy must hold the model's current weights (policy.load(model), as DevicePolicy(model,
    env) leaves it); parameters changed by other hands need a policy.load(model) again."""

    def __init__(self, policy, model, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, decoupled=False,
                 max_grad_norm=0.0):
        import torch

        self._torch = torch
        check_adam_args(lr, betas, eps, weight_decay, max_grad_norm)
        self.policy = policy
        self.lr, self.betas, self.eps = float(lr), (float(betas[0]), float(betas[1])), float(eps)
        self.weight_decay, self.decoupled = float(weight_decay), bool(decoupled)
        self.max_grad_norm = float(max_grad_norm)
        dev = policy.env.device
        if shape_of(model) != policy.shape:
            raise ValueError("the model's layers differ from the policy's %s" % (policy.shape,))
        self.params = []
        for name in ADAM_TENSORS:
            layer, part = name.split(".")
            prm = getattr(getattr(model, layer), part)
            if prm.dtype != torch.float32 or prm.device != dev or not prm.is_contiguous():
                raise ValueError("%s must be a contiguous float32 tensor on %s (it is updated in place)" % (name, dev))
            self.params.append(prm)
        all_params = list(model.parameters())
        self._order = []
        for name, prm in zip(ADAM_TENSORS, self.params):
            idx = [i for i, q in enumerate(all_params) if q is prm]
            if len(idx) != 1:
                raise ValueError("%s is not one of model.parameters()" % name)
            self._order.append(idx[0])
        if len(all_params) != len(self.params):
            raise ValueError("the model has %d parameters; DeviceAdam steps the ten of the policy's five Linears "
                             "and would leave the others untrained" % len(all_params))
        self.exp_avg = [torch.zeros_like(p) for p in self.params]
        self.exp_avg_sq = [torch.zeros_like(p) for p in self.params]
        L = _lib.load()
        need = int(L.wab_policy_adam_workspace(policy._p))
        if need == 0:
            _lib.check(-1, "wab_policy_adam_workspace")
        self._ws = torch.empty(need // 8, dtype=torch.float64, device=dev)
        self._state = torch.zeros(ctypes.sizeof(_lib.WabAdamState) // 8, dtype=torch.int64, device=dev)
        self._w = [_lib.WabPolicyWeights(*[x.data_ptr() for x in xs])
                   for xs in (self.params, self.exp_avg, self.exp_avg_sq)]

    def _config(self):
        check_adam_args(self.lr, self.betas, self.eps, self.weight_decay, self.max_grad_norm)
        return _lib.WabAdamConfig(self.lr, self.betas[0], self.betas[1], self.eps, self.weight_decay,
                                  self.max_grad_norm, 1 if self.decoupled else 0)

    def step(self):
        """One optimizer step from each parameter's .grad (RuntimeError if one is missing)."""
        t = self._torch
        ptrs = []
        for name, prm in zip(ADAM_TENSORS, self.params):
            g = prm.grad
            if g is None:
                raise RuntimeError("%s has no .grad: run loss_and_grad(..., into=model) (or backward()) before "
                                   "step()" % name)
            if g.dtype != t.float32 or g.device != prm.device or not g.is_contiguous() or g.shape != prm.shape:
                raise ValueError("%s.grad must be a contiguous float32 tensor of the parameter's shape and device"
                                 % name)
            ptrs.append(g.data_ptr())
        gw = _lib.WabPolicyWeights(*ptrs)
        cfg = self._config()
        pol = self.policy
        _lib.check(_lib.load().wab_policy_adam_step(pol._p, ctypes.addressof(self._w[0]), ctypes.addressof(gw),
                                                    ctypes.addressof(self._w[1]), ctypes.addressof(self._w[2]),
                                                    ctypes.addressof(cfg), self._state.data_ptr(), self._ws.data_ptr(),
                                                    self._ws.numel() * 8, pol.env._stream()), "wab_policy_adam_step")

    def zero_grad(self, set_to_none=False):
        """As torch's, with set_to_none False by default: loss_and_grad(into=model) overwrites the
        gradients, and a captured graph needs them to stay where they are."""
        for prm in self.params:
            if prm.grad is not None:
                if set_to_none:
                    prm.grad = None
                else:
                    prm.grad.zero_()

    def _read_state(self):
        raw = self._state.cpu().numpy().tobytes()  # (synchronises)
        return _lib.WabAdamState.from_buffer_copy(raw)

    def stats(self):
        """{"step", "skipped", "grad_norm", "clip_scale"}: steps taken, calls skipped for a
        non-finite gradient, and the latest call's gradient norm and clip factor.  Synchronises."""
        s = self._read_state()
        return {"step": int(s.step), "skipped": int(s.skipped), "grad_norm": float(s.grad_norm),
                "clip_scale": float(s.clip_scale)}

    def state_dict(self):
        """torch.optim.Adam's state_dict() layout (adam_state_dict), so that a checkpoint moves
        between the two optimizers.  Synchronises."""
        s = self._read_state()
        return adam_state_dict(int(s.step), self.exp_avg, self.exp_avg_sq, self._order, self.lr, self.betas, self.eps,
                               self.weight_decay, self.decoupled, self.max_grad_norm)

    def load_state_dict(self, sd):
        """Take the step count, moments and hyperparameters of a state_dict() of DeviceAdam or of
        torch.optim.Adam / AdamW over the same model; the beta powers are rebuilt by `step`
        sequential double multiplications.  The skipped count starts again at 0."""
        t = self._torch
        step, m, v, hyper = parse_adam_state_dict(sd, self._order, [tuple(p.shape) for p in self.params])
        self.lr, self.betas, self.eps = hyper["lr"], hyper["betas"], hyper["eps"]
        self.weight_decay, self.decoupled = hyper["weight_decay"], hyper["decoupled"]
        self.max_grad_norm = hyper.get("max_grad_norm", self.max_grad_norm)
        for k in range(len(self.params)):
            if m is None:
                self.exp_avg[k].zero_()
                self.exp_avg_sq[k].zero_()
            else:
                self.exp_avg[k].copy_(m[k].to(t.float32))
                self.exp_avg_sq[k].copy_(v[k].to(t.float32))
        b1p, b2p = adam_beta_powers(step, self.betas)
        host = _lib.WabAdamState(step, 0, b1p, b2p, 0.0, 0.0, 0)
        self._state.copy_(t.from_numpy(np.frombuffer(bytes(host), dtype=np.int64).copy()))
