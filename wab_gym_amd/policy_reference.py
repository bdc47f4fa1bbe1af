"""The device policy's numeric contracts, float64 on the CPU: what wab_policy_act, wab_policy_grad,
wab_policy_grad_ppo, wab_policy_evaluate and wab_policy_adam_step compute, stated in torch
(`reference_forward`, `reference_loss_and_grad`, `reference_ppo_loss_and_grad`) and numpy
(`reference_adam_step`, `sample_reference`, `keyed_u`).  The tests check the kernels against them;
no product path calls them.  wab_gym_amd.policy re-exports every public name here.
"""
from __future__ import annotations

import numpy as np


def reference_forward(state_dict, features, hidden=None, temperature=1.0):
    """The kernel's numeric contract in torch on the CPU: every matmul operand (features, weights,
    hidden activations after bias, leaky_relu and clamp) rounded to bf16 (nearest even), everything
    else in float64 (the kernel: fp32 MFMA accumulation, fp32 bias / leaky_relu(0.01) / clamp(-4, 4)
    / max-subtracted softmax / value).  Returns (probs [B, A], value [B]) as float64 tensors.
    `hidden`, a list, receives each hidden layer's (pre-activation, bf16 output) pair.
    temperature (the action rule of act and rollout): the logits, bias included, are scaled by
    float64(float32(1) / float32(temperature)), the factor the kernel multiplies by; the value is
    not scaled, and 1.0 leaves every bit."""
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
    if temperature != 1.0:
        logits = logits * float(np.float32(1.0) / np.float32(temperature))
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


def select_reference(probs_f32, seed, env_ids, episode, turn, mode="sample"):
    """The action rule in numpy on the float32 probabilities the kernel writes: "sample" is
    sample_reference; "greedy" is the first maximum, a = 0, best = p_0, then for k = 1 .. A - 1:
    if p_k > best: best, a = p_k, k (ties to the lowest index, a row of NaNs gives 0; no draw is
    made, and seed, env_ids, episode and turn are not read).  int8 [B]."""
    if mode == "sample":
        return sample_reference(probs_f32, seed, env_ids, episode, turn)
    if mode != "greedy":
        raise ValueError("mode must be 'sample' or 'greedy', not %r" % (mode,))
    p = np.asarray(probs_f32)
    if p.dtype != np.float32:
        raise ValueError("probs must be float32: the rule is defined on the values the kernel writes")
    a = np.zeros(p.shape[0], np.int8)
    best = p[:, 0].copy()
    for k in range(1, p.shape[1]):
        up = p[:, k] > best
        best = np.where(up, p[:, k], best)
        a[up] = k
    return a


# At the end, as policy.py's re-export of this module is: either module can then be imported first.
# (The functions above read these names when they are called.)
from .policy import (ADAM_TENSORS, LAYERS, SITE_POLICY, _state_dict, adam_beta_powers,  # noqa: E402,F401
                     check_adam_args)
