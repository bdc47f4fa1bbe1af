"""DevicePolicy — actor_critic.py's Policy (actor_critic.py:54-97) for inference on device, the
action sampled in the same launch (wab_policy_act, wab_gym_amd/csrc/wab_policy.hip).

    policy = DevicePolicy(model, env)            # model: the five Linears by the reference's names
    actions = policy.act(features)               # int8 [B]; probs=/value= tensors are filled too
    ...optimizer.step()...; policy.load(model)   # stream-ordered re-pack, no host sync
    policy.loss_and_grad(features, actions, weight, target, into=model)   # finish_episode's loss
                                                 # and loss.backward() (wab_policy_grad)

The optimizer stays in torch: loss_and_grad fills each parameter's .grad, the caller steps and
reloads.

What the kernels compute is `reference_forward` and `reference_loss_and_grad` below (the numeric
contracts, in torch on the CPU) and `sample_reference` (the sampling rule, in numpy); the tests
check the kernels against them.
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


def reference_loss_and_grad(state_dict, features, actions, weight, target, value_coef=1.0, entropy_coef=0.0,
                            value_loss="smooth_l1", scale=1.0, round_grads=True):
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
    "grads": the ten tensors in torch Linear layout}, all float64."""
    import torch

    if value_loss not in ("smooth_l1", "mse"):
        raise ValueError("value_loss must be 'smooth_l1' or 'mse'")
    sd = {k: v.detach().to("cpu", torch.float32) for k, v in _state_dict(state_dict).items()}

    def bf(x):
        return x.to(torch.float32).to(torch.bfloat16).to(torch.float64)

    def rd(g):
        return bf(g) if round_grads else g

    x0 = bf(torch.as_tensor(features).detach().to("cpu", torch.float32))
    a = torch.as_tensor(actions).detach().to("cpu", torch.int64)
    w = torch.as_tensor(weight).detach().to("cpu", torch.float64)
    tg = torch.as_tensor(target).detach().to("cpu", torch.float64)
    hidden = []
    _, v = reference_forward(sd, features, hidden=hidden)
    xs = [x0] + [h[1] for h in hidden]
    wq = {n: bf(sd[n + ".weight"]) for n in LAYERS}
    logits = xs[3] @ wq["action_head"].T + sd["action_head.bias"].to(torch.float64)
    zc = logits - logits.max(dim=-1, keepdim=True).values
    logp_all = zc - torch.log(torch.exp(zc).sum(dim=-1, keepdim=True))
    p = torch.exp(logp_all)
    H = -(p * logp_all).sum(dim=-1)
    onehot = torch.zeros_like(p)
    onehot[torch.arange(len(a)), a] = 1.0
    logp = (logp_all * onehot).sum(dim=-1)
    d = v - tg
    if value_loss == "mse":
        lv, dv = 0.5 * d * d, d
    else:
        lv = torch.where(d.abs() < 1.0, 0.5 * d * d, d.abs() - 0.5)
        dv = torch.where(d.abs() < 1.0, d, torch.sign(d))
    loss_policy, loss_value, loss_entropy = -(w * logp).sum(), lv.sum(), H.sum()
    total = scale * (loss_policy + value_coef * loss_value - entropy_coef * loss_entropy)

    Da = rd(w[:, None] * (p - onehot) + entropy_coef * p * (logp_all + H[:, None]))
    Dv = rd(value_coef * dv)[:, None]
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
    return {"loss": (loss_policy, loss_value, loss_entropy, total), "logp": logp, "value": v, "entropy": H,
            "grads": grads}


def check_loss_args(shape, features, actions, weight, target, value_loss="smooth_l1", reduction="sum", into=None,
                    accumulate=False):
    """loss_and_grad's checks that need no device: returns N, the row count.  features [N, F] or
    [T, B, F] float32, actions int8, weight and target float32 of the leading shape, all
    contiguous and on one device."""
    import torch

    F = shape[0]
    if not isinstance(features, torch.Tensor) or features.dtype != torch.float32 or features.dim() not in (2, 3) \
            or features.shape[-1] != F or not features.is_contiguous():
        raise ValueError("features must be a contiguous float32 tensor of shape [N, %d] or [T, B, %d]" % (F, F))
    lead = tuple(features.shape[:-1])
    for name, x, dt in (("actions", actions, torch.int8), ("weight", weight, torch.float32),
                        ("target", target, torch.float32)):
        if not isinstance(x, torch.Tensor) or x.dtype != dt or tuple(x.shape) != lead or not x.is_contiguous() \
                or x.device != features.device:
            raise ValueError("%s must be a contiguous %s tensor of shape %s on %s"
                             % (name, str(dt).replace("torch.", ""), lead, features.device))
    if value_loss not in _lib.VALUE_LOSS:
        raise ValueError("value_loss must be 'smooth_l1' or 'mse', not %r" % (value_loss,))
    if reduction not in ("sum", "mean"):
        raise ValueError("reduction must be 'sum' or 'mean', not %r" % (reduction,))
    if accumulate and into is None:
        raise ValueError("accumulate=True needs into=: there is no earlier gradient to add to")
    n = 1
    for k in lead:
        n *= int(k)
    if n >= 1 << 31:
        raise ValueError("loss_and_grad takes fewer than 2^31 rows")
    return n


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
                      chunk_rows=0, scale=None):
        """finish_episode()'s loss and loss.backward() (actor_critic.py:148-165) on the env's stream,
        no host synchronisation: features [N, F] or [T, B, F] (viewed, not copied), actions int8,
        weight (the reference's R - value.item(), or an advantage; a constant) and target float32
        of the leading shape.  loss = scale (loss_policy + value_coef loss_value - entropy_coef
        entropy), scale 1 ("sum") or 1 / N ("mean") unless `scale` gives it; the three parts are
        returned unscaled.  chunk_rows: rows per pass through the workspace (0: the default).
        into=model writes (accumulate=True: adds to) each parameter's .grad; otherwise the result
        holds "grads", the ten tensors by name.  Returns 0-d device tensors "loss", "loss_policy",
        "loss_value", "entropy", and with return_rows "logp", "value", "entropy_rows" [N].
        Rows whose action is out of range are left out and counted: check() raises for them."""
        t = self._torch
        n = check_loss_args(self.shape, features, actions, weight, target, value_loss, reduction, into, accumulate)
        if features.device != self.env.device:
            raise ValueError("features must be on %s" % (self.env.device,))
        grads = self._grad_targets(into, accumulate)
        L = _lib.load()
        cfg = _lib.WabPolicyLoss(float(value_coef), float(entropy_coef), _lib.VALUE_LOSS[value_loss],
                                 float(scale) if scale is not None else (1.0 / n if reduction == "mean" and n > 0
                                                                         else 1.0), 1 if accumulate else 0,
                                 int(chunk_rows))
        need = L.wab_policy_grad_workspace(self._p, n, int(chunk_rows))
        if need == 0:
            _lib.check(-1, "wab_policy_grad_workspace")
        if self._grad_ws is None or self._grad_ws.numel() < need:
            self._grad_ws = t.empty(need, dtype=t.uint8, device=self.env.device)
        loss = t.zeros(4, dtype=t.float32, device=self.env.device)
        rows = [t.empty(n, dtype=t.float32, device=self.env.device) for _ in range(3)] if return_rows else [None] * 3
        gw = _lib.WabPolicyWeights(*[grads["%s.%s" % (nm, part)].data_ptr() for nm in LAYERS
                                     for part in ("weight", "bias")])
        _lib.check(L.wab_policy_grad(self._p, features.data_ptr(), actions.data_ptr(), weight.data_ptr(),
                                     target.data_ptr(), n, ctypes.addressof(cfg), ctypes.addressof(gw),
                                     loss.data_ptr(), *[None if r is None else r.data_ptr() for r in rows],
                                     self._grad_ws.data_ptr(), self._grad_ws.numel(), self.env._stream()),
                   "wab_policy_grad")
        out = {"loss": loss[3], "loss_policy": loss[0], "loss_value": loss[1], "entropy": loss[2]}
        if into is None:
            out["grads"] = grads
        if return_rows:
            lead = tuple(features.shape[:-1])
            out["logp"], out["value"], out["entropy_rows"] = [r.view(lead) for r in rows]
        return out

    def check(self):
        """Synchronises; raises IndexError if the latest loss_and_grad left rows out because their
        action was outside [0, n_actions)."""
        if self._grad_ws is None:
            return
        bad = ctypes.c_uint64(0)
        rc = _lib.load().wab_policy_grad_bad_actions(self._p, self._grad_ws.data_ptr(), self.env._stream(),
                                                     ctypes.byref(bad))
        if bad.value:
            raise IndexError(_lib.load().wab_last_error().decode(errors="replace"))
        _lib.check(rc, "wab_policy_grad_bad_actions")

    def close(self):
        if getattr(self, "_p", None) is not None and self._p.value:
            _lib.load().wab_policy_destroy(self._p)
            self._p = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
