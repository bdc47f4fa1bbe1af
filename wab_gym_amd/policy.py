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
    with policy.acting(mode="greedy"):           # evaluation: the first maximum of probs in place of
        monitor.rollout_policy(policy, T)        # the draw (wab_policy_set_action_rule); temperature=
                                                 # scales the logits by 1 / temperature

    opt = DeviceAdam(policy, model, lr=3e-4)     # optimizer.step() and the re-pack in HIP
    opt.step()                                   # (wab_policy_adam_step): no policy.load after it

loss_and_grad fills each parameter's .grad; the caller steps with DeviceAdam, or with a torch
optimizer and reloads.

What the kernels compute is `reference_forward`, `reference_loss_and_grad` (the numeric
contracts, in torch on the CPU), `reference_adam_step` (in numpy), `sample_reference` (the
sampling rule, in numpy) and `select_reference` (the action rule: that, or the greedy first
maximum) of policy_reference.py, re-exported here; the tests check the kernels against them.
The reference's `+ U(0, 1) / 100` input noise (actor_critic.py:189) is not reproduced.
"""
from __future__ import annotations

import contextlib
import ctypes

import numpy as np

from . import _lib

LAYERS = ("affine1", "affine2", "affine3", "action_head", "value_head")
# the ten tensors by name, in wab_policy_weights' order (the flat order of the optimizer's norm)
ADAM_TENSORS = tuple("%s.%s" % (n, part) for n in LAYERS for part in ("weight", "bias"))
SITE_POLICY = 11  # keyed-RNG site of the action draw (the first id free in oracle/keyed_rng.py)


def _state_dict(module_or_state_dict):
    sd = module_or_state_dict
    if hasattr(sd, "state_dict"):
        sd = sd.state_dict()
    out = {}
    for key in ADAM_TENSORS:
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


def check_rows(shape, features, **rows):
    """features [N, F] or [T, B, F] float32, or packed (wab_gym_amd.features) int32 [N, P] or
    [T, B, P], and the named per-row tensors (actions int8, every other float32) of the leading
    shape, all contiguous and on the features' device: returns N."""
    import torch

    F = shape[0]
    if isinstance(features, torch.Tensor) and features.dtype == torch.int32:
        from .features import check_bits

        check_bits(features, F)
        if features.dim() not in (2, 3):
            raise ValueError("packed features must have shape [N, P] or [T, B, P], not %s" % (tuple(features.shape),))
    elif not isinstance(features, torch.Tensor) or features.dtype != torch.float32 or features.dim() not in (2, 3) \
            or features.shape[-1] != F or not features.is_contiguous():
        raise ValueError("features must be a contiguous float32 tensor of shape [N, %d] or [T, B, %d] (or packed "
                         "int32 rows)" % (F, F))
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


def check_action_rule(mode, temperature):
    """The argument checks of wab_policy_set_action_rule, on the host (ValueError): mode "sample"
    or "greedy"; temperature finite and > 0 as a float32, and its float32 reciprocal (what the
    kernels multiply the logits by) finite and normal.  Returns (the mode's WAB_ACT_* number, the
    temperature as float32, its reciprocal as float32)."""
    if not isinstance(mode, str) or mode not in _lib.ACTION_MODE:
        raise ValueError("mode must be 'sample' or 'greedy', not %r" % (mode,))
    with np.errstate(all="ignore"):
        tau = np.float32(temperature)
        if not (np.isfinite(tau) and tau > 0):
            raise ValueError("temperature must be finite and > 0, not %r" % (temperature,))
        inv = np.float32(1.0) / tau
    if not np.isfinite(inv) or inv < np.finfo(np.float32).tiny:
        raise ValueError("1 / temperature must be a normal float32: temperature %r is outside what the kernels "
                         "can scale by" % (temperature,))
    return _lib.ACTION_MODE[mode], tau, inv


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


class DevicePolicy:
    """The policy network on the env's device.  `module_or_state_dict` holds the five Linears by
    the reference's names (affine1, affine2, affine3, action_head, value_head); `env` is the
    BatchedWolvesAndBushesEnv (or a wrapper of it) whose envs it acts for: its episode and turn
    counters key the draw.

    The action rule (set_action_rule, acting) reaches act() and the rollouts only.  evaluate(),
    loss_and_grad() and ppo_loss_and_grad() ignore it: they are temperature 1, bit for bit.  A
    caller who trains on rollouts made under temperature != 1 owns the importance ratio: the
    behaviour log-probability of an action a is log probs[a] of the rollout's probs, not
    evaluate()'s logp."""

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
        self._shapes = dict(zip(ADAM_TENSORS, ((h1, F), (h1,), (h2, h1), (h2,), (h3, h2), (h3,), (A, h3), (A,),
                                                     (1, h3), (1,))))
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
        keep = [sd[k].detach().to(self.env.device, t.float32).contiguous() for k in ADAM_TENSORS]
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

    def set_action_rule(self, mode="sample", temperature=1.0):
        """How act() and the rollouts choose the action (wab_policy_set_action_rule): "sample", the
        keyed draw, or "greedy", the first maximum of the probabilities (ties to the lowest index),
        on the softmax of the logits divided by `temperature`.  Host state only: every act() and
        rollout_policy() enqueued afterwards follows it, a captured graph keeps the rule it was
        captured with, load() and DeviceAdam.step() leave it alone.  ValueError from
        check_action_rule."""
        m, tau, _ = check_action_rule(mode, temperature)
        rule = _lib.WabActionRule(m, float(tau))
        _lib.check(_lib.load().wab_policy_set_action_rule(self._p, ctypes.addressof(rule)),
                   "wab_policy_set_action_rule")

    @property
    def action_rule(self):
        """(mode, temperature) as the library holds them (wab_policy_get_action_rule)."""
        rule = _lib.WabActionRule()
        _lib.check(_lib.load().wab_policy_get_action_rule(self._p, ctypes.addressof(rule)),
                   "wab_policy_get_action_rule")
        names = {v: k for k, v in _lib.ACTION_MODE.items()}
        return names[int(rule.mode)], float(rule.temperature)

    @contextlib.contextmanager
    def acting(self, mode="sample", temperature=1.0):
        """with policy.acting(mode="greedy"): ... sets the rule and restores the previous one on
        exit (what was enqueued inside keeps the rule it was enqueued with)."""
        before = self.action_rule
        self.set_action_rule(mode, temperature)
        try:
            yield self
        finally:
            self.set_action_rule(*before)

    def act(self, features, out=None, probs=None, value=None):
        """Actions int8 [B] of features [B, F] float32 under the policy's action rule (sampled by
        default; one launch on the env's stream).  out, probs [B, A] float32 (the distribution the
        action is taken from) and value [B] float32 are written when given."""
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
        """The ten gradient tensors by name, in ADAM_TENSORS order: `into`'s .grad fields
        (allocated where missing), or fresh ones."""
        t = self._torch
        if into is None:
            return {k: t.empty(shp, dtype=t.float32, device=self.env.device) for k, shp in self._shapes.items()}
        out = {}
        for k, shp in self._shapes.items():
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
        no host synchronisation: features [N, F] or [T, B, F] (viewed, not copied; or packed rows,
        int32 [N, P] or [T, B, P] of wab_gym_amd.features: the dtype selects wab_policy_grad_packed,
        with the same bits in every result), actions int8,
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
        m = check_loss_args(self.shape, features, actions, weight, target, value_loss, reduction, into, accumulate)
        return self._run("grad", features, m, rows, [actions, weight, target],
                         ("logp", "value", "entropy") if return_rows else (None,) * 3,
                         loss=(value_coef, entropy_coef, value_loss, reduction, into, accumulate, chunk_rows, scale))

    def _run(self, name, features, m, rows, per_row, row_names, loss=None, ppo=None):
        """What loss_and_grad ("grad"), ppo_loss_and_grad ("grad_ppo") and evaluate ("evaluate") do
        after their argument checks: one call of wab_policy_<name>, or with rows= of its _gather
        form.  m: the checked source's rows; per_row: the input tensors after features, in the
        call's order (None: not passed); row_names: the call's row outputs in its order, "logp",
        "value", "entropy", "ratio" (None: not wanted); loss: the loss keywords (None: evaluate,
        which keeps nothing in the workspace but the two counts); ppo: (clip, value_clip, old_logp,
        old_value)."""
        t, dev = self._torch, self.env.device
        if features.device != dev:
            raise ValueError("features must be on %s" % (dev,))
        n, gather = self._row_index(rows, m)
        if ppo is not None:
            clip, value_clip, old_logp, old_value = ppo
            # (no rows: nothing to clip, and an empty old_value has no address to pass)
            vclip = float(value_clip) if value_clip is not None and float(value_clip) > 0 and n > 0 else 0.0
            per_row = per_row + [old_logp, old_value if vclip > 0 else None]
        mid, out = [], {}
        if loss is None:
            if self._grad_ws is None:
                self._grad_ws = t.empty(256, dtype=t.uint8, device=dev)
        else:
            value_coef, entropy_coef, value_loss, reduction, into, accumulate, chunk_rows, scale = loss
            grads = self._grad_targets(into, accumulate)
            cfg = _lib.WabPolicyLoss(float(value_coef), float(entropy_coef), _lib.VALUE_LOSS[value_loss],
                                     float(scale) if scale is not None else (1.0 / n if reduction == "mean" and n > 0
                                                                             else 1.0), 1 if accumulate else 0,
                                     int(chunk_rows))
            pcfg = None if ppo is None else _lib.WabPpoConfig(float(clip), vclip)
            self._workspace(n, chunk_rows)
            sums = t.zeros(4 if ppo is None else 8, dtype=t.float32, device=dev)  # loss_out[4], ppo_out[4]
            gw = _lib.WabPolicyWeights(*[grads[k].data_ptr() for k in ADAM_TENSORS])
            mid = [ctypes.addressof(x) for x in (cfg, pcfg, gw) if x is not None] + [sums.data_ptr()]
            if ppo is not None:
                mid.append(sums[4:].data_ptr())
        bufs = [None if k is None else t.empty(n, dtype=t.float32, device=dev) for k in row_names]
        # (int32 features are packed rows: the _packed calls, whose index is optional)
        packed = features.dtype == t.int32
        symbol = "wab_policy_%s%s" % (name, "_packed" if packed else "_gather" if gather else "")
        if packed and not gather:
            gather = (None, 0)
        _lib.check(getattr(_lib.load(), symbol)(
            self._p, features.data_ptr(), *[None if x is None else x.data_ptr() for x in per_row], n, *mid,
            *[None if r is None else r.data_ptr() for r in bufs],
            self._grad_ws.data_ptr(), self._grad_ws.numel(), self.env._stream(), *gather), symbol)
        if loss is not None:
            out = {"loss": sums[3], "loss_policy": sums[0], "loss_value": sums[1], "entropy": sums[2]}
            if ppo is not None:
                diag = sums[4:] / float(max(n, 1))
                out["clip_fraction"], out["approx_kl"], out["value_clip_fraction"], out["ratio_mean"] = diag.unbind(0)
                out["ppo_sums"] = sums[4:]
            if into is None:
                out["grads"] = grads
        lead = (n,) if rows is not None else tuple(features.shape[:-1])
        for k, r in zip(row_names, bufs):  # (beside the loss's sums, the entropy rows are "entropy_rows")
            if r is not None:
                out["entropy_rows" if loss is not None and k == "entropy" else k] = r.view(lead)
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
        m = check_rows(self.shape, features, **({} if actions is None else {"actions": actions}))
        return self._run("evaluate", features, m, rows, [actions],
                         ("logp" if actions is not None else None, "value", "entropy"))

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
        m = check_ppo_args(self.shape, features, actions, advantage, target, old_logp, clip, old_value, value_clip,
                           value_loss, reduction, into, accumulate)
        return self._run("grad_ppo", features, m, rows, [actions, advantage, target],
                         ("logp", "value", "entropy", "ratio") if return_rows else (None,) * 4,
                         loss=(value_coef, entropy_coef, value_loss, reduction, into, accumulate, chunk_rows, scale),
                         ppo=(clip, value_clip, old_logp, old_value))

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
        step, m, v, hyper = parse_adam_state_dict(sd, self._order, list(self.policy._shapes.values()))
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


# The numeric contracts (policy_reference.py), by name: every policy.X of before the split resolves.
# (At the end: policy_reference imports this module's names, and either can be imported first.)
from .policy_reference import (adam_fresh_state, keyed_u, pair_tree_sum, reference_adam_step,  # noqa: E402,F401
                               reference_forward, reference_loss_and_grad, reference_ppo_loss_and_grad,
                               sample_reference, select_reference, _reference_gather, _reference_head_and_backward,
                               _value_loss)
