"""DevicePolicy — actor_critic.py's Policy (actor_critic.py:54-97) for inference on device, the
action sampled in the same launch (wab_policy_act, wab_gym_amd/csrc/wab_policy.hip).

    policy = DevicePolicy(model, env)            # model: the five Linears by the reference's names
    actions = policy.act(features)               # int8 [B]; probs=/value= tensors are filled too
    ...optimizer.step()...; policy.load(model)   # stream-ordered re-pack, no host sync

Training stays in torch (backward, Adam, the batched re-forward over the stored features).

What the kernel computes is `reference_forward` below (the numeric contract, in torch on the CPU)
and `sample_reference` (the sampling rule, in numpy); the tests check the kernel against them.
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

    def close(self):
        if getattr(self, "_p", None) is not None and self._p.value:
            _lib.load().wab_policy_destroy(self._p)
            self._p = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
