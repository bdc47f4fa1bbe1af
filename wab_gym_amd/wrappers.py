"""Batched observation wrappers and the actor-critic return scan (config 5).

`PragmaticObsWrapper` mirrors the reference wrapper (wab_env.py:670-824) for a batched env:
`observation(obs)` turns the batched 7-tuple into the wrapper's 11-tuple already flattened
the way actor_critic.py feeds the policy (`gym.spaces.flatten`, actor_critic.py:188), i.e. a
float32 tensor [B, 449] computed on device by one HIP kernel (wab_featurize).
`SuperBasicObservationWrapper` (wab_env.py:900-927) does the same for its 4-tuple
(nearest bush, food, role, status): float32 [B, 90] (wab_featurize_superbasic).
"""
from __future__ import annotations

import ctypes
import warnings

from . import _lib
from .spaces import Box, Discrete, Tuple


class PragmaticObsWrapper:
    def __init__(self, env):
        self.env = env
        lib = _lib.load()
        F = lib.wab_feature_dim(env._h)
        if F < 0:
            raise ValueError("PragmaticObsWrapper cannot index a %dx%d viewport (wab_env.py:742)"
                             % (env.W, env.H))
        self.feature_dim = int(F)
        opts = env.game_options
        self.max_distance = opts["width"] // 2 + opts["height"] // 2 + 1  # wab_env.py:709
        md = self.max_distance
        self.single_observation_space = Tuple((                          # wab_env.py:710-724
            Tuple([Discrete(md + 1)] * 4), Tuple([Discrete(md + 1)] * 4), Tuple([Discrete(11)] * 4),
            Tuple([Discrete(md + 1)] * 4), Tuple([Discrete(md + 1)] * 4), Tuple([Discrete(11)] * 4),
            Discrete(2), Discrete(opts["turns_to_empty_food"] + 1), Discrete(2), Discrete(3),
            Box(0, 1, (121,))))
        self.observation_space = Box(0.0, 1.0, (env.num_envs, self.feature_dim), dtype="float32")
        self.action_space = env.action_space
        self.spec = env.spec
        t = env._torch
        self.features = t.zeros((env.num_envs, self.feature_dim), dtype=t.float32, device=env.device)

    def __getattr__(self, name):
        return getattr(self.env, name)

    def observation(self, obs=None, view_mask=None, out=None):
        """Features of the env's current observation buffer (or of `obs`, a dict with
        planes [B,3,W,S] and scalars [3,B] u8 tensors).  Returns float32 [B, F] (a view
        of `out` or of a wrapper-owned buffer overwritten by the next call)."""
        env = self.env
        t = env._torch
        if obs is None:
            env._require_planes()
            st = env._obs["struct"]
            keep = None
        else:
            st, keep = env._obs_struct(obs)
        vm = None
        if view_mask is not None:
            vm = t.as_tensor(view_mask, device=env.device).to(t.uint8).contiguous()
        dst = self.features if out is None else out
        env._check_features(dst, self.feature_dim)
        _lib.check(_lib.load().wab_featurize(env._h, ctypes.addressof(st),
                                             None if vm is None else vm.data_ptr(), dst.data_ptr(),
                                             env._stream()), "wab_featurize")
        del keep
        return dst

    def reset(self, mask=None):
        self.env.reset(mask)
        return self.observation()

    def rollout(self, actions, gamma=0.99, bootstrap=None):
        """T steps of this wrapper with the actions [T, B] and the discounted returns of the
        segment (actor_critic.py:139-143, 185-200): (features [T,B,F], reward [T,B], done [T,B],
        returns [T,B]), one kernel launch where the fused path applies (env.rollout_features)."""
        if type(self) is not PragmaticObsWrapper:
            raise NotImplementedError("rollout() fuses PragmaticObsWrapper only")
        r = self.env.rollout_features(actions, gamma=gamma, bootstrap=bootstrap)
        if r["features"].shape[0] > 0:
            self.features.copy_(r["features"][-1])  # as after T step() calls
        return r["features"], r["reward"], r["done"].view(self.env._torch.bool), r["returns"]

    def rollout_policy(self, policy, T, gamma=0.99, store_planes=False, store_features=True, return_probs=False,
                       fused=None, normalize=False, bootstrap_value=False, gae_lambda=None, whiten=False):
        """T closed-loop steps of actor_critic.main's loop (actor_critic.py:185-200) on the env's
        stream: step t's action is chosen by `policy` (a DevicePolicy) from step t's features under
        its action rule (sampled by default; policy.acting(mode="greedy") for evaluation), then
        the env steps.  No host synchronisation, so the whole call can be captured in a graph.  It
        starts from the features of the current observation (recomputed from the env's obs planes
        when they are valid, else the wrapper's own `features` as its last reset()/step()/rollout
        left them).  Returns a dict: features [T,B,F] f32 (features[t] is what actions[t] was chosen
        from; None with store_features=False), actions [T,B] int8, reward [T,B] f32, done [T,B] u8,
        value [T,B] f32, returns [T,B] f32 (discounted_returns(env=...), R after the last step = 0),
        with return_probs, probs [T,B,A] f32, and with normalize=True, normalized [T,B] f32
        (normalized_returns of the call's returns and done, actor_critic.py:145-146).  Afterwards the wrapper's `features` and the
        env's scalars, reward and done show the last step.

        fused=None runs the call as one launch (wab_rollout_policy: the policy between the steps of
        the multi-step kernel, the features never leaving the chip unless they are stored) where
        wab_rollout_policy_fused says so and store_planes is False (store_planes=True writes each
        step into the env's single obs buffer, which the launch's [T][B] layout does not express);
        otherwise as the loop of wab_policy_act + wab_step_features, two launches per step.  Both
        give the same bits (with T > 128 the returns of the one-launch path are made by
        discounted_returns after it, as in the loop).  fused=False forces the loop; fused=True
        raises NotImplementedError where the one launch does not apply.  store_features=False
        stores no intermediate feature rows (the loop then alternates between two rows).
        store_features="packed" stores them as 1 bit per feature (wab_gym_amd.features): the result
        holds feature_bits [T,B,P] int32, which DevicePolicy's evaluate and gradient calls take as
        they take features, with the same bits in every result, and features is None
        (wab_rollout_policy_packed in one launch; in the loop a wab_features_pack launch per step).

        bootstrap_value=True adds last_value [B] f32, the policy's value of the features the call
        leaves in the wrapper's `features` (one more wab_policy_act after the steps; its sampled
        actions go to the policy's own scratch `actions`, and the draw is a keyed function of
        (seed, env, episode, turn), so nothing is consumed), and returns is then
        discounted_returns(reward, done, bootstrap=last_value, env=env): an episode still open at
        step T - 1 continues with the critic's estimate instead of 0.  The scan then runs after
        the launch, as it does for T > 128; normalize=True normalises those returns.
        gae_lambda=l (needs bootstrap_value=True) adds advantage and target [T,B] f32 from
        gae(reward, done, value, last_value, gamma, l, env=env); whiten=True (needs gae_lambda)
        whitens advantage in place (whitened).  With T = 0 last_value is the value of the current
        features and the [0, B] outputs are empty.  The one launch and the loop feed the same
        kernels the same inputs: the new outputs have the same bits on both paths."""
        if gae_lambda is not None and not bootstrap_value:
            raise ValueError("gae_lambda needs bootstrap_value=True (the advantages of an open episode need "
                             "the value of the state after the last step)")
        if whiten and gae_lambda is None:
            raise ValueError("whiten=True whitens the advantages: pass gae_lambda")
        from .env import BatchedWolvesAndBushesEnv

        env = self.env
        if type(self) is not PragmaticObsWrapper or type(env) is not BatchedWolvesAndBushesEnv:
            raise NotImplementedError("rollout_policy() runs PragmaticObsWrapper over a plain "
                                      "BatchedWolvesAndBushesEnv (the egocentric observation is made per "
                                      "step(); for episode statistics put EpisodeMonitor around the "
                                      "wrapper, not under it)")
        if env._term is not None:
            raise NotImplementedError("rollout_policy() returns no terminal observations "
                                      "(return_terminal=True)")
        if not env._reset_once:
            raise RuntimeError("call reset() before rollout_policy()")
        if policy.env is not env or policy.in_features != self.feature_dim:
            raise ValueError("the policy was made for another env or feature length")
        t = env._torch
        T, B, F = int(T), env.num_envs, self.feature_dim
        if T < 0:
            raise ValueError("T must be >= 0")
        dev = env.device
        L = _lib.load()
        one_launch = fused is None or bool(fused)
        if one_launch:
            why = None
            if store_planes:
                why = "store_planes=True writes every step into the env's single obs buffer"
            elif int(L.wab_rollout_policy_fused(env._h, policy._p)) != 1:
                why = L.wab_last_error().decode(errors="replace") or "wab_rollout_policy_fused is 0"
            if why is not None:
                if fused:
                    raise NotImplementedError("rollout_policy(fused=True): " + why)
                one_launch = False
        packed = isinstance(store_features, str)
        if packed and store_features != "packed":
            raise ValueError("store_features must be True, False or 'packed', not %r" % (store_features,))
        feats = t.empty((T, B, F), dtype=t.float32, device=dev) if store_features and not packed else None
        bits = None
        if packed:
            from .features import bits_pitch

            bits = t.empty((T, B, bits_pitch(F)), dtype=t.int32, device=dev)
        actions = t.empty((T, B), dtype=t.int8, device=dev)
        value = t.empty((T, B), dtype=t.float32, device=dev)
        rew = t.empty((T, B), dtype=t.float32, device=dev)
        done = t.empty((T, B), dtype=t.uint8, device=dev)
        out = {"features": feats, "actions": actions, "reward": rew, "done": done, "value": value,
               "returns": t.empty((T, B), dtype=t.float32, device=dev)}
        if packed:
            out["feature_bits"] = bits
        probs = None
        if return_probs:
            probs = out["probs"] = t.empty((T, B, policy.n_actions), dtype=t.float32, device=dev)
        if normalize:
            out["normalized"] = t.empty((T, B), dtype=t.float32, device=dev)
        if bootstrap_value:
            out["last_value"] = t.empty((B,), dtype=t.float32, device=dev)
        if gae_lambda is not None:
            out["advantage"] = t.empty((T, B), dtype=t.float32, device=dev)
            out["target"] = t.empty((T, B), dtype=t.float32, device=dev)

        def finish(returns_made):
            """What follows the steps: the value of the state they left, the returns scan where
            the launch did not make it, the normalisation and the advantages."""
            if bootstrap_value:
                policy.act(self.features, value=out["last_value"])
            if T == 0:  # (empty outputs: nothing to scan)
                return out
            if not returns_made:
                discounted_returns(rew, done, gamma=gamma, bootstrap=out.get("last_value"), out=out["returns"],
                                   env=env)
            if normalize:
                normalized_returns(out["returns"], done, out=out["normalized"])
            if gae_lambda is not None:
                gae(rew, done, value, out["last_value"], gamma=gamma, lam=gae_lambda, env=env,
                    advantage=out["advantage"], target=out["target"])
                if whiten:
                    whitened(out["advantage"], out=out["advantage"])
            return out

        if T == 0:
            if not bootstrap_value:
                return out
            if env._planes_valid:
                self.observation()
            return finish(False)
        if env._planes_valid:
            self.observation()
        if feats is not None:
            feats[0].copy_(self.features)
        o = env._obs["struct"]
        if one_launch:
            scal = t.empty((3, T, B), dtype=t.uint8, device=dev)
            st = _lib.WabObs(None, scal[0].data_ptr(), scal[1].data_ptr(), scal[2].data_ptr())
            # (the launch's returns scan; longer segments, and returns that continue with
            # last_value, which exists only after the launch: the kernel of the loop)
            in_launch = T <= 128 and not bootstrap_value
            first = self.features if feats is None else feats
            call, name = (L.wab_rollout_policy_packed, "wab_rollout_policy_packed") if packed else \
                (L.wab_rollout_policy, "wab_rollout_policy")
            rows_out = bits if packed else feats
            _lib.check(call(env._h, policy._p, first.data_ptr(), T, ctypes.addressof(st),
                            actions.data_ptr(), value.data_ptr(),
                            None if probs is None else probs.data_ptr(), rew.data_ptr(),
                            done.data_ptr(), None if rows_out is None else rows_out.data_ptr(),
                            self.features.data_ptr(), float(gamma), None,
                            out["returns"].data_ptr() if in_launch else None, env._stream()), name)
            env._sync_last_step(scal[:, T - 1], rew[T - 1], done[T - 1])
            env._planes_valid = False
            return finish(in_launch)
        st = o if store_planes else _lib.WabObs(None, o.food_turns, o.role, o.status)
        direct = (B * F) % 4 == 0  # every step's feature slice is 16-byte aligned
        cur = self.features
        spare = None if feats is not None else t.empty_like(self.features)
        def pack_step(k, rows):  # (the loop's packed rows: one launch per step)
            if packed:
                _lib.check(L.wab_features_pack(rows.data_ptr(), B, F, bits[k].data_ptr(), None, env._stream()),
                           "wab_features_pack")

        pack_step(0, self.features)
        for k in range(T):
            src = cur if feats is None else feats[k]
            policy.act(src, out=actions[k], value=value[k], probs=None if probs is None else probs[k])
            if feats is None:
                nxt = spare if cur is self.features else self.features
            else:
                nxt = feats[k + 1] if direct and k + 1 < T else self.features
            _lib.check(L.wab_step_features(env._h, actions[k].data_ptr(), ctypes.addressof(st),
                                           rew[k].data_ptr(), done[k].data_ptr(), nxt.data_ptr(),
                                           env._stream()), "wab_step_features")
            if feats is not None and not direct and k + 1 < T:
                feats[k + 1].copy_(self.features)
            if k + 1 < T:
                pack_step(k + 1, nxt)
            cur = nxt
        if feats is None and cur is not self.features:
            self.features.copy_(cur)
        env.reward.copy_(rew[T - 1])
        env.done.copy_(done[T - 1])
        env._planes_valid = bool(store_planes)
        return finish(False)

    def step(self, actions):
        if self.env._term is None and type(self) is PragmaticObsWrapper:
            # one kernel: the step and the features of its obs (wab_step_features)
            f, reward, done = self.env.step_features(actions, self.features)
            return f, reward, done, {}
        _, reward, done, info = self.env.step(actions)
        if "terminal_obs" in info:
            t = self.env._term
            info["terminal_features"] = self.observation(
                {"planes": t["planes"], "scalars": t["scalars"]},
                out=self.env._torch.empty_like(self.features))
        return self.observation(), reward, done, info


class SuperBasicObservationWrapper(PragmaticObsWrapper):
    """SuperBasicObservationWrapper (wab_env.py:900-927): (nearest bush, food, role, status),
    flattened by gym's rules (nearest bush 4 x Discrete(max_distance), :906)."""

    def __init__(self, env):
        self.env = env
        lib = _lib.load()
        self.feature_dim = int(lib.wab_superbasic_dim(env._h))
        opts = env.game_options
        self.max_distance = opts["width"] // 2 + opts["height"] // 2 + 1  # wab_env.py:903
        md = self.max_distance
        self.single_observation_space = Tuple((                          # wab_env.py:904-911
            Tuple([Discrete(md)] * 4), Discrete(opts["turns_to_empty_food"] + 1), Discrete(2), Discrete(3)))
        self.observation_space = Box(0.0, 1.0, (env.num_envs, self.feature_dim), dtype="float32")
        self.action_space = env.action_space
        self.spec = env.spec
        t = env._torch
        self.features = t.zeros((env.num_envs, self.feature_dim), dtype=t.float32, device=env.device)

    def observation(self, obs=None, view_mask=None, out=None):
        """Features of the env's current observation buffer (or of `obs`, as in
        PragmaticObsWrapper.observation; the view mask is not part of this wrapper)."""
        env = self.env
        if obs is None:
            env._require_planes()
            st = env._obs["struct"]
            keep = None
        else:
            st, keep = env._obs_struct(obs)
        dst = self.features if out is None else out
        env._check_features(dst, self.feature_dim)
        _lib.check(_lib.load().wab_featurize_superbasic(env._h, ctypes.addressof(st), dst.data_ptr(),
                                                        env._stream()), "wab_featurize_superbasic")
        del keep
        return dst


def discounted_returns(reward, done, gamma=0.99, bootstrap=None, out=None, env=None):
    """R_t = r_t + gamma * R_{t+1}, restarted after each done (actor_critic.py:139-143),
    over [T, B] device tensors; one HIP kernel, double accumulation, float32 out.  With `env`
    (the env whose steps returned `reward`) each float32 reward is first mapped back to the
    exact double the reference's step() returns, so the result is float32 of finish_episode's
    own double returns bit for bit (wab_discounted_returns_exact)."""
    import torch

    r = reward.to(torch.float32).contiguous()
    d = done.to(torch.uint8).contiguous()
    T, B = r.shape
    if d.shape != (T, B):
        raise ValueError("done must have the shape of reward [T, B]")
    o = torch.empty_like(r) if out is None else out
    if o.shape != (T, B) or o.dtype != torch.float32 or not o.is_contiguous():
        raise ValueError("out must be a contiguous float32 tensor of shape [T, B]")
    bs = None if bootstrap is None else bootstrap.to(torch.float32).contiguous()
    stream = ctypes.c_void_p(torch.cuda.current_stream(r.device).cuda_stream)
    L = _lib.load()
    args = (r.data_ptr(), d.data_ptr(), T, B, float(gamma), None if bs is None else bs.data_ptr(), o.data_ptr(),
            stream)
    if env is not None:
        if r.device != env.device:
            raise ValueError("reward is on %s, the env on %s" % (r.device, env.device))
        try:
            _lib.check(L.wab_discounted_returns_exact(env._h, *args), "wab_discounted_returns_exact")
            return o
        except ValueError as e:
            if "round to the same" not in str(e):
                raise
            # two of the options' rewards are one float32: the doubles are not recoverable
            warnings.warn("discounted_returns(env=...): %s; using the float32 rewards" % e)
    _lib.check(L.wab_discounted_returns(*args), "wab_discounted_returns")
    return o


def normalize_episode_returns(returns, done, eps=1.1920928955078125e-07):
    """(R - mean) / (std + eps) per episode segment of every env, as finish_episode does per
    episode (actor_critic.py:145-146; torch.std is unbiased; eps = float32 machine eps).
    Segments still open at the end of the rollout are normalised as they stand.  Two-pass
    segment statistics with scatter_add (trainer-side plumbing, not the env hot path)."""
    import torch

    T, B = returns.shape
    d = done.to(torch.int64)
    seg = torch.cumsum(d, 0) - d                           # dones strictly before t
    key = (torch.arange(B, device=returns.device).unsqueeze(0) * (T + 1) + seg).flatten()
    x = returns.to(torch.float64).flatten()
    n = torch.zeros(B * (T + 1), dtype=torch.float64, device=returns.device)
    cnt = n.clone().scatter_add_(0, key, torch.ones_like(x))
    mean = n.clone().scatter_add_(0, key, x) / cnt.clamp(min=1)
    dev = x - mean[key]
    var = n.clone().scatter_add_(0, key, dev * dev) / (cnt - 1)
    std = torch.sqrt(var)[key]
    return ((x - mean[key]) / (std + eps)).to(returns.dtype).reshape(T, B)


def normalized_returns(returns, done, eps=1.1920928955078125e-07, out=None):
    """normalize_episode_returns as one HIP kernel (wab_normalize_episode_returns): (R - mean) /
    (std + eps) per episode segment of every env's column of the [T, B] returns, a segment still
    open at the last step normalised as it stands, a one-step segment NaN (torch.std of one
    element).  Per segment the sum, the squared deviations and the division run in float64 in
    step order, so the result does not vary from run to run; float32 out (`out`, which may be
    `returns` itself, or a new tensor).  CPU tensors take normalize_episode_returns."""
    import torch

    if returns.dim() != 2 or tuple(done.shape) != tuple(returns.shape):
        raise ValueError("returns and done must have one shape [T, B]")
    if returns.device != done.device:
        raise ValueError("returns is on %s, done on %s" % (returns.device, done.device))
    T, B = returns.shape
    if out is not None and (tuple(out.shape) != (T, B) or out.dtype != torch.float32 or not out.is_contiguous()
                            or out.device != returns.device):
        raise ValueError("out must be a contiguous float32 tensor of shape [T, B] on the device of returns")
    if returns.device.type != "cuda":
        res = normalize_episode_returns(returns, done, eps=eps)
        if out is None:
            return res
        out.copy_(res)
        return out
    x = returns.to(torch.float32).contiguous()
    d = (done.view(torch.uint8) if done.dtype == torch.bool else done.to(torch.uint8)).contiguous()
    o = torch.empty_like(x) if out is None else out
    with torch.cuda.device(x.device):
        stream = ctypes.c_void_p(torch.cuda.current_stream(x.device).cuda_stream)
        _lib.check(_lib.load().wab_normalize_episode_returns(x.data_ptr(), d.data_ptr(), T, B, float(eps),
                                                             o.data_ptr(), stream), "wab_normalize_episode_returns")
    return o


def _exact_rewards(reward, env):
    """float64 rewards of the float32 `reward` (a CPU tensor): with `env`, each float32 that is one
    of the options' step rewards (0 + r_x or 0 + r_eat + r_x, wab_env.py:251-340) becomes that
    double, as wab_discounted_returns_exact maps it; other floats, and all of them without `env`
    or when two of the rewards round to one float32 (with a warning), convert as they are."""
    import numpy as np
    import torch

    r64 = reward.to(torch.float64)
    if env is None:
        return r64
    o = env.game_options
    rx = [o[k] for k in ("reward_per_turn", "reward_for_finishing", "reward_for_starving", "reward_for_being_killed")]
    table = {}
    for v in [0 + r for r in rx] + [0 + o["reward_for_eating"] + r for r in rx]:
        v = float(v)
        if table.setdefault(int(np.float32(v).view(np.int32)), v) != v:
            warnings.warn("gae(env=...): two of the options' rewards round to the same float32; using the "
                          "float32 rewards")
            return r64
    bits = reward.contiguous().view(torch.int32)
    for b, v in table.items():
        r64 = torch.where(bits == b, torch.full((), v, dtype=torch.float64), r64)
    return r64


def gae(reward, done, value, last_value=None, gamma=0.99, lam=0.95, env=None, advantage=None, target=None):
    """Generalised advantage estimation over the [T, B] reward, done and value of a rollout
    segment: (advantage, target), both float32 [T, B].  Per env, in float64, from t = T - 1 down:
    delta = (r + (done ? 0 : gamma * v_next)) - v, A = delta + (done ? 0 : gamma * lam * A),
    advantage = float32(A), target = float32(A + v), v_next starting at last_value [B] (None = 0),
    the critic's value of the state after the last step (wab_gae, include/wab.h: the contract in
    full).  One HIP kernel for device tensors.  With `env` (the env whose steps returned `reward`)
    each float32 reward is first mapped back to the exact double the reference's step() returns, as
    discounted_returns(env=...) does, with the same fallback and warning where the options make
    that ambiguous.  `advantage` and `target` may be given (contiguous float32 [T, B], not
    overlapping an input).  CPU tensors take the same arithmetic in torch."""
    import torch

    if reward.dim() != 2 or tuple(done.shape) != tuple(reward.shape) or tuple(value.shape) != tuple(reward.shape):
        raise ValueError("reward, done and value must have one shape [T, B]")
    T, B = reward.shape
    dev = reward.device
    if last_value is not None and tuple(last_value.shape) != (B,):
        raise ValueError("last_value must have the shape [B]")
    for name, x in (("done", done), ("value", value), ("last_value", last_value), ("advantage", advantage),
                    ("target", target)):
        if x is not None and x.device != dev:
            raise ValueError("%s is on %s, reward on %s" % (name, x.device, dev))
    for name, x in (("advantage", advantage), ("target", target)):
        if x is not None and (tuple(x.shape) != (T, B) or x.dtype != torch.float32 or not x.is_contiguous()):
            raise ValueError("%s must be a contiguous float32 tensor of shape [T, B]" % name)
    r = reward.to(torch.float32).contiguous()
    d = (done.view(torch.uint8) if done.dtype == torch.bool else done.to(torch.uint8)).contiguous()
    v = value.to(torch.float32).contiguous()
    lv = None if last_value is None else last_value.to(torch.float32).contiguous()
    adv = torch.empty_like(r) if advantage is None else advantage
    tgt = torch.empty_like(r) if target is None else target
    if dev.type != "cuda":
        r64, v64 = _exact_rewards(r, env), v.to(torch.float64)
        zero = torch.zeros((), dtype=torch.float64)
        gl = float(gamma) * float(lam)
        A = torch.zeros(B, dtype=torch.float64)
        vnext = A.clone() if lv is None else lv.to(torch.float64)
        for k in range(T - 1, -1, -1):
            dk = d[k] != 0
            delta = (r64[k] + torch.where(dk, zero, float(gamma) * vnext)) - v64[k]
            A = delta + torch.where(dk, zero, gl * A)
            adv[k] = A.to(torch.float32)
            tgt[k] = (A + v64[k]).to(torch.float32)
            vnext = v64[k]
        return adv, tgt
    if env is not None and dev != env.device:
        raise ValueError("reward is on %s, the env on %s" % (dev, env.device))
    if T == 0 or B == 0:
        return adv, tgt
    L = _lib.load()
    with torch.cuda.device(dev):
        stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        args = (r.data_ptr(), d.data_ptr(), v.data_ptr(), None if lv is None else lv.data_ptr(), T, B, float(gamma),
                float(lam), adv.data_ptr(), tgt.data_ptr(), stream)
        if env is not None:
            try:
                _lib.check(L.wab_gae(env._h, *args), "wab_gae")
                return adv, tgt
            except ValueError as e:
                if "round to the same" not in str(e):
                    raise
                # two of the options' rewards are one float32: the doubles are not recoverable
                warnings.warn("gae(env=...): %s; using the float32 rewards" % e)
        _lib.check(L.wab_gae(None, *args), "wab_gae")
    return adv, tgt


_whiten_workspaces = {}


def whitened(x, eps=1.1920928955078125e-07, out=None):
    """(x - mean) / (std + eps) over all elements of a contiguous float32 tensor, the usual
    normalisation of a batch of advantages (wab_whiten): std unbiased as torch.std, everything in
    float64, float32 out (`out`, which may be `x` itself, or a new tensor); one element gives NaN.
    The sums run in a fixed order, so two runs on one input give the same bits, and the call can
    be captured in a graph (its workspace is kept per device; a call made during a capture takes
    one from torch's allocator, which the capture owns).  CPU tensors take torch in float64."""
    import torch

    if x.dtype != torch.float32 or not x.is_contiguous():
        raise ValueError("x must be a contiguous float32 tensor")
    if out is not None and (tuple(out.shape) != tuple(x.shape) or out.dtype != torch.float32
                            or not out.is_contiguous() or out.device != x.device):
        raise ValueError("out must be a contiguous float32 tensor of the shape and on the device of x")
    o = torch.empty_like(x) if out is None else out
    n = x.numel()
    if x.device.type != "cuda":
        if n > 0:
            xd = x.to(torch.float64)
            dev = xd - xd.mean()
            var = (dev * dev).sum() / (n - 1) if n > 1 else torch.full((), float("nan"), dtype=torch.float64)
            o.copy_((dev / (torch.sqrt(var) + eps)).to(torch.float32))
        return o
    if n == 0:
        return o
    L = _lib.load()
    size = int(L.wab_whiten_workspace(n))
    if size < 0:
        _lib.check(-1, "wab_whiten_workspace")
    with torch.cuda.device(x.device):
        if torch.cuda.is_current_stream_capturing():
            ws = torch.empty(size // 8, dtype=torch.float64, device=x.device)
        else:
            key = (x.device.index, size)
            ws = _whiten_workspaces.get(key)
            if ws is None:
                ws = _whiten_workspaces[key] = torch.empty(size // 8, dtype=torch.float64, device=x.device)
        stream = ctypes.c_void_p(torch.cuda.current_stream(x.device).cuda_stream)
        _lib.check(L.wab_whiten(x.data_ptr(), n, float(eps), o.data_ptr(), ws.data_ptr(), stream), "wab_whiten")
    return o
