"""The contract of wab_gae and a reference for wab_whiten, in numpy on the CPU, and the inputs
the advantage tests share (tests/test_gae_host.py, tests/test_gpu_gae.py,
tests/test_gpu_rollout_policy_gae.py).  The segments are those of tests/returns_cases.py with a
value column and a last value added."""
from __future__ import annotations

import math

import numpy as np

import returns_cases as rc
from test_featurizer_oracle import reward_table, step_reward_values



def exact_rewards(reward, opts=None, table=True):
    """float64 [T, B]: with `table` each float32 that is one of the option set's step rewards
    becomes that double (the table rule restated in tests/test_featurizer_oracle.py); every other
    float, and all of them without, converts as it is."""
    reward = np.asarray(reward, np.float32)
    r = reward.astype(np.float64)
    if table:
        bits = reward.view(np.uint32)
        for b, v in reward_table(opts):
            r[bits == np.uint32(b)] = v
    return r


def gae_reference(r64, done, value, last_value, gamma, lam):
    """The contract of wab_gae (include/wab.h), vectorised over B, one Python loop over t.
    r64 float64 [T, B] (exact_rewards), done u8, value f32 [T, B], last_value f32 [B] or None.
    Returns (advantage, target) float32 [T, B]."""
    T, B = r64.shape
    v64 = np.asarray(value, np.float32).astype(np.float64)
    gamma, lam = float(gamma), float(lam)
    gl = gamma * lam
    A = np.zeros(B, np.float64)
    vnext = np.zeros(B, np.float64) if last_value is None else np.asarray(last_value, np.float32).astype(np.float64)
    adv = np.empty((T, B), np.float32)
    tgt = np.empty((T, B), np.float32)
    with np.errstate(all="ignore"):
        for t in range(T - 1, -1, -1):
            d = done[t] != 0
            v = v64[t]
            delta = (r64[t] + np.where(d, 0.0, gamma * vnext)) - v
            A = delta + np.where(d, 0.0, gl * A)
            adv[t] = A.astype(np.float32)
            tgt[t] = (A + v).astype(np.float32)
            vnext = v
    return adv, tgt


def returns_reference(r64, done, bootstrap, gamma):
    """The existing scan's bootstrapped returns in float64 (R = d ? 0 : R; R = r + gamma R),
    unrounded: float64 [T, B]."""
    T, B = r64.shape
    R = np.zeros(B, np.float64) if bootstrap is None else np.asarray(bootstrap, np.float32).astype(np.float64)
    out = np.empty((T, B), np.float64)
    with np.errstate(all="ignore"):
        for t in range(T - 1, -1, -1):
            R = np.where(done[t] != 0, 0.0, R)
            R = r64[t] + float(gamma) * R
            out[t] = R
    return out


def whiten_reference(x, eps=1.1920928955078125e-07):
    """(x - mean) / (std + eps), std unbiased: the two sums exact (math.fsum), the rest float64;
    float32 out.  One element gives NaN."""
    x = np.asarray(x, np.float32)
    x64 = x.astype(np.float64).ravel()
    n = x64.size
    mean = math.fsum(x64.tolist()) / n
    dev = x64 - mean
    ss = math.fsum((dev * dev).tolist())
    with np.errstate(all="ignore"):
        var = np.float64(ss) / np.float64(n - 1)
        return (dev / (np.sqrt(var) + eps)).astype(np.float32).reshape(x.shape)


def make_gae_case(T, B, name="defaults", seed=0, scale=4.0):
    """(reward, done, value [T, B] f32, last_value [B] f32, options): returns_cases.make_case of
    the option set `name` with its bootstrap as last_value, and a value column of float32 normals
    of the given scale that holds -0.0 (about one entry in sixteen) and, for B >= 12, one column
    of infinities (column 6: +inf at even steps, -inf at odd ones, so both an inf - inf NaN and
    its stop at the next done are exercised)."""
    opts = rc.options_of(name)
    reward, done, last = rc.make_case(T, B, step_reward_values(opts), seed=seed)
    rng = np.random.RandomState(77 + 13 * seed + T)
    value = (rng.standard_normal((T, B)) * scale).astype(np.float32)
    value[rng.randint(0, 16, size=(T, B)) == 0] = np.float32(-0.0)
    last = (last * np.float32(scale)).astype(np.float32)
    if B >= 12:
        value[0::2, 6] = np.inf
        value[1::2, 6] = -np.inf
        last[7] = np.float32(-0.0)
    return reward, done, value, last, opts


def make_whiten_input(n, seed=0, mean=3.0, std=0.5):
    """float32 normals with |mean| <= 10 std."""
    assert abs(mean) <= 10 * std
    rng = np.random.RandomState(4000 + seed + n % 1000)
    return (rng.standard_normal(n) * std + mean).astype(np.float32)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits(got, want):
    """Equal float32 bits, any NaN standing for any other (a NaN's payload is not part of the
    contract)."""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(bits(got)[~nan], bits(want)[~nan])


def finite_columns(value, last):
    return np.isfinite(value).all(0) & np.isfinite(last)


def check_lambda_one(target, returns32, r_abs_max, value, last, cols):
    """Identity 3: |target - returns| <= one float32 ulp of M per column, M the largest of |R|,
    |value| and |last_value| there (absolute: A + v cancels near zero); at most 1 % of the entries
    differ at all.  Returns (differing share, worst error / bound) for the record."""
    M = np.maximum(np.maximum(r_abs_max, np.abs(value).max(0)), np.abs(last)).astype(np.float32)
    bound = np.spacing(M[cols]).astype(np.float64)
    err = np.abs(target[:, cols].astype(np.float64) - returns32[:, cols].astype(np.float64))
    differ = float((bits(target[:, cols]) != bits(returns32[:, cols])).mean())
    worst = float((err / bound[None]).max())
    assert (err <= bound[None]).all(), worst
    assert differ <= 0.01, differ
    return differ, worst
