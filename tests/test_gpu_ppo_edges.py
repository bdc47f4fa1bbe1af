"""wab_policy_grad_ppo and wab_policy_evaluate on the GPU where include/wab.h states what the head
does and tests/test_gpu_ppo.py stays clear of it: the ties of the strict comparisons, the +-30
clamp, NaN rows, bad actions under PPO, and calls with two or more row blocks in every slab.

Nothing here has a tolerance on a decision.  The head's decisions are float32 functions of values
the kernel returns (logp, value, ratio), which tests/test_gpu_ppo.py holds to the contract.  The
rows are built at run time from those bits so that they sit on the ties (tests/ppo_cases.py:
tie_old_logp, tie_advantages, tie_value_rows), ppc.predict_head repeats the head on the host with
the same float32 operations, and the tests assert the counts exactly and the gradients bit for bit
through the effective-weight identity (test 3 of tests/test_gpu_ppo.py): a PPO step is
loss_and_grad's of weight = w_eff and target = value where the value loss is clipped.

The float sums (loss_policy, loss_value, the k3 sum and the ratio sum) are held to one unit in the
last place of the float32 rounding of the predictor's float64 sum.  That is derived, not
measured: the device adds at most 257 float32 terms (k3: doubles) in double and rounds once; the
double sums of the two orders differ by less than 257 * 2^-53 of the sum of magnitudes, which
moves the float32 rounding to its neighbour at the most while the sum is not cancelled below
2^-16 of the sum of magnitudes (asserted, a condition on the inputs).

1. ties of the policy clip: old_logp = fl32(logp - ln 1.25) (and ln 0.75) moved -4 .. 4 units,
   the clip chosen from the returned ratios so that fl32(1.0f +- clip) is one of them; advantages
   of both signs and both zeros;
2. ties of the value term: |u| <, ==, > c for c = 0.25 and fl32(0.2), targets at the float32
   midpoint of value and vc (l2 == l1) and 1 away from value and vc (smooth_l1's kink);
3. the clamp (logp -+ 31, -+ 1000, -+inf and a mix are one result; -+ 29.5 is another), a NaN
   old_logp and a NaN advantage (the row's own outputs, the sums, DeviceAdam's skip, the next
   clean call), bad actions in three blocks;
4. N with two or more row blocks in every slab: evaluate's one-pass grid, ratio 1, mixed rows,
   chunk_rows at and past S, and what a big call leaves behind for a small and an empty one.

expf.  The clamped ratio is compared with exp(+-30) in float64 under HIP's documented bound for
expf, 1 ULP ("HIP math API", single precision mathematical functions table, the row expf, of the
HIP documentation of ROCm 7: "Maximum ULP difference 1" against the correctly rounded result).
A ROCm installation carries no copy of that table (its share/doc has licences and API headers,
no accuracy figures), so the number is quoted from the public document, not read from a file.
The test allows that 1 unit from fl32(exp(+-30)), exp in float64.

Measured on an MI355X (first run; DESIGN.md, "wab_policy_grad_ppo", has the same figures), rows
at (<, ==, >) of each tie, N = 257:

  r vs hi (the median ratio was 1.25 itself, clip 0.25; 18 distinct ratios ref, 21 odd)
      ref: A > 0 (46, 11, 46)   A < 0 (46, 10, 47)   A == 0 (23, 5, 23)
      odd: A > 0 (46, 11, 46)   A < 0 (45, 11, 47)   A == 0 (23, 5, 23)
  r vs lo (0.75, clip 0.25; 9 distinct ratios ref, 18 odd)
      ref and odd: A > 0 (45, 12, 46)   A < 0 (45, 11, 47)   A == 0 (22, 6, 23)
  value term, the same for smooth_l1 and mse  |u| vs c     l2 vs l1      |v - t| vs 1    |vc - t| vs 1
      ref, c = 0.25                           (46, 126, 85)  (15, 47, 23)  (157, 25, 75)   (70, 12, 3)
      odd, c = 0.25                           (85, 65, 107)  (25, 47, 35)  (163, 18, 76)   (89, 15, 3)
      ref, c = fl32(0.2)                      (59, 97, 101)  (37, 21, 43)  (159, 23, 75)   (85, 12, 4)
      odd, c = fl32(0.2)                      (98, 26, 133)  (22, 79, 32)  (169, 24, 64)   (112, 17, 4)
  the clamped ratio: 10686474223616.0 and 9.357622912219837e-14 on both nets, 0 units from
      fl32(exp(30)) and fl32(exp(-30))
  test 4: of the 15233 (ref) and 16513 ((17, 33, 33, 33, 5)) mixed rows none was within 2^-10 of a
      decision.

Two of the relations asked of these tests cannot hold as first written, and are stated as what
does hold.  With ratio 1 the PPO step's loss_policy is -sum(A), not the A2C step's -sum(A logp),
and the total follows it: the gradients, loss_value, entropy and the rows are the A2C step's bit
for bit, loss_policy is held to its own exact value.  A bad-action row is left out of the entropy
sum, a valid row of A = 0 is not: the comparison run's entropy sum loses those rows' H on the
host, to one unit, like its k3 and ratio sums; and those rows take old_value = value as well, so
that the value clip gives them neither a loss nor a count."""
import numpy as np
import pytest
import torch

import policy_grad_cases as pgc
import ppo_cases as ppc
import test_gpu_ppo as tp
from test_gpu_ppo import DEV, cpu, dev, same, same_grads
from wab_gym_amd import policy

pytestmark = pytest.mark.gpu
F32 = np.float32
SUMS = ("loss_policy", "loss_value", "entropy", "loss", "ppo_sums")
ROWS_OUT = ("logp", "value", "entropy_rows", "ratio")
EXPF_ULP = 1  # HIP math API, expf: maximum ULP difference 1 (see the docstring)
BIG_NETS = ("ref", (17, 33, 33, 33, 5))


def inputs(net, n):
    a, w, t = pgc.rows(net, n)
    return {"x": pgc.features(net, n), "a": a, "adv": w, "t": t}


def evaluate(pol, c):
    ev = cpu(pol.evaluate(dev(c["x"], torch.float32), dev(c["a"], torch.int8)))
    pol.check()
    return {k: v.numpy() for k, v in ev.items()}


def run_ppo(pol, c, check=True, **kw):
    """ppo_loss_and_grad on host arrays (c: x, a, adv, t, old_logp and, with value_clip, old_value)."""
    ov = c.get("old_value")
    r = pol.ppo_loss_and_grad(dev(c["x"], torch.float32), dev(c["a"], torch.int8), dev(c["adv"], torch.float32),
                              dev(c["t"], torch.float32), dev(c["old_logp"], torch.float32),
                              old_value=None if ov is None else dev(ov, torch.float32), return_rows=True, **kw)
    if check:
        pol.check()
    return cpu(r)


def first_difference(r1, r2, rows=True):
    """The first of the ten gradients, the eight sums and the four row outputs that differs."""
    for k in same_grads(r1["grads"], r2["grads"]):
        return k
    for k in SUMS + (ROWS_OUT if rows else ()):
        if not same(r1[k], r2[k]):
            return k
    return None


def predicted(got, c, clip, value_clip, value_loss):
    return ppc.predict_head(got["logp"].numpy(), got["value"].numpy(), got["ratio"].numpy(), c["adv"], c["t"],
                            c["old_logp"], c.get("old_value"), clip, value_clip, value_loss)


def assert_effective_weight_case(pol, got, c, p, **kw):
    """The gradients are loss_and_grad's of weight = the predicted w_eff and target = value where
    the predictor finds the value loss clipped, bit for bit."""
    t2 = np.where(p["value_clipped"], got["value"].numpy(), c["t"]).astype(np.float32)
    a2c = tp.run_a2c(pol, c["x"], c["a"], p["w_eff"], t2, **kw)
    assert not same_grads(got["grads"], a2c["grads"]), (kw, same_grads(got["grads"], a2c["grads"]))


def assert_float_sums(got, p, rows=None):
    """Each float sum within one unit in the last place of fl32(the predictor's float64 sum)."""
    keep = slice(None) if rows is None else rows
    terms = {"loss_policy": p["lpol"], "loss_value": p["lv"], 1: p["k3"], 3: got["ratio"].numpy()}
    for k, term in terms.items():
        t64 = term[keep].astype(np.float64)
        want, mag = float(t64.sum()), float(np.abs(t64).sum())
        assert abs(want) >= 2.0 ** -16 * mag, ("the rows cancel: the one-unit bound does not apply", k, want, mag)
        have = float(got[k]) if isinstance(k, str) else float(got["ppo_sums"][k])
        assert ppc.units_apart(have, want) <= 1, (k, have, want)


def assert_counts(got, p):
    assert got["ppo_sums"][0] == float(p["n_clipped"]) and got["ppo_sums"][2] == float(p["n_value_clipped"]), \
        (got["ppo_sums"].tolist(), p["n_clipped"], p["n_value_clipped"])


# ------------------------------------------------------------------ 1. ties of the policy clip
@pytest.mark.parametrize("net", ("ref", "odd"))
@pytest.mark.parametrize("side", ("hi", "lo"))
def test_policy_clip_ties(net, side):
    n, upper = 257, side == "hi"
    pol = tp.policy_for(net)
    c = inputs(net, n)
    ev = evaluate(pol, c)
    c["old_logp"] = ppc.tie_old_logp(ev["logp"], 1.25 if upper else 0.75)
    ratio = run_ppo(pol, c, clip=0.5)["ratio"].numpy()  # (the ratio does not depend on clip or advantage)
    c["adv"] = ppc.tie_advantages(ratio)
    assert np.signbit(c["adv"][c["adv"] == 0]).any() and not np.signbit(c["adv"][c["adv"] == 0]).all()
    bound = ppc.tie_bound(ratio, c["adv"], upper)
    clip = ppc.clip_for_bound(bound, upper)
    assert (F32(1.0) + F32(clip) if upper else F32(1.0) - F32(clip)) == bound
    met = [ppc.groups(ratio[rows], bound) for rows in (c["adv"] > 0, c["adv"] < 0, c["adv"] == 0)]
    print("%s r vs %s = %r (clip %r), %d distinct ratios: rows <, ==, > of A > 0 %s, A < 0 %s, A == 0 %s"
          % (net, side, float(bound), clip, len(np.unique(ratio)), met[0], met[1], met[2]))
    assert all(min(g) >= 1 for g in met), met  # (a condition on the inputs)
    runs = {}
    for value_loss in ("smooth_l1", "mse"):
        for chunk_rows in (0, 128):
            kw = dict(value_coef=0.5, entropy_coef=0.01, value_loss=value_loss, chunk_rows=chunk_rows)
            got = runs[value_loss, chunk_rows] = run_ppo(pol, c, clip=clip, **kw)
            assert same(got["ratio"], torch.as_tensor(ratio))
            p = predicted(got, c, clip, None, value_loss)
            # the strict side: a row at the bound is not clipped, whatever its advantage
            at = ratio == bound
            assert not p["clipped"][at].any() and p["clipped"][~at].any() and p["n_value_clipped"] == 0
            assert_counts(got, p)
            assert_effective_weight_case(pol, got, c, p, **kw)
            assert_float_sums(got, p)
        assert first_difference(runs[value_loss, 0], runs[value_loss, 128]) is None
    pol.close()


# ------------------------------------------------------------------ 2. ties of the value term
@pytest.mark.parametrize("net", ("ref", "odd"))
@pytest.mark.parametrize("value_clip", (0.25, 0.2))
def test_value_clip_ties(net, value_clip):
    n = 257
    pol = tp.policy_for(net)
    c = inputs(net, n)
    ev = evaluate(pol, c)
    c["old_logp"] = ppc.tie_old_logp(ev["logp"], 1.25)  # (near the policy bound as well, clip fixed)
    target = c["t"]
    for value_loss in ("smooth_l1", "mse"):
        c["old_value"], c["t"], info = ppc.tie_value_rows(ev["value"], target, value_clip, value_loss)
        runs = {}
        for chunk_rows in (0, 128):
            kw = dict(value_coef=0.5, entropy_coef=0.01, value_loss=value_loss, chunk_rows=chunk_rows)
            got = runs[chunk_rows] = run_ppo(pol, c, clip=ppc.CLIP, value_clip=value_clip, **kw)
            assert same(got["value"], torch.as_tensor(ev["value"])) and same(got["logp"], torch.as_tensor(ev["logp"]))
            p = predicted(got, c, ppc.CLIP, value_clip, value_loss)
            out = p["outside"]
            u_met = info["u"]
            l_met = ppc.groups(p["l2"][out], p["l1"][out])
            vc = c["old_value"] + np.where(ev["value"] - c["old_value"] > 0, F32(value_clip), -F32(value_clip))
            k_met = (ppc.groups(np.abs(ev["value"] - c["t"]), F32(1.0)), ppc.groups(np.abs(vc - c["t"])[out], F32(1.0)))
            if chunk_rows == 0:
                print("%s c = %r %s: rows <, ==, > of |u| vs c %s, l2 vs l1 %s, |v - t| vs 1 %s, |vc - t| vs 1 %s"
                      % (net, float(F32(value_clip)), value_loss, u_met, l_met, k_met[0], k_met[1]))
            # conditions on the inputs: every group of every tie is met, l2 == l1 by 8 rows or more
            assert min(u_met) >= 8 and u_met[2] == out.sum() and min(l_met) >= 8, (u_met, l_met)
            assert min(k_met[0]) >= 1 and min(k_met[1]) >= 1, k_met
            # the strict side: l2 == l1 is not clipped, |u| == c is inside
            assert not p["value_clipped"][out & (p["l1"] == p["l2"])].any() and p["n_value_clipped"] == l_met[2]
            assert_counts(got, p)
            assert_effective_weight_case(pol, got, c, p, **kw)
            assert_float_sums(got, p)
        assert first_difference(runs[0], runs[128]) is None
    pol.close()


# ------------------------------------------------------------------ 3. clamp, NaN, bad actions
def test_the_clamp_at_30():
    """d beyond +-30 is cut to +-30 by comparisons, whatever lies beyond: every output of the call
    is one set of bits for logp -+ 31, -+ 1000, -+inf and a mix of them per row."""
    n = 257
    for net in ("ref", "odd"):
        pol = tp.policy_for(net)
        c = inputs(net, n)
        c["adv"] = np.where(c["adv"] == 0, F32(0.5), c["adv"]).astype(np.float32)  # both signs
        assert (c["adv"] > 0).sum() >= 64 and (c["adv"] < 0).sum() >= 64
        logp = evaluate(pol, c)["logp"]
        kw = dict(value_coef=0.5, entropy_coef=0.01)
        for sign, exact in ((-1.0, np.exp(30.0)), (1.0, np.exp(-30.0))):  # old_logp below logp: d = +30
            beyond = [(logp + F32(sign * 31.0)).astype(np.float32), (logp + F32(sign * 1000.0)).astype(np.float32),
                      np.full(n, sign * np.inf, np.float32)]
            beyond.append(np.choose(np.arange(n) % 3, beyond))
            runs = []
            for old in beyond:
                c["old_logp"] = old
                runs.append(run_ppo(pol, c, clip=ppc.CLIP, **kw))
            for other in runs[1:]:
                assert first_difference(runs[0], other) is None, first_difference(runs[0], other)
            got = runs[0]
            r = got["ratio"].numpy()
            assert len(np.unique(r)) == 1
            away = int(ppc.units_apart(r[0], exact))
            print("%s: the clamped ratio %r is %d units from fl32(exp(%d)) = %r"
                  % (net, float(r[0]), away, -30 * sign, float(F32(exact))))
            assert away <= EXPF_ULP
            # not clamped at 29.5
            c["old_logp"] = (logp + F32(sign * 29.5)).astype(np.float32)
            inside = run_ppo(pol, c, clip=ppc.CLIP, **kw)
            assert bool((inside["ratio"] != got["ratio"][0]).all())
            assert bool(((inside["ratio"] < got["ratio"][0]) if sign < 0 else (inside["ratio"] > got["ratio"][0])).all())
            # the step itself: rows with A < 0 at r = e^30 are not clipped and weigh about 1e13 A
            c["old_logp"] = beyond[3]
            p = predicted(got, c, ppc.CLIP, None, "smooth_l1")
            assert bool((p["d"] == F32(-30.0 * sign)).all())
            assert np.array_equal(p["clipped"], c["adv"] > 0 if sign < 0 else c["adv"] < 0)
            if sign < 0:
                assert np.abs(p["w_eff"]).max() > 1e13
            assert_counts(got, p)
            assert_effective_weight_case(pol, got, c, p, **kw)
            for k in pgc.GRAD_NAMES:
                assert bool(torch.isfinite(got["grads"][k]).all()), k
            assert all(bool(torch.isfinite(got[k]).all()) for k in SUMS + ROWS_OUT)
        pol.close()


@pytest.mark.parametrize("what", ("old_logp", "advantage"))
def test_a_nan_row(what):
    """A NaN stays a NaN: it reaches the row's ratio (old_logp), loss_policy and the gradients, is
    counted as not clipped, touches no other row, makes DeviceAdam skip, and is gone with the
    next call."""
    n, row = 129, 128  # the row is the second block's
    _, model = tp.model_of(seed=2)
    pol = policy.DevicePolicy(model, tp.env_for(5, 128))
    opt = policy.DeviceAdam(pol, model, lr=1e-2, max_grad_norm=0.5)
    c = inputs("ref", n)
    ev = evaluate(pol, c)
    c["old_logp"] = (ev["logp"] + np.resize(np.array(ppc.DELTAS, np.float32), n)).astype(np.float32)
    c["old_value"] = (ev["value"] + np.resize(np.array(ppc.EPSILONS, np.float32), n)).astype(np.float32)
    c["adv"] = c["adv"].copy()
    c["adv"][row] = 2.0
    c["old_logp"][row] = ev["logp"][row] - F32(0.5)  # r = e^0.5, A > 0: clipped in the clean run
    kw = dict(clip=ppc.CLIP, value_clip=ppc.VALUE_CLIP, value_coef=0.5, entropy_coef=0.01)
    clean = run_ppo(pol, c, **kw)
    pc_ = predicted(clean, c, ppc.CLIP, ppc.VALUE_CLIP, "smooth_l1")
    assert pc_["clipped"][row] and all(bool(torch.isfinite(clean[k]).all()) for k in SUMS)
    assert_counts(clean, pc_)
    bad = dict(c)
    key = "old_logp" if what == "old_logp" else "adv"
    bad[key] = c[key].copy()
    bad[key][row] = np.nan
    got = run_ppo(pol, bad, **kw)
    p = predicted(got, bad, ppc.CLIP, ppc.VALUE_CLIP, "smooth_l1")
    others = np.arange(n) != row
    for k in ROWS_OUT:
        assert np.array_equal(got[k].numpy()[others].view(np.int32), clean[k].numpy()[others].view(np.int32)), k
    for k in ("logp", "value", "entropy_rows"):
        assert same(got[k], clean[k]), k
    if what == "old_logp":
        assert np.isnan(float(got["ratio"][row]))
        assert np.isnan(float(got["ppo_sums"][1])) and np.isnan(float(got["ppo_sums"][3]))
    else:  # the ratio, k3 and their sums do not read the advantage
        assert same(got["ratio"], clean["ratio"])
        assert same(got["ppo_sums"][1], clean["ppo_sums"][1]) and same(got["ppo_sums"][3], clean["ppo_sums"][3])
    # no comparison with a NaN holds: the row is not clipped; the value term does not see it
    assert not p["clipped"][row]
    assert_counts(got, p)
    assert got["ppo_sums"][0] == clean["ppo_sums"][0] - 1 and got["ppo_sums"][2] == clean["ppo_sums"][2]
    assert np.isnan(float(got["loss_policy"])) and np.isnan(float(got["loss"]))
    assert same(got["loss_value"], clean["loss_value"]) and same(got["entropy"], clean["entropy"])
    assert bool(torch.isnan(got["grads"]["action_head.bias"]).any())
    # into=model and a step: skipped, nothing moves
    feats = dev(c["x"][:128], torch.float32)

    def act():
        probs, value = torch.empty((128, 5), device=DEV), torch.empty(128, device=DEV)
        actions = pol.act(feats, probs=probs, value=value).clone()
        return probs.cpu(), value.cpu(), actions.cpu()

    before_act = act()
    before = [q.detach().clone() for q in model.parameters()]
    out = pol.ppo_loss_and_grad(dev(bad["x"], torch.float32), dev(bad["a"], torch.int8), dev(bad["adv"], torch.float32),
                                dev(bad["t"], torch.float32), dev(bad["old_logp"], torch.float32),
                                old_value=dev(bad["old_value"], torch.float32), into=model, **kw)
    assert "grads" not in out and bool(torch.isnan(model.action_head.bias.grad).any())
    opt.step()
    pol.check()
    stats = opt.stats()
    assert stats["skipped"] == 1 and stats["step"] == 0, stats
    assert all(torch.equal(q.detach(), b) for q, b in zip(model.parameters(), before))
    assert all(not bool(m.any()) for m in opt.exp_avg + opt.exp_avg_sq)
    after_act = act()
    assert same(after_act[0], before_act[0]) and same(after_act[1], before_act[1])
    assert torch.equal(after_act[2], before_act[2])
    # the next clean call on the same workspace
    again = run_ppo(pol, c, **kw)
    assert first_difference(clean, again) is None, first_difference(clean, again)
    pol.close()


@pytest.mark.parametrize("net", ("ref", "odd"))
def test_bad_actions_under_ppo(net):
    """Rows whose action is out of range take no part: ratio and logp 0, none of the eight sums
    and no gradient sees them.  The comparison run gives those rows a valid action, A = 0, target
    = value and old_value = value (inside the value clip: no loss, no gradient, no count); its
    ratio sum and k3 sum, which count them, lose exactly those rows' terms on the host, and its
    entropy sum their H."""
    n = 257
    pol = tp.policy_for(net)
    c = inputs(net, n)
    ev = evaluate(pol, c)
    c["old_logp"] = (ev["logp"] + np.resize(np.array(ppc.DELTAS, np.float32), n)).astype(np.float32)
    c["old_value"] = (ev["value"] + np.resize(np.array(ppc.EPSILONS, np.float32), n)).astype(np.float32)
    rows = {5: 6, 128 + 77: -1, 256: 127}  # blocks 0, 1, 2
    bad, ok = dict(c), dict(c)
    for k in ("a", "adv", "t", "old_value"):
        bad[k], ok[k] = c[k].copy(), c[k].copy()
    for i, action in rows.items():
        bad["a"][i] = action
        bad["adv"][i] = 1.5  # (what the row would weigh if it took part)
        ok["adv"][i], ok["t"][i], ok["old_value"][i] = 0.0, ev["value"][i], ev["value"][i]
        bad["old_value"][i] = ok["old_value"][i]
    for i, delta in zip(sorted(rows), (-0.5, 0.0625, 0.5)):  # (every left-out row has r != 1 and k3 != 0)
        c["old_logp"][i] = ev["logp"][i] + F32(delta)
    bad["old_logp"] = ok["old_logp"] = c["old_logp"]
    idx = np.array(sorted(rows))
    others = np.setdiff1d(np.arange(n), idx)
    for chunk_rows in (0, 128):
        kw = dict(clip=ppc.CLIP, value_clip=ppc.VALUE_CLIP, value_coef=0.5, entropy_coef=0.0, chunk_rows=chunk_rows)
        want = run_ppo(pol, ok, **kw)
        got = run_ppo(pol, bad, check=False, **kw)
        with pytest.raises(IndexError, match="3 rows"):
            pol.check()
        assert bool((got["ratio"][idx] == 0).all()) and bool((got["logp"][idx] == 0).all())
        assert not same_grads(got["grads"], want["grads"]), same_grads(got["grads"], want["grads"])
        for k in ("loss_policy", "loss_value", "loss"):
            assert same(got[k], want[k]), (k, chunk_rows)
        assert got["ppo_sums"][0] == want["ppo_sums"][0] and got["ppo_sums"][2] == want["ppo_sums"][2]
        for k in ROWS_OUT:
            assert np.array_equal(got[k].numpy()[others].view(np.int32), want[k].numpy()[others].view(np.int32)), k
        p = predicted(want, ok, ppc.CLIP, ppc.VALUE_CLIP, "smooth_l1")
        assert_counts(want, p)
        assert not p["clipped"][idx].any() and not p["value_clipped"][idx].any()
        assert bool((want["ratio"][idx] != 1).all()) and (p["k3"][idx] > 0).all()
        assert_float_sums(got, p, rows=others)
        assert not same(got["ppo_sums"][3], want["ppo_sums"][3]) and not same(got["ppo_sums"][1], want["ppo_sums"][1])
        h = want["entropy_rows"].numpy().astype(np.float64)
        assert ppc.units_apart(float(got["entropy"]), h[others].sum()) <= 1
        assert ppc.units_apart(float(want["entropy"]), h.sum()) <= 1 and not same(got["entropy"], want["entropy"])
        clean = run_ppo(pol, ok, **kw)  # (check() inside: a following clean call reports none)
        assert first_difference(want, clean) is None
    pol.close()


# ------------------------------------------------------------------ 4. more than one block per slab
def mixed_rows(ev, c, n, seed):
    """old_logp and old_value from ppc.DELTAS and ppc.EPSILONS added to evaluate's bits; a row
    whose host-side decisions are not clear by more than 2^-10 (relative) takes delta 0 and the
    small eps of its sign, which are (ties are tests 1 and 2).  Returns the number of such rows."""
    rng = np.random.RandomState(seed)
    delta = rng.choice(ppc.DELTAS, size=n).astype(np.float32)
    eps = rng.choice(ppc.EPSILONS, size=n).astype(np.float32)
    m = 2.0 ** -10
    lo, hi, cc = ppc.LO, ppc.HI, float(F32(ppc.VALUE_CLIP))
    for _ in range(2):
        old_logp, old_value = (ev["logp"] + delta).astype(np.float32), (ev["value"] + eps).astype(np.float32)
        r = np.exp((ev["logp"] - old_logp).astype(np.float64))
        clear = (np.abs(r - hi) > m * hi) & (np.abs(r - lo) > m * lo)
        v, t = ev["value"].astype(np.float64), c["t"].astype(np.float64)
        u = v - old_value
        vc = old_value + np.where(u > 0, cc, -cc)
        clear &= np.abs(np.abs(u) - cc) > m * cc
        clear &= np.abs(np.abs(v - t) - 1.0) > m
        out = np.abs(u) > cc
        clear &= ~out | (np.abs(np.abs(vc - t) - 1.0) > m)
        for value_loss in ("smooth_l1", "mse"):
            l1, l2 = ppc._loss(v - t, value_loss), ppc._loss(vc - t, value_loss)
            clear &= ~out | (np.abs(l2 - l1) > m * np.maximum(l1, l2))
        dropped = int((~clear).sum())
        delta[~clear] = 0.0
        eps[~clear] = np.sign(eps[~clear]) * F32(0.0625)
    assert clear.all()
    return old_logp, old_value, dropped


@pytest.mark.parametrize("net", BIG_NETS, ids=str)
def test_two_blocks_in_every_slab(net):
    from test_gpu_policy_grad_slabs import slabs_of

    pol = tp.policy_for(net)
    S = slabs_of(pol, net)
    # evaluate's one-pass grid past block S, and a last block of 5 rows
    for n in (pgc.fold_rows_n(S), pgc.two_per_slab_n(S)):
        c = inputs(net, n)
        ev = evaluate(pol, c)
        lg = tp.run_a2c(pol, c["x"], c["a"], c["adv"], c["t"])
        for k, k2 in (("logp", "logp"), ("value", "value"), ("entropy", "entropy_rows")):
            assert same(torch.as_tensor(ev[k]), lg[k2]), (k, n)
    assert n == 2 * S * 128 + 129 and (n + 127) // 128 == 2 * S + 2
    chunks = (0, 128 * 3, 128 * S, 128 * (S + 1))
    kw = dict(value_coef=0.5, entropy_coef=0.01)
    # ratio 1: the PPO instance of the backward kernel and the seven-term loss task give the A2C step
    c["old_logp"] = ev["logp"]
    for chunk_rows in chunks:
        a2c = tp.run_a2c(pol, c["x"], c["a"], c["adv"], c["t"], chunk_rows=chunk_rows, **kw)
        got = run_ppo(pol, c, clip=ppc.CLIP, chunk_rows=chunk_rows, **kw)
        assert not same_grads(got["grads"], a2c["grads"]), chunk_rows
        for k in ("loss_value", "entropy", "logp", "value", "entropy_rows"):
            assert same(got[k], a2c[k]), (k, chunk_rows)
        # loss_policy is -sum(1.0f A) here and -sum(A logp) there, and the total follows it: its own
        # value (the advantages are dyadic, the double sum is exact), and the total from the parts
        assert float(got["loss_policy"]) == float(F32(-c["adv"].astype(np.float64).sum()))
        total = float(got["loss_policy"]) + 0.5 * float(got["loss_value"]) - float(F32(0.01)) * float(got["entropy"])
        assert abs(float(got["loss"]) - total) <= 2.0 ** -22 * (abs(float(got["loss_policy"])) + float(got["loss_value"])
                                                                + float(got["entropy"]))
        assert bool((got["ratio"] == 1.0).all())
        assert got["ppo_sums"].tolist() == [0.0, 0.0, 0.0, float(n)], chunk_rows
    # mixed rows
    c["old_logp"], c["old_value"], dropped = mixed_rows(ev, c, n, 77)
    print("%s N=%d: %d rows within 2^-10 of a decision took the plain delta and eps" % (net, n, dropped))
    for value_loss in ("smooth_l1", "mse"):
        base = None
        for chunk_rows in chunks + (0,):
            kw2 = dict(value_loss=value_loss, chunk_rows=chunk_rows, **kw)
            got = run_ppo(pol, c, clip=ppc.CLIP, value_clip=ppc.VALUE_CLIP, **kw2)
            if base is None:
                base = got
                p = predicted(got, c, ppc.CLIP, ppc.VALUE_CLIP, value_loss)
                cl, vcl, out = p["clipped"], p["value_clipped"], p["outside"]
                assert min(cl.sum(), (~cl).sum(), vcl.sum(), (out & ~vcl).sum(), (~out).sum()) >= n // 16
                assert_counts(got, p)
                assert_effective_weight_case(pol, got, c, p, **kw2)
                assert all(bool((got["grads"][k] != 0).any()) for k in pgc.GRAD_NAMES)
            else:
                assert first_difference(base, got) is None, (chunk_rows, first_difference(base, got))
    # what the big call leaves behind
    small = {k: v[:130] for k, v in c.items()}
    F = pgc.net_shape(net)[0]
    z = np.zeros(0, np.float32)
    empty = {"x": np.zeros((0, F), np.float32), "a": np.zeros(0, np.int8), "adv": z, "t": z, "old_logp": z, "old_value": z}
    kw3 = dict(clip=ppc.CLIP, value_clip=ppc.VALUE_CLIP, **kw)
    for rows in (small, empty):
        used = run_ppo(pol, rows, **kw3)
        fresh = tp.policy_for(net)
        want = run_ppo(fresh, rows, **kw3)
        fresh.close()
        assert first_difference(want, used) is None, (len(rows["a"]), first_difference(want, used))
    assert all(float(x) == 0.0 for k in SUMS for x in used[k].reshape(-1))
    assert float(run_ppo(pol, small, **kw3)["ppo_sums"][3]) > 0
    pol.close()
