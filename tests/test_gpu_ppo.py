"""wab_policy_evaluate and wab_policy_grad_ppo on the GPU (DevicePolicy.evaluate, ppo_loss_and_grad)
against their contract (wab_gym_amd.policy.reference_ppo_loss_and_grad) and against the verified
wab_policy_grad:

1. evaluate's rows are loss_and_grad's row outputs bit for bit (value: act's);
2. with old_logp from evaluate the ratio is exactly 1 and every gradient is loss_and_grad's of
   weight = advantage, bit for bit;
3. on mixed rows (tests/ppo_cases.py) the gradients are loss_and_grad's of the effective weight
   ratio * A (0 where clipped) and of target = value where the value loss is clipped, bit for bit;
4. everything clipped gives all-zero gradients;
5. every output within half of E (what the bf16 contract costs against stock fp32 autograd of the
   textbook formula), the counts exact;
6. the edges: N = 0, accumulate over two ranges, mean, [T, B, F], into=model, a captured graph of
   evaluate, the clipped step and DeviceAdam.step, the refused arguments;
7. a short run of examples/train_ppo.py's update.

Measured on an MI355X (max |kernel - contract| / E, worst case per net): see DESIGN.md,
"wab_policy_grad_ppo"."""
import ctypes
import functools
import importlib.util
import os

import numpy as np
import pytest
import torch

import policy_cases as pc
import policy_grad_cases as pgc
import ppo_cases as ppc
from wab_gym_amd import _lib, policy
from wab_gym_amd.env import BatchedWolvesAndBushesEnv
from wab_gym_amd.wrappers import PragmaticObsWrapper

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID, E_STATE = -1, -4  # WAB_E_INVALID, WAB_E_STATE (include/wab.h)
DIAG = ("clip_fraction", "approx_kl", "value_clip_fraction", "ratio_mean")


@functools.lru_cache(maxsize=None)
def env_for(n_actions, B):
    env = BatchedWolvesAndBushesEnv(dict(pc.OPTS_REF if n_actions == 5 else pc.OPTS_ODD), num_envs=B, seed=pc.SEED,
                                    device=DEV)
    env.reset()
    return env


def policy_for(net, B=128):
    return policy.DevicePolicy(pgc.state_dict(net), env_for(pgc.net_shape(net)[4], B))


def dev(x, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(x), dtype=dtype).to(DEV)


def cpu(r):
    out = {k: v.cpu() for k, v in r.items() if k != "grads"}
    if "grads" in r:
        out["grads"] = {k: v.cpu() for k, v in r["grads"].items()}
    return out


def run_a2c(pol, x, a, w, t, **kw):
    r = pol.loss_and_grad(dev(x, torch.float32), dev(a, torch.int8), dev(w, torch.float32), dev(t, torch.float32),
                          return_rows=True, **kw)
    pol.check()
    return cpu(r)


def run_ppo(pol, c, old_logp=None, value_clip=ppc.VALUE_CLIP, clip=ppc.CLIP, **kw):
    """ppo_loss_and_grad on a case's host arrays; everything back on the CPU."""
    olp = c["old_logp"] if old_logp is None else old_logp
    r = pol.ppo_loss_and_grad(dev(c["x"], torch.float32), dev(c["a"], torch.int8), dev(c["adv"], torch.float32),
                              dev(c["t"], torch.float32), dev(olp, torch.float32), clip=clip,
                              old_value=dev(c["old_value"], torch.float32), value_clip=value_clip, return_rows=True,
                              **kw)
    pol.check()
    return cpu(r)


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and bool((a.view(torch.int32) == b.view(torch.int32)).all())


def same_grads(g1, g2):
    return [k for k in pgc.GRAD_NAMES if not same(g1[k], g2[k])]


def plain_case(net, n):
    """policy_grad_cases' rows as a case (old_logp and old_value to be filled by the test)."""
    a, w, t = pgc.rows(net, n)
    return {"x": pgc.features(net, n), "a": a, "adv": w, "t": t, "old_logp": np.zeros(n, np.float32),
            "old_value": np.zeros(n, np.float32)}


# ------------------------------------------------------------------ 1. evaluate
@pytest.mark.parametrize("net", pgc.NETS, ids=str)
@pytest.mark.parametrize("n", ppc.ROWS)
def test_evaluate_is_the_gradients_forward(net, n):
    c = plain_case(net, n)
    A = pgc.net_shape(net)[4]
    pol = policy.DevicePolicy(pgc.state_dict(net), env_for(A, n))
    x, a = dev(c["x"], torch.float32), dev(c["a"], torch.int8)
    ev = cpu(pol.evaluate(x, a))
    pol.check()
    lg = run_a2c(pol, c["x"], c["a"], c["adv"], c["t"])
    assert sorted(ev) == ["entropy", "logp", "value"]
    assert same(ev["logp"], lg["logp"]) and same(ev["value"], lg["value"]) and same(ev["entropy"], lg["entropy_rows"])
    value = torch.empty(n, device=DEV)
    pol.act(x, value=value)
    assert same(ev["value"], value.cpu())
    ev2 = cpu(pol.evaluate(x))
    assert sorted(ev2) == ["entropy", "value"] and same(ev2["value"], ev["value"]) and same(ev2["entropy"], ev["entropy"])
    ev3 = cpu(pol.evaluate(x.view(1, n, -1), a.view(1, n)))
    assert ev3["logp"].shape == (1, n) and same(ev3["logp"].view(n), ev["logp"])
    pol.close()


def test_evaluate_counts_a_bad_action():
    n = 130
    c = plain_case("odd", n)
    pol = policy_for("odd")
    a_bad = c["a"].copy()
    a_bad[129] = 6
    ev = pol.evaluate(dev(c["x"], torch.float32), dev(a_bad, torch.int8))
    with pytest.raises(IndexError, match="1 rows"):
        pol.check()
    assert float(ev["logp"][129]) == 0.0
    good = pol.evaluate(dev(c["x"], torch.float32), dev(c["a"], torch.int8))
    pol.check()
    assert same(ev["logp"][:129].cpu(), good["logp"][:129].cpu())
    with pytest.raises(ValueError):
        pol.evaluate(dev(c["x"], torch.float32), dev(c["a"], torch.int8).long())
    pol.close()


# ------------------------------------------------------------------ 2. ratio 1 is A2C
@pytest.mark.parametrize("net", pgc.NETS, ids=str)
@pytest.mark.parametrize("n", ppc.ROWS)
def test_ratio_one_is_the_a2c_step(net, n):
    c = plain_case(net, n)
    pol = policy_for(net)
    old = pol.evaluate(dev(c["x"], torch.float32), dev(c["a"], torch.int8))["logp"].cpu().numpy()
    for chunk_rows in (0, 128):
        for clip in (0.05, 0.25):
            kw = dict(value_coef=0.5, entropy_coef=0.01, chunk_rows=chunk_rows)
            a2c = run_a2c(pol, c["x"], c["a"], c["adv"], c["t"], **kw)
            got = run_ppo(pol, c, old_logp=old, value_clip=None, clip=clip, **kw)
            assert not same_grads(got["grads"], a2c["grads"]), (chunk_rows, clip)
            for k in ("value", "logp", "entropy_rows", "loss_value", "entropy"):
                assert same(got[k], a2c[k]), k
            assert bool((got["ratio"] == 1.0).all())
            assert got["ppo_sums"].tolist() == [0.0, 0.0, 0.0, float(n)]
            assert [float(got[k]) for k in DIAG] == [0.0, 0.0, 0.0, 1.0]
            assert float(got["loss_policy"]) == float(np.float32(-c["adv"].astype(np.float64).sum()))
    pol.close()


# ------------------------------------------------------------------ 3. the effective-weight case
@pytest.mark.parametrize("net", pgc.NETS, ids=str)
@pytest.mark.parametrize("n", ppc.ROWS)
def test_general_case_is_the_effective_weight_case(net, n):
    c = ppc.case(net, n)
    pol = policy_for(net)
    for value_loss in ("smooth_l1", "mse"):
        for ec in (0.0, 0.01):
            ref, _ = ppc.contract_and_cost(net, n, 0.5, ec, value_loss)
            for chunk_rows in (0, 128):
                kw = dict(value_coef=0.5, entropy_coef=ec, value_loss=value_loss, chunk_rows=chunk_rows)
                got = run_ppo(pol, c, **kw)
                w_eff = got["ratio"].numpy() * c["adv"]
                assert w_eff.dtype == np.float32
                w_eff[ref["clipped"].numpy()] = 0.0
                t2 = np.where(ref["value_clipped"].numpy(), got["value"].numpy(), c["t"]).astype(np.float32)
                a2c = run_a2c(pol, c["x"], c["a"], w_eff, t2, **kw)
                assert not same_grads(got["grads"], a2c["grads"]), (value_loss, ec, chunk_rows)
                assert all(bool((got["grads"][k] != 0).any()) for k in pgc.GRAD_NAMES) or n == 1 \
                    or net == (1, 1, 1, 1, 5)
    pol.close()


# ------------------------------------------------------------------ 4. everything clipped
def test_everything_clipped_is_zero():
    n = 257
    c = dict(plain_case("ref", n))
    c["adv"] = (np.abs(c["adv"]) + 0.25).astype(np.float32)
    pol = policy_for("ref")
    logp = pol.evaluate(dev(c["x"], torch.float32), dev(c["a"], torch.int8))["logp"].cpu().numpy()
    got = run_ppo(pol, c, old_logp=logp - np.float32(1.0), value_clip=None, value_coef=0.0, entropy_coef=0.0)
    for k in pgc.GRAD_NAMES:
        assert bool((got["grads"][k].view(torch.int32) == 0).all()), k
    assert float(got["clip_fraction"]) == 1.0 and got["ppo_sums"][0] == n
    hi = np.float32(1.0) + np.float32(ppc.CLIP)
    assert float(got["loss_policy"]) == float(np.float32(-(c["adv"].astype(np.float64) * float(hi)).sum()))
    pol.close()


# ------------------------------------------------------------------ 5. against the contract
WORST = {}


def check_gate(got, ref, E, what, worst):
    """max |kernel - contract| <= 0.5 E per gradient tensor, loss part, row output and sum (exact
    where E is 0); prints each ratio before it asserts."""
    pairs = [(k, got["grads"][k].double(), ref["grads"][k]) for k in pgc.GRAD_NAMES]
    pairs += [(k, got[k].double(), ref["loss"][i]) for i, k in enumerate(("loss_policy", "loss_value", "entropy", "loss"))]
    pairs += [("logp", got["logp"].double(), ref["logp"]), ("value", got["value"].double(), ref["value"]),
              ("entropy_rows", got["entropy_rows"].double(), ref["entropy"]), ("ratio", got["ratio"].double(), ref["ratio"]),
              ("k3_sum", got["ppo_sums"][1].double(), ref["ppo"][1]), ("ratio_sum", got["ppo_sums"][3].double(), ref["ppo"][3])]
    failed = []
    for k, g, r in pairs:
        err = float((g - r).abs().max())
        ratio = err / E[k] if E[k] > 0 else (0.0 if err == 0 else float("inf"))
        print("%s %s: err %.3e  E %.3e  ratio %.4f" % (what, k, err, E[k], ratio))
        worst[k] = max(worst.get(k, 0.0), ratio)
        if not err <= 0.5 * E[k]:
            failed.append((k, err, E[k]))
    assert not failed, (what, failed)


@pytest.mark.parametrize("net", pgc.NETS, ids=str)
@pytest.mark.parametrize("n", ppc.ROWS)
def test_against_the_contract(net, n):
    c = ppc.case(net, n)
    pol = policy_for(net)
    worst = WORST.setdefault(str(net), {})
    missed = []
    for value_loss in ("smooth_l1", "mse"):
        for ec in (0.0, 0.01):
            ref, E = ppc.contract_and_cost(net, n, 0.5, ec, value_loss)
            got = run_ppo(pol, c, value_coef=0.5, entropy_coef=ec, value_loss=value_loss)
            assert got["ppo_sums"][0] == float(ref["ppo"][0]) and got["ppo_sums"][2] == float(ref["ppo"][2])
            try:  # (every configuration is run and printed before the first miss is raised)
                check_gate(got, ref, E, "%s N=%d %s ec=%g" % (net, n, value_loss, ec), worst)
            except AssertionError as e:
                missed.append(e)
            for i, k in enumerate(DIAG):
                assert abs(float(got[k]) - float(got["ppo_sums"][i]) / n) <= 2.0 ** -23 * abs(float(got[k]))
    print("worst ratios so far, %s: %s" % (net, "  ".join("%s %.4f" % kv for kv in sorted(worst.items()))))
    pol.close()
    if missed:
        raise missed[0]


# ------------------------------------------------------------------ 6. edges
def test_no_rows_give_zeros():
    pol = policy_for("odd")
    z = np.zeros(0, np.float32)
    c = {"x": np.zeros((0, 37), np.float32), "a": np.zeros(0, np.int8), "adv": z, "t": z, "old_logp": z, "old_value": z}
    got = run_ppo(pol, c)
    assert all(bool((got["grads"][k] == 0).all()) for k in pgc.GRAD_NAMES)
    assert all(float(got[k]) == 0.0 for k in ("loss", "loss_policy", "loss_value", "entropy") + DIAG)
    assert got["ratio"].shape == (0,)
    ev = pol.evaluate(dev(c["x"], torch.float32), dev(c["a"], torch.int8))
    assert ev["logp"].shape == (0,)
    pol.check()
    pol.close()


def model_of(seed=0):
    spec = importlib.util.spec_from_file_location("train_ppo", os.path.join(REPO, "examples", "train_ppo.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    torch.manual_seed(seed)
    return mod, mod.Policy(449, 5).to(DEV)


def test_accumulate_mean_views_into_model_and_rerun():
    n = 257
    c = ppc.case("ref", n)
    _, model = model_of()
    pol = policy.DevicePolicy(model, env_for(5, 128))
    keys = ("x", "a", "adv", "t", "old_logp", "old_value")
    dt = dict(a=torch.int8)
    full = {k: dev(c[k], dt.get(k, torch.float32)) for k in keys}

    def call(lo, hi, **kw):
        s = slice(lo, hi)
        return pol.ppo_loss_and_grad(full["x"][s], full["a"][s], full["adv"][s], full["t"][s], full["old_logp"][s],
                                     clip=ppc.CLIP, old_value=full["old_value"][s], value_clip=ppc.VALUE_CLIP,
                                     entropy_coef=0.01, **kw)

    once = call(0, n)
    assert not same_grads(call(0, n)["grads"], once["grads"])  # a second run: the same bits
    assert all(p.grad is None for p in model.parameters())
    p1, p2 = call(0, 128), call(128, n)
    out = call(0, 128, into=model)
    assert "grads" not in out
    out2 = call(128, n, into=model, accumulate=True)
    sd = dict(model.named_parameters())
    for k in pgc.GRAD_NAMES:
        assert same(sd[k].grad, p1["grads"][k] + p2["grads"][k]), k  # (a two-term fp32 sum has no order)
    # accumulate adds to the caller's sums as it does to loss_out: here each call has its own, so the parts add up
    for k in ("ppo_sums",):
        assert torch.equal(p1[k] + p2[k], out[k] + out2[k])
    assert float(p1["ppo_sums"][0] + p2["ppo_sums"][0]) == float(once["ppo_sums"][0])
    assert float(p1["ppo_sums"][2] + p2["ppo_sums"][2]) == float(once["ppo_sums"][2])
    # [T, B, F] is its [T B, F] view: 257 = 1 x 257
    s3 = pol.ppo_loss_and_grad(full["x"].view(1, n, -1), *[full[k].view(1, n) for k in ("a", "adv", "t", "old_logp")],
                               clip=ppc.CLIP, old_value=full["old_value"].view(1, n), value_clip=ppc.VALUE_CLIP,
                               entropy_coef=0.01, return_rows=True)
    assert not same_grads(s3["grads"], once["grads"]) and same(s3["loss"], once["loss"]) and s3["ratio"].shape == (1, n)
    # mean: scale 1 / N on the total and the gradients, the parts and the diagnostics unscaled
    mean = call(0, n, reduction="mean")
    inv = np.float32(1.0 / n)
    for k in pgc.GRAD_NAMES:
        diff = mean["grads"][k].double() - once["grads"][k].double() * float(inv)
        assert float(diff.abs().max()) <= 2.0 ** -22 * float(once["grads"][k].abs().max()) * float(inv), k
    assert same(mean["loss_policy"], once["loss_policy"]) and same(mean["ppo_sums"], once["ppo_sums"])
    pol.check()
    pol.close()


def test_accumulate_adds_to_ppo_out():
    """The C call with loss->accumulate adds to ppo_out as it does to loss_out."""
    n = 129
    c = ppc.case("odd", n)
    pol = policy_for("odd")
    L = _lib.load()
    t = {k: dev(c[k], torch.int8 if k == "a" else torch.float32) for k in ("x", "a", "adv", "t", "old_logp", "old_value")}
    first = pol.ppo_loss_and_grad(t["x"], t["a"], t["adv"], t["t"], t["old_logp"], clip=ppc.CLIP,
                                  old_value=t["old_value"], value_clip=ppc.VALUE_CLIP)
    grads = first["grads"]
    sums = torch.cat([torch.stack([first[k] for k in ("loss_policy", "loss_value", "entropy", "loss")]),
                      first["ppo_sums"]]).clone()
    cfg = _lib.WabPolicyLoss(1.0, 0.0, 0, 1.0, 1, 0)
    ppo = _lib.WabPpoConfig(ppc.CLIP, ppc.VALUE_CLIP)
    gw = _lib.WabPolicyWeights(*[grads[k].data_ptr() for k in pgc.GRAD_NAMES])
    want = {k: (g + g).cpu() for k, g in grads.items()}
    _lib.check(L.wab_policy_grad_ppo(pol._p, t["x"].data_ptr(), t["a"].data_ptr(), t["adv"].data_ptr(), t["t"].data_ptr(),
                                     t["old_logp"].data_ptr(), t["old_value"].data_ptr(), n, ctypes.addressof(cfg),
                                     ctypes.addressof(ppo), ctypes.addressof(gw), sums.data_ptr(), sums[4:].data_ptr(),
                                     None, None, None, None, pol._grad_ws.data_ptr(), pol._grad_ws.numel(),
                                     pol.env._stream()), "wab_policy_grad_ppo")
    torch.cuda.synchronize()
    assert not same_grads({k: g.cpu() for k, g in grads.items()}, want)
    assert torch.equal(sums[4:].cpu(), (first["ppo_sums"] + first["ppo_sums"]).cpu()) and float(sums[7]) > 0
    pol.close()


def test_refused_arguments():
    n = 129
    c = ppc.case("odd", n)
    pol = policy_for("odd")
    L = _lib.load()
    t = {k: dev(c[k], torch.int8 if k == "a" else torch.float32) for k in ("x", "a", "adv", "t", "old_logp", "old_value")}
    base = dict(features=t["x"], actions=t["a"], advantage=t["adv"], target=t["t"], old_logp=t["old_logp"])
    for kw in (dict(clip=0.0), dict(clip=1.0), dict(clip=float("nan")), dict(value_clip=0.2),
               dict(old_logp=t["old_logp"].double()), dict(old_logp=t["old_logp"].cpu()), dict(chunk_rows=100),
               dict(accumulate=True)):
        args = dict(base)
        args.update(kw)
        with pytest.raises(ValueError):
            pol.ppo_loss_and_grad(**args)
    with pytest.raises(ValueError):
        pol.evaluate(t["x"][:, :5])
    # the C calls' own checks
    first = pol.ppo_loss_and_grad(**base)
    gw = _lib.WabPolicyWeights(*[first["grads"][k].data_ptr() for k in pgc.GRAD_NAMES])
    cfg = _lib.WabPolicyLoss(1.0, 0.0, 0, 1.0, 0, 0)
    ws, st = pol._grad_ws, pol.env._stream()

    def c_call(clip, value_clip, old_logp, old_value, ws_ptr=None):
        ppo = _lib.WabPpoConfig(clip, value_clip)
        return L.wab_policy_grad_ppo(pol._p, t["x"].data_ptr(), t["a"].data_ptr(), t["adv"].data_ptr(), t["t"].data_ptr(),
                                     old_logp, old_value, n, ctypes.addressof(cfg), ctypes.addressof(ppo),
                                     ctypes.addressof(gw), None, None, None, None, None, None,
                                     ws.data_ptr() if ws_ptr is None else ws_ptr, ws.numel(), st)

    olp, ov = t["old_logp"].data_ptr(), t["old_value"].data_ptr()
    assert c_call(0.2, 0.0, olp, None) == 0
    for args in ((0.0, 0.0, olp, None), (1.0, 0.0, olp, None), (float("nan"), 0.0, olp, None), (0.2, 0.0, None, None),
                 (0.2, 0.25, olp, None), (0.2, 0.0, olp + 2, None), (0.2, 0.25, olp, ov + 1)):
        assert c_call(*args) == E_INVALID, args
    assert c_call(0.2, 0.0, olp, None, ws_ptr=ws.data_ptr() + 64) == E_INVALID
    small = torch.empty(512, dtype=torch.uint8, device=DEV)
    ptr = (small.data_ptr() + 255) & ~255
    assert L.wab_policy_evaluate(pol._p, t["x"].data_ptr(), None, n, olp, None, None, ptr, 256, st) == E_INVALID
    assert L.wab_policy_evaluate(pol._p, t["x"].data_ptr(), t["a"].data_ptr(), n, olp, None, None, ptr, 255, st) \
        == E_INVALID
    assert L.wab_policy_evaluate(pol._p, t["x"].data_ptr(), None, n, None, ov, None, ptr, 256, st) == 0
    torch.cuda.synchronize()
    # before the first load: a policy created through the C call alone
    shp = _lib.WabPolicyShape(37, 40, 40, 40, 6)
    raw = ctypes.c_void_p()
    _lib.check(L.wab_policy_create(ctypes.addressof(shp), 0, ctypes.byref(raw)), "wab_policy_create")
    assert L.wab_policy_evaluate(raw, t["x"].data_ptr(), None, n, None, ov, None, ptr, 256, st) == E_STATE
    L.wab_policy_destroy(raw)
    pol.close()


def test_a_captured_graph_of_evaluate_ppo_and_adam_equals_eager():
    B, T = 256, 4
    _, model = model_of(seed=5)
    env = BatchedWolvesAndBushesEnv(dict(pc.OPTS_REF), num_envs=B, seed=pc.SEED, device=DEV)
    wrapper = PragmaticObsWrapper(env)
    wrapper.reset()
    pol = policy.DevicePolicy(model, env)
    opt = policy.DeviceAdam(pol, model, lr=1e-3, max_grad_norm=0.5)
    r = wrapper.rollout_policy(pol, T, bootstrap_value=True, gae_lambda=0.95, whiten=True)
    start = [p.detach().clone() for p in model.parameters()]

    def reset():
        with torch.no_grad():
            for p, q in zip(model.parameters(), start):
                p.copy_(q)
        pol.load(model)
        for m in opt.exp_avg + opt.exp_avg_sq:
            m.zero_()
        opt._state.zero_()

    def sequence():
        old = pol.evaluate(r["features"], r["actions"])["logp"]
        out = None
        for s in (slice(0, 2), slice(2, 4)):  # the second minibatch sees the first's step: ratio != 1
            out = pol.ppo_loss_and_grad(r["features"][s], r["actions"][s], r["advantage"][s], r["target"][s], old[s],
                                        clip=0.2, old_value=r["value"][s], value_clip=0.2, into=model,
                                        reduction="mean", entropy_coef=0.01)
            opt.step()
        return out

    eager = sequence()
    want = [p.detach().clone() for p in model.parameters()]
    want_out = {k: eager[k].clone() for k in ("loss", "approx_kl", "ratio_mean")}
    assert float(want_out["approx_kl"]) > 0 and all(not torch.equal(p, q) for p, q in zip(want, start))
    reset()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        cap = sequence()
    for _ in range(2):
        reset()
        g.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(p.detach(), q) for p, q in zip(model.parameters(), want))
        assert all(torch.equal(cap[k], want_out[k]) for k in want_out)
    pol.check()
    pol.close()


# ------------------------------------------------------------------ 7. a short run
def test_a_short_ppo_run(capsys):
    B, T = 256, 16
    mod, model = model_of(seed=3)
    env = BatchedWolvesAndBushesEnv(dict(pc.OPTS_REF), num_envs=B, seed=pc.SEED, device=DEV)
    wrapper = PragmaticObsWrapper(env)
    wrapper.reset()
    pol = policy.DevicePolicy(model, env)
    opt = policy.DeviceAdam(pol, model, lr=3e-4, max_grad_norm=0.5)
    before = [p.detach().clone() for p in model.parameters()]
    results = mod.update(wrapper, pol, model, opt, T, epochs=2, minibatches=2, clip=0.2, value_clip=0.2,
                         entropy_coef=0.01, report=mod.print_epoch)
    pol.check()
    printed = capsys.readouterr().out.split()
    numbers = []
    for w in printed:
        try:
            numbers.append(float(w))
        except ValueError:
            pass
    assert len(numbers) == 2 * 3 and all(np.isfinite(numbers)), printed  # loss, clip fraction, kl per epoch
    flat = [o for outs in results for o in outs]
    assert len(flat) == 4
    assert float(flat[0]["approx_kl"]) == 0.0 and float(flat[0]["clip_fraction"]) == 0.0
    assert float(flat[0]["ratio_mean"]) == 1.0 and float(flat[0]["value_clip_fraction"]) == 0.0
    for o in flat[1:]:
        assert float(o["approx_kl"]) >= 0.0 and np.isfinite(float(o["loss"]))
    assert any(float(o["approx_kl"]) > 0.0 for o in flat[1:])
    assert all(not torch.equal(p.detach(), q) for p, q in zip(model.parameters(), before))
    assert opt.stats()["step"] == 4 and opt.stats()["skipped"] == 0
    pol.close()
