"""wab_policy_grad on the GPU (DevicePolicy.loss_and_grad) against its contract
(wab_gym_amd.policy.reference_loss_and_grad):

1. every term in its place, bit for bit: one live row, dW_l the outer product of db_l and x_{l-1};
2. sums across tiles, slabs and chunks, bit for bit: two live rows, fl32(term_1 + term_2).  The
   two rows lie in row blocks 0 and 1, two slabs, so this is the reducer's add; sums inside a
   slab (a slab's second block, N > 128 slabs) are tests/test_gpu_policy_grad_slabs.py's;
3. chunk_rows changes no bit, and neither does a second run;
4. every tensor, loss and row output within half of E (what the bf16 contract itself costs
   against stock fp32 autograd on the same inputs, tests/policy_grad_cases.py);
5. the edges: N = 0, accumulate, mean, [T, B, F], a bad action, into=model, one training step,
   a captured graph.

Measured on an MI355X (max |kernel - contract| / E, worst case per tensor): see DESIGN.md,
"wab_policy_grad.hip"."""
import ctypes
import functools
import importlib.util
import os

import numpy as np
import pytest
import torch

import policy_cases as pc
import policy_grad_cases as pgc
from wab_gym_amd import _lib, policy
from wab_gym_amd.env import BatchedWolvesAndBushesEnv
from wab_gym_amd.wrappers import PragmaticObsWrapper

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADS = ("action_head", "value_head")


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


def run(pol, x, a, w, t, **kw):
    """loss_and_grad on host arrays; everything back on the CPU."""
    r = pol.loss_and_grad(dev(x, torch.float32), dev(a, torch.int8), dev(w, torch.float32), dev(t, torch.float32),
                          return_rows=True, **kw)
    out = {k: v.cpu() for k, v in r.items() if k != "grads"}
    out["grads"] = {k: v.cpu() for k, v in r["grads"].items()}
    pol.check()
    return out


def same(a, b):
    return a.shape == b.shape and torch.equal(a, b)


def same_result(r1, r2):
    return all(same(r1["grads"][k], r2["grads"][k]) for k in pgc.GRAD_NAMES) and \
        all(same(r1[k], r2[k]) for k in r1 if k != "grads")


def layer_inputs(net, x):
    """x_0 .. x_3 of the contract (bf16 values as float64), by the layer that reads them."""
    hidden = []
    policy.reference_forward(pgc.state_dict(net), x, hidden=hidden)
    xs = [torch.as_tensor(x).float().to(torch.bfloat16).double()] + [h[1] for h in hidden]
    return dict(zip(policy.LAYERS, xs + [xs[3]]))


def one_live(w, t, value, live):
    """weights and targets under which every row but `live` has G_4 = 0 exactly (entropy_coef 0)."""
    w1, t1 = np.zeros_like(w), np.asarray(value, dtype=np.float32).copy()
    for i in live:
        w1[i] = w[i] if w[i] != 0 else 1.5
        t1[i] = t[i]
    return w1, t1


def check_gate(got, ref, E, what, worst=None, keys=None):
    """max |kernel - contract| <= 0.5 E per gradient tensor, loss part and row output; prints
    each ratio before it asserts."""
    pairs = [(k, got["grads"][k].double(), ref["grads"][k]) for k in (pgc.GRAD_NAMES if keys is None else keys)]
    if keys is None:
        pairs += [(k, got[k].double(), ref["loss"][i]) for i, k in
                  enumerate(("loss_policy", "loss_value", "entropy", "loss"))]
        pairs += [("logp", got["logp"].double(), ref["logp"]), ("value", got["value"].double(), ref["value"]),
                  ("entropy_rows", got["entropy_rows"].double(), ref["entropy"])]
    failed = []
    for k, g, r in pairs:
        err = float((g - r).abs().max())
        ratio = err / E[k] if E[k] > 0 else (0.0 if err == 0 else float("inf"))
        print("%s %s: err %.3e  E %.3e  ratio %.4f" % (what, k, err, E[k], ratio))
        if worst is not None:
            worst[k] = max(worst.get(k, 0.0), ratio)
        if not err <= 0.5 * E[k]:
            failed.append((k, err, E[k]))
    assert not failed, (what, failed)


# ------------------------------------------------------------------ 1. one live row, exactly
@pytest.mark.parametrize("net", pgc.EXACT_NETS, ids=str)
@pytest.mark.parametrize("n", (129, 257))
def test_one_live_row_every_term_in_its_place(net, n):
    sd, x = pgc.state_dict(net), pgc.features(net, n)
    a, w, t = pgc.rows(net, n)
    pol = policy_for(net)
    value = run(pol, x, a, w, t)["value"].numpy()
    xs = layer_inputs(net, x)
    for live in (0, 31, 32, 127, 128, n - 1):
        w1, t1 = one_live(w, t, value, (live,))
        ref = policy.reference_loss_and_grad(sd, x, a, w1, t1)
        E = pgc.cost_of(ref, pgc.fp32_loss_and_grad(sd, x, a, w1, t1))
        for scale in (1.0, 0.25):
            got = run(pol, x, a, w1, t1, scale=scale)
            some = False
            for layer in policy.LAYERS:
                db = got["grads"][layer + ".bias"].double()
                want = (db[:, None] * xs[layer][live][None, :]).float()  # (db / scale) * x * scale: exact
                assert same(got["grads"][layer + ".weight"], want), (layer, live, scale)
                some = some or bool((db != 0).any())
            assert some, (live, scale)
            if scale == 1.0:
                check_gate(got, ref, E, "one live row %d of %d" % (live, n), keys=[l + ".bias" for l in policy.LAYERS])
            else:
                for k in pgc.GRAD_NAMES:
                    assert same(got["grads"][k], (full[k].double() * 0.25).float()), (k, live)
            full = got["grads"]
    pol.close()


# ------------------------------------------------------------------ 2. two live rows, exactly
@pytest.mark.parametrize("net", pgc.EXACT_NETS, ids=str)
@pytest.mark.parametrize("pair", ((5, 200), (127, 128)))
def test_two_live_rows_sum_across_tiles_slabs_and_chunks(net, pair):
    n = 257
    x = pgc.features(net, n)
    a, w, t = pgc.rows(net, n)
    pol = policy_for(net)
    value = run(pol, x, a, w, t)["value"].numpy()
    terms = [run(pol, x, a, *one_live(w, t, value, (i,)))["grads"] for i in pair]
    w2, t2 = one_live(w, t, value, pair)
    for chunk_rows in (0, 128):
        got = run(pol, x, a, w2, t2, chunk_rows=chunk_rows)["grads"]
        for k in pgc.GRAD_NAMES:
            assert same(got[k], terms[0][k] + terms[1][k]), (k, chunk_rows)  # (a two-term fp32 sum has no order)
            assert bool((terms[0][k] != 0).any()) or net == (1, 1, 1, 1, 5)
    pol.close()


# ------------------------------------------------------------------ 3. chunking changes no bit
def test_chunking_and_rerunning_change_no_bit():
    n = 600
    x = pgc.features("ref", n)
    a, w, t = pgc.rows("ref", n)
    pol = policy_for("ref")
    plan = (ctypes.c_int32 * 5)()
    _lib.check(_lib.load().wab_debug_policy_grad_plan(pol._p, 0, plan), "wab_debug_policy_grad_plan")
    assert plan[0] == 128 and plan[1] > 1 and plan[2] % 128 == 0 and plan[2] >= 600 and 0 < plan[3] <= 160 * 1024
    kw = dict(value_coef=0.5, entropy_coef=0.01)
    base = run(pol, x, a, w, t, **kw)
    assert same_result(base, run(pol, x, a, w, t, **kw))
    for chunk_rows in (128, 256):
        assert same_result(base, run(pol, x, a, w, t, chunk_rows=chunk_rows, **kw)), chunk_rows
    assert all(bool((base["grads"][k] != 0).any()) for k in pgc.GRAD_NAMES)
    with pytest.raises(ValueError):
        run(pol, x, a, w, t, chunk_rows=100)
    pol.close()


# ------------------------------------------------------------------ 4. against the contract
WORST = {}


@pytest.mark.parametrize("net", pgc.NETS, ids=str)
@pytest.mark.parametrize("n", pgc.ROWS)
def test_against_the_contract(net, n):
    x = pgc.features(net, n)
    a, w, t = pgc.rows(net, n)
    A = pgc.net_shape(net)[4]
    pol = policy.DevicePolicy(pgc.state_dict(net), env_for(A, n))
    worst = WORST.setdefault(str(net), {})
    for value_loss in ("smooth_l1", "mse"):
        for ec in (0.0, 0.01):
            ref, E = pgc.contract_and_cost(net, n, 0.5, ec, value_loss)
            got = run(pol, x, a, w, t, value_coef=0.5, entropy_coef=ec, value_loss=value_loss)
            check_gate(got, ref, E, "%s N=%d %s ec=%g" % (net, n, value_loss, ec), worst)
    if isinstance(net, tuple):  # nothing to round: wab_policy_act's bits, and the contract's
        value = torch.empty(n, device=DEV)
        pol.act(dev(x, torch.float32), value=value)
        assert same(got["value"], value.cpu())
        assert same(got["value"].double(), ref["value"])
    print("worst ratios so far, %s: %s" % (net, "  ".join("%s %.4f" % kv for kv in sorted(worst.items()))))
    pol.close()


# ------------------------------------------------------------------ 5. edges
def test_no_rows_give_zeros():
    pol = policy_for("odd")
    got = run(pol, np.zeros((0, 37), np.float32), np.zeros(0, np.int8), np.zeros(0, np.float32), np.zeros(0, np.float32))
    assert all(bool((got["grads"][k] == 0).all()) for k in pgc.GRAD_NAMES)
    assert all(float(got[k]) == 0.0 for k in ("loss", "loss_policy", "loss_value", "entropy"))
    assert got["logp"].shape == (0,)
    pol.close()


def model_of(net, seed=0):
    spec = importlib.util.spec_from_file_location("train_actor_critic", os.path.join(REPO, "examples",
                                                                                   "train_actor_critic.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    torch.manual_seed(seed)
    shape = pgc.net_shape(net)
    if shape[1:4] == (128, 150, 128):
        return mod, mod.Policy(shape[0], shape[4]).to(DEV)
    return mod, None


def test_accumulate_mean_views_and_into_model():
    n, T = 258, 2
    x = pgc.features("ref", n)
    a, w, t = pgc.rows("ref", n)
    _, model = model_of("ref")
    env = env_for(5, 128)
    pol = policy.DevicePolicy(model, env)
    args = [dev(x, torch.float32), dev(a, torch.int8), dev(w, torch.float32), dev(t, torch.float32)]
    once = pol.loss_and_grad(*args, entropy_coef=0.01)
    assert all(p.grad is None for p in model.parameters())
    # [T, B, F] is its [T B, F] view
    r3 = pol.loss_and_grad(args[0].view(T, n // T, -1), *[v.view(T, n // T) for v in args[1:]], entropy_coef=0.01,
                           return_rows=True)
    assert all(same(r3["grads"][k], once["grads"][k]) for k in pgc.GRAD_NAMES) and same(r3["loss"], once["loss"])
    assert r3["logp"].shape == (T, n // T)
    # into=model allocates and fills .grad; accumulate adds: twice is 2 x once up to the add's rounding
    out = pol.loss_and_grad(*args, entropy_coef=0.01, into=model)
    assert "grads" not in out
    sd = dict(model.named_parameters())
    for k in pgc.GRAD_NAMES:
        assert same(sd[k].grad, once["grads"][k]), k
    pol.loss_and_grad(*args, entropy_coef=0.01, into=model, accumulate=True)
    for k in pgc.GRAD_NAMES:
        assert same(sd[k].grad, once["grads"][k] + once["grads"][k]), k  # (x + x is exact)
    # mean: scale 1 / N on the total and the gradients, the parts unscaled
    mean = pol.loss_and_grad(*args, entropy_coef=0.01, reduction="mean")
    inv = np.float32(1.0 / n)
    for k in pgc.GRAD_NAMES:
        ratio = mean["grads"][k].double() - once["grads"][k].double() * float(inv)
        assert float(ratio.abs().max()) <= 2.0 ** -22 * float(once["grads"][k].abs().max()) * float(inv), k
    assert same(mean["loss_policy"], once["loss_policy"])
    assert abs(float(mean["loss"]) - float(once["loss"]) / n) <= 1e-6 * abs(float(once["loss"]) / n)
    # requirements of into=: parameters on the policy's device, all ten present
    with pytest.raises(ValueError):
        pol.loss_and_grad(*args, into=model_of("ref")[1].cpu())
    with pytest.raises(ValueError):
        pol.loss_and_grad(*args, into=torch.nn.Linear(449, 128).to(DEV))
    pol.close()


def test_out_of_range_action_is_reported_and_left_out():
    n = 130
    x = pgc.features("odd", n)
    a, w, t = pgc.rows("odd", n)
    pol = policy_for("odd")
    a_bad = a.copy()
    a_bad[129] = 6
    args = [dev(x, torch.float32), dev(a_bad, torch.int8), dev(w, torch.float32), dev(t, torch.float32)]
    bad = pol.loss_and_grad(*args)
    with pytest.raises(IndexError, match="1 rows"):
        pol.check()
    good = pol.loss_and_grad(args[0][:129], args[1][:129], args[2][:129], args[3][:129])
    pol.check()
    assert all(same(bad["grads"][k], good["grads"][k]) for k in pgc.GRAD_NAMES) and same(bad["loss"], good["loss"])
    pol.close()


def test_one_training_step_and_a_captured_update():
    B, T = 256, 16
    mod, model = model_of("ref", seed=3)
    env = BatchedWolvesAndBushesEnv(dict(pc.OPTS_REF), num_envs=B, seed=pc.SEED, device=DEV)
    wrapper = PragmaticObsWrapper(env)
    wrapper.reset()
    opt = torch.optim.SGD(model.parameters(), lr=1e-2)
    pol = policy.DevicePolicy(model, env)
    before = [p.detach().clone() for p in model.parameters()]
    out = mod.update(wrapper, pol, model, opt, T, entropy_coef=0.01)
    pol.check()
    assert np.isfinite(float(out["loss"])) and float(out["entropy"]) > 0
    assert all(not torch.equal(p.detach(), q) for p, q in zip(model.parameters(), before))
    feats = wrapper.features.clone()
    assert int(pol.act(feats).min()) >= 0
    # the update's device work (loss_and_grad into .grad) captured in a graph replays to the same bits
    r = wrapper.rollout_policy(pol, T, bootstrap_value=True, gae_lambda=0.95, whiten=True)
    args = (r["features"], r["actions"], r["advantage"], r["target"])
    eager = pol.loss_and_grad(*args, into=model, reduction="mean")
    want = [p.grad.clone() for p in model.parameters()]
    want_loss = eager["loss"].clone()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        cap = pol.loss_and_grad(*args, into=model, reduction="mean")
    for _ in range(2):
        for p in model.parameters():
            p.grad.fill_(7.0)
        g.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(p.grad, q) for p, q in zip(model.parameters(), want))
        assert torch.equal(cap["loss"], want_loss)
    pol.close()
