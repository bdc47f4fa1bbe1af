"""wab_policy_grad's numeric contract on the CPU (wab_gym_amd.policy.reference_loss_and_grad):
the hand-written backward pass against float64 autograd of the straight-through forward, the
test inputs' own guarantees, what the bf16 contract costs against stock fp32 autograd (E_grad,
DESIGN.md's table), and loss_and_grad's argument checks that need no device."""
import re
import os

import numpy as np
import pytest
import torch

import policy_cases as pc
import policy_grad_cases as pgc
from wab_gym_amd import _lib, policy

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "wab.h")


def straight_through_autograd(sd, feats, actions, weight, target, value_coef, entropy_coef, value_loss, scale):
    """float64 autograd of reference_forward with every bf16 rounding given derivative 1."""
    p = {k: v.detach().double().requires_grad_(True) for k, v in sd.items()}

    def bfq(x):
        return x + (x.detach().float().to(torch.bfloat16).double() - x.detach())

    slope = float(np.float32(0.01))
    x = torch.as_tensor(feats).float().to(torch.bfloat16).double()
    for i, name in enumerate(policy.LAYERS[:3]):
        z = x @ bfq(p[name + ".weight"]).T + p[name + ".bias"]
        y = torch.where(z >= 0, z, z * slope)
        if i == 2:
            y = y.clamp(-4.0, 4.0)
        x = bfq(y)
    logits = x @ bfq(p["action_head.weight"]).T + p["action_head.bias"]
    v = (x @ bfq(p["value_head.weight"]).T + p["value_head.bias"])[:, 0]
    logp_all = torch.log_softmax(logits, dim=-1)
    a = torch.as_tensor(actions).long()
    w, t = torch.as_tensor(weight).double(), torch.as_tensor(target).double()
    logp = logp_all.gather(1, a[:, None])[:, 0]
    H = -(logp_all.exp() * logp_all).sum(dim=-1)
    d = v - t
    lv = 0.5 * d * d if value_loss == "mse" else torch.where(d.abs() < 1, 0.5 * d * d, d.abs() - 0.5)
    parts = (-(w * logp).sum(), lv.sum(), H.sum())
    total = scale * (parts[0] + value_coef * parts[1] - entropy_coef * parts[2])
    total.backward()
    return parts + (total,), {k: p[k].grad for k in pgc.GRAD_NAMES}, logp, v, H


@pytest.mark.parametrize("net", pgc.NETS, ids=str)
@pytest.mark.parametrize("value_loss", ("smooth_l1", "mse"))
@pytest.mark.parametrize("entropy_coef", (0.0, 0.01))
def test_contract_is_the_straight_through_gradient(net, value_loss, entropy_coef):
    n = 129
    sd, x = pgc.state_dict(net), pgc.features(net, n)
    a, w, t = pgc.rows(net, n)
    got = policy.reference_loss_and_grad(sd, x, a, w, t, 0.5, entropy_coef, value_loss, 0.25, round_grads=False)
    loss, grads, logp, v, H = straight_through_autograd(sd, x, a, w, t, 0.5, entropy_coef, value_loss, 0.25)
    for k in pgc.GRAD_NAMES:
        ref = grads[k].detach()
        assert tuple(got["grads"][k].shape) == tuple(sd[k].shape), k
        err = float((got["grads"][k] - ref).abs().max())
        assert err <= 1e-10 * max(float(ref.abs().max()), 1e-300), (k, err)
        assert bool((ref != 0).any()) or net == (1, 1, 1, 1, 5), k
    for g, r in zip(got["loss"], loss):
        assert abs(float(g) - float(r.detach())) <= 1e-10 * abs(float(r.detach()))
    for g, r in ((got["logp"], logp), (got["value"], v), (got["entropy"], H)):
        assert float((g - r.detach()).abs().max()) <= 1e-10 * float(r.detach().abs().max())


def test_rounded_gradients_differ_and_scale_is_applied_once():
    sd, x = pgc.state_dict("odd"), pgc.features("odd", 128)
    a, w, t = pgc.rows("odd", 128)
    r1 = policy.reference_loss_and_grad(sd, x, a, w, t, scale=1.0)
    r4 = policy.reference_loss_and_grad(sd, x, a, w, t, scale=0.25)
    ru = policy.reference_loss_and_grad(sd, x, a, w, t, round_grads=False)
    for k in pgc.GRAD_NAMES:
        assert torch.equal(r4["grads"][k], r1["grads"][k] * 0.25), k
    assert any(not torch.equal(r1["grads"][k], ru["grads"][k]) for k in pgc.GRAD_NAMES)
    assert float(r4["loss"][3]) == 0.25 * float(r1["loss"][3])
    assert float(r4["loss"][0]) == float(r1["loss"][0])


@pytest.mark.parametrize("net", pgc.EXACT_NETS, ids=str)
@pytest.mark.parametrize("n", pgc.ROWS)
def test_exact_nets_stay_exact_on_these_rows(net, n):
    assert pc.exact_certificate(pgc.state_dict(net), pgc.features(net, n)) > 0


@pytest.mark.parametrize("net", pgc.RANDOM_NETS)
@pytest.mark.parametrize("n", pgc.ROWS)
def test_pool_has_enough_rows_clear_of_the_kinks(net, n):
    x = pgc.features(net, n)  # (asserts that the pool suffices)
    assert x.shape == (n, pgc.net_shape(net)[0])
    assert (pgc.kink_margins(pgc.state_dict(net), x) > 0).all()
    a, w, t = pgc.rows(net, n)
    if n >= 127:
        _, v = policy.reference_forward(pgc.state_dict(net), x)
        d = np.abs(v.numpy() - t)
        assert (d < 1).any() and (d > 1).any() and (w > 0).any() and (w < 0).any() and (w == 0).any()
        hidden = []
        policy.reference_forward(pgc.state_dict(net), x, hidden=hidden)
        assert all(bool((z < 0).any()) and bool((z > 0).any()) for z, _ in hidden)


def test_what_the_contract_costs_against_fp32_autograd():
    """E_grad per tensor for the reference net (printed: DESIGN.md's table): positive and finite.
    (It is not small against the gradient: with unrounded weights some units sit on the other
    side of a kink, and their whole term differs.)"""
    for n in pgc.ROWS:
        ref, E = pgc.contract_and_cost("ref", n)
        print("ref net N=%d: " % n + "  ".join("%s %.3e" % (k, E[k]) for k in pgc.GRAD_NAMES))
        print("          losses: " + "  ".join("%s %.3e" % (k, E[k]) for k in
                                               ("loss_policy", "loss_value", "entropy", "logp", "value", "entropy_rows")))
        for k in pgc.GRAD_NAMES:
            assert 0 < E[k] < float("inf"), (n, k, E[k])


def test_slab_table_is_the_plans_formula():
    """tests/test_gpu_policy_grad_slabs.py builds every N from S: the table, the formula's mirror
    and the header's constants agree, and each N puts the blocks where its test says."""
    tasks = {(1, 1, 1, 1, 5): 4, (17, 33, 33, 33, 5): 7, "odd": 6, "ref": 35, (449, 129, 150, 128, 6): 50, "wide": 41}
    for net, S in pgc.SLABS.items():
        assert pgc.plan_tasks(net) == tasks[net] and pgc.plan_slabs(net) == S, net
        n = pgc.fold_rows_n(S)
        live = pgc.fold_live_rows(S)
        assert [b for b, _ in live] == [0, S, 2 * S, 1, S + 1, 5, (n - 1) // 128] and live[-1][1] == n - 1
        assert all(i // 128 == b for b, i in live) and {i % 128 for _, i in live} >= {0, 31, 32, 127}
        blocks = (pgc.two_per_slab_n(S) + 127) // 128
        assert min(len(range(s, blocks, S)) for s in range(S)) == 2
    src = open(os.path.join(os.path.dirname(HEADER), "..", "wab_gym_amd", "csrc", "wab_policy_grad.h")).read()
    assert re.search(r"kGradMaxSlabs = 64;", src) and re.search(r"int s = \(2048 \+ t - 1\) / t;", src)
    assert re.search(r"kGradDefaultChunk = 32768;", src)


def test_fold_orders_of_the_slab_cases():
    """pgc.fold on terms whose three orders give three different fp32 results."""
    S, e = 3, np.float32(2.0 ** -24)
    one = np.float32(1.0)
    # slab 0 holds blocks 0, 3, 6; slab 1 block 1
    terms = {0: np.array([one, one]), 3: np.array([e, e]), 6: np.array([e, -one]), 1: np.array([0, e])}
    terms = {b: v.astype(np.float32) for b, v in terms.items()}
    up = np.float32(1.0 + 2.0 ** -23)
    # column 0: (1 + e) + e = 1, but (e + e) + 1 = 1 + 2^-23.  Column 1: slab 0 is ((1 + e) - 1) = 0 or
    # ((-1 + e) + 1) = e, then slab 1's e; in one accumulator 1 + e + e - 1 = 0
    assert np.array_equal(pgc.fold(terms, S, "slabs"), np.array([one, e], np.float32))
    assert np.array_equal(pgc.fold(terms, S, "descending"), np.array([up, 2 * e], np.float32))
    assert np.array_equal(pgc.fold(terms, S, "flat"), np.array([one, 0], np.float32))
    assert np.array_equal(pgc.fold(terms, S, "slabs", 0.25), np.array([0.25, e / 4], np.float32))
    assert pgc.fold_f64({0: 1.0, 3: 2.0 ** -53, 6: 2.0 ** -53, 1: 2.0 ** -52}, S) == 1.0 + 2.0 ** -52


def test_mfma_accumulate_model_gives_the_recorded_results():
    """pgc.mfma_accumulate against what the instruction returned on an MI355X
    (tests/golden/make_golden_mfma.py): every record, among them those where fl32(C + a b) is
    another float32, with C under the product and above it."""
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mfma_accumulate.npz"))
    c, a, b, d = z["c"], z["a"], z["b"], z["d"]
    assert len(c) >= 16384 and bool((c == 0).any())
    assert np.array_equal(pgc.mfma_accumulate(c, a, b), d)
    rne = (c.astype(np.float64) + a.astype(np.float64) * b.astype(np.float64)).astype(np.float32)
    ec, ep = np.frexp(c)[1], np.frexp(a)[1] + np.frexp(b)[1] - 1
    other = rne != d
    assert int((other & (ec < ep)).sum()) > 100 and int((other & (ec > ep + 8)).sum()) > 0
    # a product alone, or an accumulator alone, comes back as it is
    assert np.array_equal(pgc.mfma_accumulate(np.zeros_like(a), a, b), a * b)
    assert np.array_equal(pgc.mfma_accumulate(c, a, np.zeros_like(b)), c)


def test_header_and_mirror_carry_the_gradient_abi():
    src = open(HEADER).read()
    version = int(re.search(r"#define\s+WAB_ABI_VERSION\s+(\d+)", src).group(1))
    assert version == _lib.ABI_VERSION and version >= 12
    for name in ("wab_policy_grad_workspace", "wab_policy_grad", "wab_policy_grad_bad_actions",
                 "wab_debug_policy_grad_plan"):
        assert re.search(r"\b%s\(" % name, src) and name in _lib.EXPORTED, name
    fields = re.search(r"typedef struct wab_policy_loss \{(.*?)\} wab_policy_loss;", src, re.S).group(1)
    names = re.findall(r"(?:float|int32_t)\s+(\w+);", fields)
    assert names == [f[0] for f in _lib.WabPolicyLoss._fields_]


def test_loss_and_grad_argument_checks():
    shape = pc.NET_ODD
    x = torch.zeros((4, 3, 37))
    a = torch.zeros((4, 3), dtype=torch.int8)
    w, t = torch.zeros((4, 3)), torch.zeros((4, 3))
    assert policy.check_loss_args(shape, x, a, w, t) == 12
    assert policy.check_loss_args(shape, x.view(12, 37), a.view(12), w.view(12), t.view(12), "mse", "mean") == 12
    assert policy.check_loss_args(shape, x[:0], a[:0], w[:0], t[:0]) == 0
    bad = [
        dict(features=x.double()), dict(features=torch.zeros((4, 3, 36))), dict(features=torch.zeros(37)),
        dict(features=x.transpose(0, 1)), dict(actions=a.long()), dict(actions=a.view(12)),
        dict(weight=w.double()), dict(target=t[:, :2]), dict(value_loss="huber"), dict(reduction="none"),
        dict(accumulate=True),
    ]
    for kw in bad:
        args = dict(features=x, actions=a, weight=w, target=t)
        args.update(kw)
        with pytest.raises(ValueError):
            policy.check_loss_args(shape, **args)
    with pytest.raises(ValueError):
        policy.reference_loss_and_grad(pc.weights("odd"), x.view(12, 37), a.view(12), w.view(12), t.view(12),
                                       value_loss="huber")
