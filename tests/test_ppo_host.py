"""wab_policy_grad_ppo's numeric contract on the CPU (wab_gym_amd.policy.reference_ppo_loss_and_grad):
the hand-written clipped loss and backward pass against float64 autograd of the textbook formula
on the straight-through forward, the anchor old_logp = logp, the test rows' own guarantees
(tests/ppo_cases.py), the float32 head predictor and the tie builders that
tests/test_gpu_ppo_edges.py relies on, the header and its mirror at ABI 14, and
ppo_loss_and_grad's argument checks that need no device."""
import os
import re

import numpy as np
import pytest
import torch

import policy_cases as pc
import policy_grad_cases as pgc
import ppo_cases as ppc
from wab_gym_amd import _lib, policy

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "wab.h")


def straight_through_ppo_autograd(sd, c, clip, value_clip, value_coef, entropy_coef, value_loss, scale):
    """float64 autograd of the textbook clipped loss on reference_forward with every bf16
    rounding given derivative 1 (tests/test_policy_grad_host.py's straight_through_autograd)."""
    p = {k: v.detach().double().requires_grad_(True) for k, v in sd.items()}

    def bfq(x):
        return x + (x.detach().float().to(torch.bfloat16).double() - x.detach())

    slope = float(np.float32(0.01))
    x = torch.as_tensor(c["x"]).float().to(torch.bfloat16).double()
    for i, name in enumerate(policy.LAYERS[:3]):
        z = x @ bfq(p[name + ".weight"]).T + p[name + ".bias"]
        y = torch.where(z >= 0, z, z * slope)
        if i == 2:
            y = y.clamp(-4.0, 4.0)
        x = bfq(y)
    logits = x @ bfq(p["action_head.weight"]).T + p["action_head.bias"]
    v = (x @ bfq(p["value_head.weight"]).T + p["value_head.bias"])[:, 0]
    logp_all = torch.log_softmax(logits, dim=-1)
    a = torch.as_tensor(c["a"]).long()
    A, t = torch.as_tensor(c["adv"]).double(), torch.as_tensor(c["t"]).double()
    olp, ov = torch.as_tensor(c["old_logp"]).double(), torch.as_tensor(c["old_value"]).double()
    logp = logp_all.gather(1, a[:, None])[:, 0]
    H = -(logp_all.exp() * logp_all).sum(dim=-1)
    r = torch.exp(logp - olp)
    lo, hi = float(np.float32(1.0) - np.float32(clip)), float(np.float32(1.0) + np.float32(clip))
    lpol = -torch.min(r * A, torch.clamp(r, lo, hi) * A).sum()

    def l(e):
        return 0.5 * e * e if value_loss == "mse" else torch.where(e.abs() < 1, 0.5 * e * e, e.abs() - 0.5)

    lv = l(v - t)
    if value_clip:
        cc = float(np.float32(value_clip))
        lv = torch.max(lv, l(ov + torch.clamp(v - ov, -cc, cc) - t))
    parts = (lpol, lv.sum(), H.sum())
    total = scale * (parts[0] + value_coef * parts[1] - entropy_coef * parts[2])
    total.backward()
    return parts + (total,), {k: p[k].grad for k in pgc.GRAD_NAMES}, logp, v, H, r


@pytest.mark.parametrize("net", pgc.NETS, ids=str)
@pytest.mark.parametrize("value_loss", ("smooth_l1", "mse"))
@pytest.mark.parametrize("entropy_coef", (0.0, 0.01))
@pytest.mark.parametrize("value_clip", (None, ppc.VALUE_CLIP), ids=("vclip_off", "vclip_on"))
def test_contract_is_the_textbook_gradient(net, value_loss, entropy_coef, value_clip):
    n = 129
    sd, c = pgc.state_dict(net), ppc.case(net, n)
    got = policy.reference_ppo_loss_and_grad(sd, c["x"], c["a"], c["adv"], c["t"], c["old_logp"], ppc.CLIP,
                                             c["old_value"], value_clip, 0.5, entropy_coef, value_loss, 0.25,
                                             round_grads=False)
    loss, grads, logp, v, H, r = straight_through_ppo_autograd(sd, c, ppc.CLIP, value_clip, 0.5, entropy_coef,
                                                               value_loss, 0.25)
    for k in pgc.GRAD_NAMES:
        ref = grads[k].detach()
        assert tuple(got["grads"][k].shape) == tuple(sd[k].shape), k
        err = float((got["grads"][k] - ref).abs().max())
        assert err <= 1e-10 * max(float(ref.abs().max()), 1e-300), (k, err)
        assert bool((ref != 0).any()) or net == (1, 1, 1, 1, 5), k
    for g, rr in zip(got["loss"], loss):
        assert abs(float(g) - float(rr.detach())) <= 1e-10 * abs(float(rr.detach()))
    for g, rr in ((got["logp"], logp), (got["value"], v), (got["entropy"], H), (got["ratio"], r)):
        assert float((g - rr.detach()).abs().max()) <= 1e-10 * float(rr.detach().abs().max())


@pytest.mark.parametrize("net", pgc.NETS, ids=str)
def test_old_logp_equal_to_logp_is_the_a2c_gradient(net):
    n = 129
    sd, c = pgc.state_dict(net), ppc.case(net, n)
    a2c = policy.reference_loss_and_grad(sd, c["x"], c["a"], c["adv"], c["t"], 0.5, 0.01)
    got = policy.reference_ppo_loss_and_grad(sd, c["x"], c["a"], c["adv"], c["t"], a2c["logp"], ppc.CLIP, None, None,
                                             0.5, 0.01)
    for k in pgc.GRAD_NAMES:
        assert torch.equal(got["grads"][k], a2c["grads"][k]), k
    assert [float(x) for x in got["ppo"]] == [0.0, 0.0, 0.0, float(n)]
    assert bool((got["ratio"] == 1.0).all()) and not bool(got["clipped"].any())
    assert float(got["loss"][0]) == -float(torch.as_tensor(c["adv"]).double().sum())


@pytest.mark.parametrize("net", pgc.NETS, ids=str)
@pytest.mark.parametrize("n", (129, 257))
def test_case_rows_cover_every_kind_and_the_pool_suffices(net, n):
    c = ppc.case(net, n)  # (asserts that the pool suffices)
    kept, pool = c["kept_of_pool"]
    print("%s n=%d: %d of %d pool rows clear of the PPO kinks" % (net, n, kept, pool))
    assert c["x"].shape == (n, pgc.net_shape(net)[0]) and kept >= n
    ref = policy.reference_ppo_loss_and_grad(pgc.state_dict(net), c["x"], c["a"], c["adv"], c["t"], c["old_logp"],
                                             ppc.CLIP, c["old_value"], ppc.VALUE_CLIP)
    r, cl, vcl = ref["ratio"].numpy(), ref["clipped"].numpy(), ref["value_clipped"].numpy()
    clamped = np.abs(ref["value"].numpy() - c["old_value"].astype(np.float64)) > float(np.float32(ppc.VALUE_CLIP))
    assert (cl & (r > ppc.HI)).any() and (cl & (r < ppc.LO)).any() and (~cl & (r != 1.0)).any()
    assert vcl.any() and (clamped & ~vcl).any()
    assert [float(x) for x in ref["ppo"]][0::2] == [float(cl.sum()), float(vcl.sum())]


# ------------------------------------------------------------------ the float32 head predictor (ppc.predict_head)
@pytest.mark.parametrize("net", pgc.NETS, ids=str)
@pytest.mark.parametrize("n", ppc.ROWS)
@pytest.mark.parametrize("value_loss", ("smooth_l1", "mse"))
def test_predictor_decides_as_the_contract_on_clear_rows(net, n, value_loss):
    """The case rows are 8 E clear of every kink, so float32 and float64 decide alike."""
    c = ppc.case(net, n)
    ref, _ = ppc.contract_and_cost(net, n, 0.5, 0.0, value_loss)
    f32 = [ref[k].numpy().astype(np.float32) for k in ("logp", "value", "ratio")]
    p = ppc.predict_head(*f32, c["adv"], c["t"], c["old_logp"], c["old_value"], ppc.CLIP, ppc.VALUE_CLIP, value_loss)
    assert np.array_equal(p["clipped"], ref["clipped"].numpy())
    assert np.array_equal(p["value_clipped"], ref["value_clipped"].numpy())
    assert [p["n_clipped"], p["n_value_clipped"]] == [int(ref["ppo"][0]), int(ref["ppo"][2])]
    want = {"lpol": float(ref["loss"][0]), "lv": float(ref["loss"][1]), "k3": float(ref["ppo"][1]),
            "ratio": float(ref["ppo"][3])}
    for k in ("lpol", "lv", "ratio"):
        assert abs(p["sums"][k] - want[k]) <= 1e-6 * abs(want[k]), (k, p["sums"][k], want[k])
    # k3 = expm1(d) - d is about d^2 / 2, and rounding logp to float32 moves d by up to 2^-24 |logp|
    # (the float32 difference adds 2^-24 |d|), so k3 by |expm1(d)| times that: relative to k3 that is
    # 2^-23 |logp| / |d|, which at d = 0.0625 is already 2e-6.  So 1e-6 of the sum holds where rows
    # with |d| = 0.5 carry the sum, which is every case of 128 rows and more (at most 7.9e-8), and
    # cannot hold for a single row of small d: the four random-weight single rows give 1.8e-6
    # ((449,128,150,128,5)), 1.6e-6 (ref), 2.9e-6 (odd) and, with delta = 0 where the contract's own
    # d is the 1e-8 that rounding removes, 1 (wide).  Those are held to the mean-value bound
    # instead, per row, summed: |k3'| = |expm1| <= expm1(|d| + delta) between the two d, delta the move
    d64 = np.abs(p["d"].astype(np.float64))
    delta = 2.0 ** -24 * (np.abs(f32[0].astype(np.float64)) + d64)
    room = float((np.expm1(d64 + delta) * delta).sum())
    err = abs(p["sums"]["k3"] - want["k3"])
    print("%s n=%d k3: err %.3e, 1e-6 of the sum %.3e, rounding's room %.3e" % (net, n, err, 1e-6 * abs(want["k3"]), room))
    assert err <= 1e-6 * abs(want["k3"]) or (n == 1 and err <= 1.01 * room), (p["sums"]["k3"], want["k3"], room)
    # the effective weight and the value gradient are the contract's, to float32's rounding
    w_ref = np.where(ref["clipped"].numpy(), 0.0, ref["ratio"].numpy() * c["adv"])
    assert np.abs(p["w_eff"] - w_ref).max() <= 2.0 ** -22 * max(np.abs(w_ref).max(), 1e-30)
    off = ppc.predict_head(*f32, c["adv"], c["t"], c["old_logp"], None, ppc.CLIP, None, value_loss)
    assert off["n_value_clipped"] == 0 and not off["outside"].any() and np.array_equal(off["lv"], off["l1"])


def one_row(ratio=1.0, adv=1.0, value=0.0, target=0.0, old_value=0.0, clip=0.25, value_clip=0.25,
            value_loss="smooth_l1", logp=-1.0, old_logp=-1.0):
    f = lambda x: np.array([x], np.float32)
    return ppc.predict_head(f(logp), f(value), f(ratio), f(adv), f(target), f(old_logp), f(old_value), clip, value_clip,
                            value_loss)


def test_predictor_is_strict_on_every_tie():
    """include/wab.h: clipped = (A > 0 && r > hi) || (A < 0 && r < lo); |u| <= c is inside;
    value_clipped = l2 > l1; smooth_l1 is quadratic for |d| < 1.  One row per tie and its
    neighbours one unit in the last place away."""
    up, down = (lambda x: float(ppc.move_units(np.float32(x), 1))), (lambda x: float(ppc.move_units(np.float32(x), -1)))
    hi, lo = 1.25, 0.75
    # r == hi, r == lo: not clipped, the weight is r A; one unit past: clipped, weight 0, the loss at the bound
    for r, adv, clipped in ((hi, 2.0, False), (up(hi), 2.0, True), (down(hi), 2.0, False), (up(hi), -2.0, False),
                            (lo, -2.0, False), (down(lo), -2.0, True), (up(lo), -2.0, False), (down(lo), 2.0, False)):
        p = one_row(ratio=r, adv=adv)
        assert bool(p["clipped"][0]) == clipped, (r, adv)
        assert p["w_eff"][0] == (0.0 if clipped else np.float32(r) * np.float32(adv))
        assert p["lpol"][0] == (-(np.float32(adv) * np.float32(hi if adv > 0 else lo)) if clipped
                                else -(np.float32(r) * np.float32(adv)))
    # A == 0, of either sign, outside the clip range: not clipped, weight (-)0
    for r in (2.0, 0.5):
        for adv in (0.0, -0.0):
            p = one_row(ratio=r, adv=adv)
            assert not p["clipped"][0] and p["w_eff"][0] == 0.0 and p["n_clipped"] == 0
            assert np.signbit(p["w_eff"][0]) == np.signbit(np.float32(adv))
    # |u| == c: inside, the plain loss (old_value 0, c = 0.25: u = value, exact)
    for v, outside in ((0.25, False), (up(0.25), True), (-0.25, False), (down(-0.25), True), (down(0.25), False)):
        p = one_row(value=v, target=v, value_clip=0.25)  # (l1 = 0, l2 = l(+-c - v) > 0 once outside)
        assert bool(p["outside"][0]) == outside and bool(p["value_clipped"][0]) == outside, v
        assert p["dv"][0] == 0.0
    # l2 == l1: value 1, old_value 0, c 0.25 -> vc 0.25; the target at the midpoint 0.625 ties, and
    # the loss and its gradient are the unclipped row's
    for value_loss in ("smooth_l1", "mse"):
        for t, vcl in ((0.625, False), (up(0.625), True), (down(0.625), False)):
            p = one_row(value=1.0, target=t, value_loss=value_loss)
            assert p["outside"][0] and bool(p["value_clipped"][0]) == vcl, (value_loss, t)
            assert (p["l1"][0] == p["l2"][0]) == (t == 0.625)
            assert p["dv"][0] == (0.0 if vcl else np.float32(1.0) - np.float32(t))
            assert p["lv"][0] == max(p["l1"][0], p["l2"][0])
    # |vc - t| == 1 and |v - t| == 1: linear from 1 on (0.5 either way at 1), quadratic one unit below
    for vc_t, quad in ((1.0, False), (down(1.0), True), (up(1.0), False), (-1.0, False), (up(-1.0), True)):
        p = one_row(value=4.0, old_value=-0.25, target=-vc_t)  # vc = 0, vc - t = vc_t exactly
        want = np.float32(0.5) * np.float32(vc_t) * np.float32(vc_t) if quad else np.abs(np.float32(vc_t)) - np.float32(0.5)
        assert p["l2"][0] == want, vc_t
        q = one_row(value=vc_t, target=0.0, value_clip=None)
        assert q["l1"][0] == want and q["dv"][0] == (np.float32(vc_t) if quad else np.sign(np.float32(vc_t)))
        assert one_row(value=vc_t, target=0.0, value_clip=None, value_loss="mse")["l1"][0] \
            == np.float32(0.5) * np.float32(vc_t) * np.float32(vc_t)
    # the clamp, by comparisons: +-30 exactly stays, beyond is cut, a NaN stays a NaN
    for d, want in ((30.0, 30.0), (31.0, 30.0), (np.inf, 30.0), (-30.0, -30.0), (-1000.0, -30.0), (-np.inf, -30.0),
                    (down(30.0), down(30.0))):
        assert one_row(logp=0.0, old_logp=-d)["d"][0] == np.float32(want)
    p = one_row(old_logp=np.nan, ratio=np.nan, adv=2.0)
    assert np.isnan(p["d"][0]) and not p["clipped"][0] and np.isnan(p["w_eff"][0]) and np.isnan(p["sums"]["k3"])


@pytest.mark.parametrize("net", ("ref", "odd"))
def test_tie_builders_reach_every_group_from_the_contracts_values(net):
    """tests/test_gpu_ppo_edges.py builds its rows from the device's bits with these; here from the
    contract's logp and value rounded to float32, numpy's float32 exp for the ratio."""
    n = 257
    a, w, t = pgc.rows(net, n)
    ref = policy.reference_loss_and_grad(pgc.state_dict(net), pgc.features(net, n), a, w, t)
    logp, value = (ref[k].numpy().astype(np.float32) for k in ("logp", "value"))
    for bound, upper in ((1.25, True), (0.75, False)):
        old = ppc.tie_old_logp(logp, bound)
        ratio = np.exp(logp - old)
        assert ratio.dtype == np.float32
        adv = ppc.tie_advantages(ratio)
        assert [(adv > 0).sum(), (adv < 0).sum(), (adv == 0).sum()] == [103, 103, 51] and np.signbit(adv[adv == 0]).any()
        b = ppc.tie_bound(ratio, adv, upper)
        clip = ppc.clip_for_bound(b, upper)
        assert (np.float32(1.0) + np.float32(clip) if upper else np.float32(1.0) - np.float32(clip)) == b
        for rows in (adv > 0, adv < 0, adv == 0):
            assert min(ppc.groups(ratio[rows], b)) >= 1, (bound, ppc.groups(ratio[rows], b))
    for c in (0.25, 0.2):
        for value_loss in ("smooth_l1", "mse"):
            ov, t2, info = ppc.tie_value_rows(value, t, c, value_loss)
            p = ppc.predict_head(logp, value, np.ones(n, np.float32), w, t2, logp, ov, 0.2, c, value_loss)
            out = p["outside"]
            print(net, c, value_loss, info, "l2 <, ==, > l1:", ppc.groups(p["l2"][out], p["l1"][out]))
            assert min(info["u"]) >= 8 and info["u"][2] == out.sum()
            assert min(ppc.groups(p["l2"][out], p["l1"][out])) >= 8
            assert min(ppc.groups(np.abs(value - t2), np.float32(1.0))) >= 2


def test_header_and_mirror_carry_the_ppo_abi():
    src = open(HEADER).read()
    version = int(re.search(r"#define\s+WAB_ABI_VERSION\s+(\d+)", src).group(1))
    assert version == _lib.ABI_VERSION == 14
    for name in ("wab_policy_grad_ppo", "wab_policy_evaluate"):
        assert re.search(r"\b%s\(" % name, src) and name in _lib.EXPORTED, name
    fields = re.search(r"typedef struct wab_ppo_config \{(.*?)\} wab_ppo_config;", src, re.S).group(1)
    assert re.findall(r"float\s+(\w+);", fields) == [f[0] for f in _lib.WabPpoConfig._fields_] == ["clip", "value_clip"]
    # wab_policy_loss is what it was
    fields = re.search(r"typedef struct wab_policy_loss \{(.*?)\} wab_policy_loss;", src, re.S).group(1)
    assert re.findall(r"(?:float|int32_t)\s+(\w+);", fields) == [f[0] for f in _lib.WabPolicyLoss._fields_]


def test_ppo_loss_and_grad_argument_checks():
    shape = pc.NET_ODD
    x = torch.zeros((4, 3, 37))
    a = torch.zeros((4, 3), dtype=torch.int8)
    w, t, olp, ov = (torch.zeros((4, 3)) for _ in range(4))
    assert policy.check_ppo_args(shape, x, a, w, t, olp) == 12
    assert policy.check_ppo_args(shape, x, a, w, t, olp, 0.1, ov, 0.2, "mse", "mean") == 12
    assert policy.check_ppo_args(shape, x, a, w, t, olp, value_clip=0.0) == 12  # (off: no old_value needed)
    assert policy.check_ppo_args(shape, x[1:3], a[1:3], w[1:3], t[1:3], olp[1:3]) == 6  # a minibatch is a view
    bad = [
        dict(clip=0.0), dict(clip=1.0), dict(clip=float("nan")), dict(clip=-0.2), dict(value_clip=float("nan")),
        dict(value_clip=0.2), dict(value_clip=0.2, old_value=ov.double()), dict(value_clip=0.2, old_value=ov[:, :2]),
        dict(old_logp=None), dict(old_logp=olp.double()), dict(old_logp=olp.view(12)),
        dict(old_logp=olp.transpose(0, 1)), dict(advantage=w.double()), dict(value_loss="huber"),
        dict(accumulate=True),
    ]
    for kw in bad:
        args = dict(features=x, actions=a, advantage=w, target=t, old_logp=olp)
        args.update(kw)
        with pytest.raises(ValueError):
            policy.check_ppo_args(shape, **args)
    with pytest.raises(ValueError):
        policy.reference_ppo_loss_and_grad(pc.weights("odd"), x.view(12, 37), a.view(12), w.view(12), t.view(12),
                                           olp.view(12), value_clip=0.2)
