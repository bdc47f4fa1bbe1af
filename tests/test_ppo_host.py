"""wab_policy_grad_ppo's numeric contract on the CPU (wab_gym_amd.policy.reference_ppo_loss_and_grad):
the hand-written clipped loss and backward pass against float64 autograd of the textbook formula
on the straight-through forward, the anchor old_logp = logp, the test rows' own guarantees
(tests/ppo_cases.py), the header and its mirror at ABI 14, and ppo_loss_and_grad's argument checks
that need no device."""
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
