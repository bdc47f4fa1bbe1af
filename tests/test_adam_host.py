"""wab_policy_adam_step's host side, no GPU: the header and its ctypes mirror, the numeric
contract (wab_gym_amd.policy.reference_adam_step) against torch.optim.Adam, the order of the
norm's sum, the argument checks and the state_dict layout.

reference_adam_step and torch's float32 Adam round the same formulas in different orders, so
neither is compared with the other: both are compared with torch's Adam in float64 on the same
inputs, E_ref = max |reference - float64| against E_torch = max |torch float32 - float64| per
tensor after 10 steps, and E_ref <= 4 E_torch is required.  Measured (DESIGN.md,
"wab_policy_opt.hip"): E_torch and E_ref are 4e-9 to 1.4e-7, their ratio E_ref / E_torch between
0.50 and 1.26 and exactly 1 for most tensors (the two differ in few elements)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import adam_cases as ac
from wab_gym_amd import _lib, policy

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "wab.h")
STEPS = 10


def test_abi_of_header_and_mirror():
    src = open(HEADER).read()
    version = int(re.search(r"#define\s+WAB_ABI_VERSION\s+(\d+)", src).group(1))
    assert version == _lib.ABI_VERSION and version >= 13
    for name in ("wab_policy_adam_workspace", "wab_policy_adam_step"):
        assert re.search(r"\b%s\(" % name, src) and name in _lib.EXPORTED, name


def test_struct_layouts_match_c(tmp_path):
    mirrors = (("wab_adam_config", _lib.WabAdamConfig), ("wab_adam_state", _lib.WabAdamState))
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "%s"' % HEADER, "int main(void){"]
    for cname, mirror in mirrors:
        lines.append('printf("%%zu\\n", sizeof(%s));' % cname)
        lines += ['printf("%%zu\\n", offsetof(%s, %s));' % (cname, f) for f, _ in mirror._fields_]
    lines.append("return 0;}")
    prog = tmp_path / "layout.c"
    prog.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-o", str(exe), str(prog)], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    for cname, mirror in mirrors:
        assert out.pop(0) == ctypes.sizeof(mirror), cname
        for f, _ in mirror._fields_:
            assert out.pop(0) == getattr(mirror, f).offset, (cname, f)
    assert ctypes.sizeof(_lib.WabAdamState) == 48 and _lib.WabAdamState.grad_norm.offset == 32
    assert bytes(_lib.WabAdamState()) == bytes(48)  # a fresh optimizer is all-zero bytes


# ------------------------------------------------------------------ against torch's Adam
def torch_run(which, dtype, kind, steps, max_norm=0.0, grad_scale=1.0, **hyper):
    prm = [torch.tensor(p, dtype=dtype, requires_grad=True) for p in ac.params(which)]
    opt = kind(prm, **hyper)
    for k in range(steps):
        for p, g in zip(prm, ac.grads(which, k, grad_scale)):
            p.grad = torch.tensor(g, dtype=dtype)
        if max_norm > 0:
            torch.nn.utils.clip_grad_norm_(prm, max_norm)
        opt.step()
    return [p.detach().double().numpy() for p in prm]


CASES = {
    "adam": (torch.optim.Adam, dict(lr=1e-3), dict(lr=1e-3)),
    "adam_betas": (torch.optim.Adam, dict(lr=3e-4, betas=(0.8, 0.99), eps=1e-6),
                   dict(lr=3e-4, betas=(0.8, 0.99), eps=1e-6)),
    "l2": (torch.optim.Adam, dict(lr=1e-3, weight_decay=0.05), dict(lr=1e-3, weight_decay=0.05)),
    "adamw": (torch.optim.AdamW, dict(lr=1e-3, weight_decay=0.05), dict(lr=1e-3, weight_decay=0.05, decoupled=True)),
}


def gate(which, what, base, t32, ref):
    failed = []
    for name, b, t, r in zip(ac.NAMES, base, t32, ref):
        e_torch, e_ref = float(np.abs(t - b).max()), float(np.abs(r.astype(np.float64) - b).max())
        print("%s %s %s: E_torch %.3e  E_ref %.3e  ratio %.3f" % (which, what, name, e_torch, e_ref,
                                                                 e_ref / e_torch if e_torch else float(e_ref > 0)))
        if not e_ref <= 4.0 * e_torch:
            failed.append((name, e_ref, e_torch))
    assert not failed, (which, what, failed)


@pytest.mark.parametrize("which", ("ref", "odd"))
@pytest.mark.parametrize("case", sorted(CASES))
def test_reference_is_adam_within_fp32_rounding(which, case):
    kind, torch_kw, ref_kw = CASES[case]
    base = torch_run(which, torch.float64, kind, STEPS, **torch_kw)
    t32 = torch_run(which, torch.float32, kind, STEPS, **torch_kw)
    ref = ac.reference_run(which, STEPS, **ref_kw)[-1]
    assert ref[3]["step"] == STEPS and ref[3]["skipped"] == 0 and float(ref[3]["clip_scale"]) == 1.0
    assert any(float(np.abs(b - p).max()) > 1e-3 for b, p in zip(base, ac.params(which)))  # (it moved)
    gate(which, case, base, t32, [x for x in ref[0]])


@pytest.mark.parametrize("which", ("ref", "odd"))
def test_clip_is_clip_grad_norm(which):
    kw = dict(lr=1e-3)
    base = torch_run(which, torch.float64, torch.optim.Adam, STEPS, max_norm=0.5, grad_scale=1e3, **kw)
    t32 = torch_run(which, torch.float32, torch.optim.Adam, STEPS, max_norm=0.5, grad_scale=1e3, **kw)
    run = ac.reference_run(which, STEPS, grad_scale=1e3, max_grad_norm=0.5, **kw)
    assert all(0.0 < float(r[3]["clip_scale"]) < 1e-2 for r in run)
    gate(which, "clip", base, t32, run[-1][0])
    # the norm is torch's, the clip factor its rule
    g = ac.grads(which, STEPS - 1, 1e3)
    norm = float(torch.linalg.vector_norm(torch.cat([torch.tensor(x).double().reshape(-1) for x in g])))
    assert abs(float(run[-1][3]["grad_norm"]) - norm) <= 2.0 ** -23 * norm
    assert abs(float(run[-1][3]["clip_scale"]) - 0.5 / (norm + 1e-6)) <= 2.0 ** -23 * 0.5 / norm
    # inactive: a norm below the limit leaves c == 1 and the bits of the unclipped step
    loose = ac.reference_run(which, 2, max_grad_norm=1e9, **kw)[-1]
    plain = ac.reference_run(which, 2, **kw)[-1]
    assert float(loose[3]["clip_scale"]) == 1.0
    assert all(np.array_equal(a, b) for a, b in zip(loose[0], plain[0]))


# ------------------------------------------------------------------ the order of the norm's sum
def test_pair_tree_is_not_a_sequential_sum():
    q = np.array([1.0] + [2.0 ** -54] * 11)
    seq = 0.0
    for x in q:
        seq += x
    assert seq == 1.0  # every term is below half an ulp of the running sum
    # the tree over 16: [1, 2^-53 x 5, 0, 0] -> [1, 2^-52, 2^-52, 0] -> [1 + 2^-52, 2^-52] -> 1 + 2^-51
    assert policy.pair_tree_sum(q) == 1.0 + 2.0 ** -51
    assert policy.pair_tree_sum(np.array([3.0])) == 3.0 and policy.pair_tree_sum(np.array([1.0, 2.0, 4.0])) == 7.0
    # a non-finite gradient anywhere makes S non-finite, and only then
    big = np.full(1 << 12, np.finfo(np.float32).max, np.float64)
    assert np.isfinite(policy.pair_tree_sum(big * big))
    for bad in (np.nan, np.inf, -np.inf):
        big[-1] = bad
        assert not np.isfinite(policy.pair_tree_sum(big * big))


def test_non_finite_gradient_skips_the_reference_step():
    p, m, v, st = ac.reference_five("odd")[1]
    g = [x.copy() for x in ac.grads("odd", 2)]
    g[9][0] = np.nan
    p2, m2, v2, st2 = policy.reference_adam_step(p, g, m, v, st, max_grad_norm=0.5)
    assert all(np.array_equal(a, b) for a, b in zip(p + m + v, p2 + m2 + v2))
    assert st2["step"] == 2 and st2["skipped"] == 1 and st2["beta1_pow"] == st["beta1_pow"]
    assert np.isnan(st2["grad_norm"]) and float(st2["clip_scale"]) == 1.0
    g[9][0] = 0.0
    g[0][-1, -1] = np.inf
    st3 = policy.reference_adam_step(p2, g, m2, v2, st2, max_grad_norm=0.5)[3]
    assert st3["skipped"] == 2 and np.isinf(st3["grad_norm"]) and float(st3["clip_scale"]) == 0.0


def test_beta_powers_are_running_products():
    st = ac.reference_five("odd")[4][3]
    assert st["step"] == 5
    assert (st["beta1_pow"], st["beta2_pow"]) == policy.adam_beta_powers(5, (0.9, 0.999))
    assert policy.adam_beta_powers(0, (0.9, 0.999)) == (0.0, 0.0)
    assert policy.adam_beta_powers(3, (0.9, 0.999)) == (0.9 * 0.9 * 0.9, 0.999 * 0.999 * 0.999)


# ------------------------------------------------------------------ arguments
@pytest.mark.parametrize("bad", (dict(lr=-1e-3), dict(lr=float("nan")), dict(betas=(1.0, 0.999)),
                                 dict(betas=(0.9, -0.1)), dict(betas=(0.9,)), dict(eps=0.0), dict(eps=-1e-8),
                                 dict(weight_decay=-0.1), dict(max_grad_norm=float("nan"))), ids=str)
def test_argument_checks(bad):
    kw = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, max_grad_norm=0.0)
    policy.check_adam_args(**kw)
    kw.update(bad)
    with pytest.raises(ValueError):
        policy.check_adam_args(**kw)
    z = ac.zeros("tiny")
    with pytest.raises(ValueError):
        policy.reference_adam_step(list(ac.params("tiny")), ac.grads("tiny"), z, z, policy.adam_fresh_state(), **kw)


def test_lr_zero_is_allowed_and_moves_only_the_moments():
    p, m, v, st = ac.reference_run("odd", 1, lr=0.0)[0]
    assert all(np.array_equal(a, b) for a, b in zip(p, ac.params("odd")))
    assert all(bool((a != 0).any()) for a in m + v) and st["step"] == 1


# ------------------------------------------------------------------ the state_dict layout
def order_of(model):
    named = [n for n, _ in model.named_parameters()]
    return [named.index(n) for n in ac.NAMES]


def stepped(model, opt, steps, first=0):
    by_name = dict(model.named_parameters())
    for k in range(first, first + steps):
        for n, g in zip(ac.NAMES, ac.grads("odd", k)):
            by_name[n].grad = torch.tensor(g)
        opt.step()


def test_state_dict_moves_between_torch_adam_and_the_device_layout():
    registered = ("value_head", "affine1", "affine3", "affine2", "action_head")  # not ADAM_TENSORS' order
    model = ac.make_model("odd", registered)
    order, shapes = order_of(model), ac.shapes(ac.NETS["odd"])
    assert order != list(range(10))
    opt = torch.optim.Adam(model.parameters(), lr=2e-3, betas=(0.8, 0.99), weight_decay=0.01)
    # a fresh optimizer: an empty state
    step, m, v, hyper = policy.parse_adam_state_dict(opt.state_dict(), order, shapes)
    assert (step, m, v) == (0, None, None) and hyper["lr"] == 2e-3 and not hyper["decoupled"]
    stepped(model, opt, 3)
    sd = opt.state_dict()
    step, m, v, hyper = policy.parse_adam_state_dict(sd, order, shapes)
    assert step == 3 and hyper == {"lr": 2e-3, "betas": (0.8, 0.99), "eps": 1e-8, "weight_decay": 0.01,
                                   "decoupled": False}
    by_name = dict(model.named_parameters())
    for k, n in enumerate(ac.NAMES):  # tensor k of the flat order is the moment of that parameter
        assert torch.equal(m[k], opt.state[by_name[n]]["exp_avg"]) and tuple(m[k].shape) == tuple(shapes[k])
        assert torch.equal(v[k], opt.state[by_name[n]]["exp_avg_sq"])
    # and back: torch's Adam loads what adam_state_dict writes and continues with the same bits
    back = policy.adam_state_dict(step, m, v, order, hyper["lr"], hyper["betas"], hyper["eps"], hyper["weight_decay"],
                                  hyper["decoupled"], 0.5)
    assert set(back["param_groups"][0]) == set(sd["param_groups"][0]) | {"max_grad_norm"}
    assert policy.parse_adam_state_dict(back, order, shapes)[3]["max_grad_norm"] == 0.5
    twin = ac.make_model("odd", registered)
    twin.load_state_dict(model.state_dict())
    opt2 = torch.optim.Adam(twin.parameters())
    opt2.load_state_dict(back)
    stepped(model, opt, 2, first=3)
    stepped(twin, opt2, 2, first=3)
    assert all(torch.equal(a, b) for a, b in zip(model.parameters(), twin.parameters()))
    assert policy.parse_adam_state_dict(torch.optim.AdamW(ac.make_model("odd").parameters()).state_dict(), order,
                                        shapes)[3]["decoupled"]
    # layouts DeviceAdam cannot take
    for spoil in ("amsgrad", "groups", "steps", "partial", "shape"):
        bad = {"state": {i: dict(s) for i, s in sd["state"].items()}, "param_groups": [dict(sd["param_groups"][0])]}
        if spoil == "amsgrad":
            bad["param_groups"][0]["amsgrad"] = True
        elif spoil == "groups":
            bad["param_groups"] = bad["param_groups"] * 2
        elif spoil == "steps":
            bad["state"][4]["step"] = torch.tensor(7.0)
        elif spoil == "partial":
            del bad["state"][2]
        else:
            bad["state"][order[0]]["exp_avg"] = torch.zeros(3, 3)
        with pytest.raises(ValueError):
            policy.parse_adam_state_dict(bad, order, shapes)
