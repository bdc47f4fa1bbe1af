"""wab_policy_adam_step on the GPU (DeviceAdam, and the C-ABI through ctypes for the net no handle
can run) against its contract, wab_gym_amd.policy.reference_adam_step: everything is compared bit
for bit.  The nets of tests/adam_cases.py: the reference's, one with nothing a multiple of a tile,
one wider than 128, the minimum of everything, and one with more than 1024 first-level partials
of the norm (the two-level tree)."""
import ctypes
import functools
import importlib.util
import os

import numpy as np
import pytest
import torch

import adam_cases as ac
import policy_cases as pc
import policy_grad_cases as pgc
from wab_gym_amd import _lib, policy
from wab_gym_amd.env import BatchedWolvesAndBushesEnv
from wab_gym_amd.wrappers import PragmaticObsWrapper

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B_ACT = 128


@functools.lru_cache(maxsize=None)
def env_for(n_actions, B=B_ACT):
    env = BatchedWolvesAndBushesEnv(dict(pc.OPTS_REF if n_actions == 5 else pc.OPTS_ODD), num_envs=B, seed=pc.SEED,
                                    device=DEV)
    env.reset()
    return env


def bits(x):
    x = np.ascontiguousarray(x)
    return x.view({4: np.uint32, 8: np.uint64}[x.dtype.itemsize])


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def state_matches(got, want, non_finite=False):
    """got: a _lib.WabAdamState read back; want: the reference's state dict."""
    ok = (int(got.step) == want["step"] and int(got.skipped) == want["skipped"]
          and same_bits(np.float32(got.clip_scale), np.float32(want["clip_scale"])))
    if want["step"] > 0:
        ok = ok and same_bits(np.float64(got.beta1_pow), np.float64(want["beta1_pow"])) \
            and same_bits(np.float64(got.beta2_pow), np.float64(want["beta2_pow"]))
    if non_finite:  # (a NaN's payload is not part of the contract)
        w = np.float32(want["grad_norm"])
        return ok and (np.isnan(got.grad_norm) if np.isnan(w) else got.grad_norm == w)
    return ok and same_bits(np.float32(got.grad_norm), np.float32(want["grad_norm"]))


class Raw:
    """wab_policy_adam_step through ctypes on device tensors: a policy handle needs no env."""

    def __init__(self, which):
        self.L = _lib.load()
        shp = _lib.WabPolicyShape(*ac.NETS[which])
        self.pol = ctypes.c_void_p()
        _lib.check(self.L.wab_policy_create(ctypes.addressof(shp), 0, ctypes.byref(self.pol)), "wab_policy_create")
        self.p = [torch.from_numpy(x.copy()).to(DEV) for x in ac.params(which)]
        self.m = [torch.zeros_like(x) for x in self.p]
        self.v = [torch.zeros_like(x) for x in self.p]
        self.state = torch.zeros(6, dtype=torch.int64, device=DEV)
        self.ws_bytes = int(self.L.wab_policy_adam_workspace(self.pol))
        assert self.ws_bytes > 0 and self.ws_bytes % 8 == 0
        self.ws = torch.empty(self.ws_bytes // 8, dtype=torch.float64, device=DEV)

    @staticmethod
    def weights(xs):
        return _lib.WabPolicyWeights(*[x.data_ptr() for x in xs])

    def stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)

    def load(self):
        w = self.weights(self.p)
        _lib.check(self.L.wab_policy_load(self.pol, ctypes.addressof(w), self.stream()), "wab_policy_load")

    def call(self, grads, ws_bytes=None, state=None, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0,
             decoupled=False, max_grad_norm=0.0):
        self.g = [torch.from_numpy(np.ascontiguousarray(x)).to(DEV) for x in grads]
        sets = [self.weights(x) for x in (self.p, self.g, self.m, self.v)]
        cfg = _lib.WabAdamConfig(lr, betas[0], betas[1], eps, weight_decay, max_grad_norm, 1 if decoupled else 0)
        return self.L.wab_policy_adam_step(self.pol, *[ctypes.addressof(s) for s in sets], ctypes.addressof(cfg),
                                           self.state.data_ptr() if state is None else state, self.ws.data_ptr(),
                                           self.ws_bytes if ws_bytes is None else ws_bytes, self.stream())

    def read(self):
        st = _lib.WabAdamState.from_buffer_copy(self.state.cpu().numpy().tobytes())
        return tuple([x.cpu().numpy() for x in xs] for xs in (self.p, self.m, self.v)) + (st,)

    def close(self):
        torch.cuda.synchronize()
        self.L.wab_policy_destroy(self.pol)


def assert_matches(got, want, what, non_finite=False):
    """(params, exp_avg, exp_avg_sq, state) read from the device against the reference's."""
    for kind, g, w in zip(("param", "exp_avg", "exp_avg_sq"), got[:3], want[:3]):
        for name, a, b in zip(ac.NAMES, g, w):
            assert same_bits(a, b), (what, kind, name, int((bits(a) != bits(b)).sum()), a.size)
    st = got[3]
    assert state_matches(st, want[3], non_finite), (what, {f: getattr(st, f) for f, _ in st._fields_}, want[3])


class Dev:
    """A model holding ac.params(which) on the device, its DevicePolicy and a DeviceAdam."""

    def __init__(self, which, B=B_ACT, **hyper):
        self.which = which
        self.model = ac.make_model(which).to(DEV)
        self.pol = policy.DevicePolicy(self.model, env_for(ac.NETS[which][4], B))
        self.opt = policy.DeviceAdam(self.pol, self.model, **hyper)
        self.by_name = dict(self.model.named_parameters())

    def step(self, grads):
        for name, g in zip(ac.NAMES, grads):
            self.by_name[name].grad = torch.from_numpy(np.ascontiguousarray(g)).to(DEV)
        self.opt.step()

    def read(self):
        return ([self.by_name[n].detach().cpu().numpy() for n in ac.NAMES], [x.cpu().numpy() for x in self.opt.exp_avg],
                [x.cpu().numpy() for x in self.opt.exp_avg_sq], self.opt._read_state())

    def act(self, pol=None):
        """(probs, value) of the shared feature rows under the policy's image as it is."""
        pol = self.pol if pol is None else pol
        F, A = ac.NETS[self.which][0], ac.NETS[self.which][4]
        x = torch.from_numpy(pc.odd_features(B_ACT, F)).to(DEV)
        probs = torch.empty(B_ACT, A, device=DEV)
        value = torch.empty(B_ACT, device=DEV)
        pol.act(x, probs=probs, value=value)
        return probs.cpu().numpy(), value.cpu().numpy()

    def image_is_the_parameters(self):
        """the image the step wrote acts like a fresh policy loaded from the updated parameters"""
        fresh = policy.DevicePolicy(self.model, self.pol.env)
        got, want = self.act(), self.act(fresh)
        fresh.close()
        return same_bits(got[0], want[0]) and same_bits(got[1], want[1])

    def close(self):
        self.pol.close()


# ------------------------------------------------------------------ one step and five, every net
@pytest.mark.parametrize("which", ("ref", "odd", "wide", "two_level"))
def test_five_steps_match_the_reference_and_the_image_follows(which):
    d = Dev(which)
    before = d.act()
    want = ac.reference_five(which)
    for k in range(5):
        d.step(ac.grads(which, k))
        if k in (0, 4):
            assert_matches(d.read(), want[k], "%s step %d" % (which, k + 1))
            assert d.image_is_the_parameters(), (which, k)
    after = d.act()
    assert not same_bits(before[0], after[0])  # (the steps changed what the policy does)
    assert d.opt.stats() == {"step": 5, "skipped": 0, "grad_norm": float(want[4][3]["grad_norm"]), "clip_scale": 1.0}
    d.close()


def test_the_smallest_net_through_the_c_abi():
    r = Raw("tiny")
    # refusals first, each before anything is launched: the state stays all zero
    g = ac.grads("tiny", 0)
    assert r.call(g) == -4  # WAB_E_STATE: nothing loaded yet
    r.load()
    for bad in (dict(lr=-1.0), dict(betas=(1.0, 0.999)), dict(betas=(0.9, -0.5)), dict(eps=0.0),
                dict(weight_decay=-1.0), dict(lr=float("nan")), dict(ws_bytes=r.ws_bytes - 1),
                dict(state=r.state.data_ptr() + 4)):
        assert r.call(g, **bad) == -1, bad
    assert int(r.read()[3].step) == 0 and bytes(r.read()[3]) == bytes(48)
    want = ac.reference_five("tiny")
    for k in range(5):
        assert r.call(ac.grads("tiny", k)) == 0
        if k in (0, 4):
            assert_matches(r.read(), want[k], "tiny step %d" % (k + 1))
    r.close()


def test_two_level_tree_is_two_levels():
    n = ac.count(ac.NET_TWO_LEVEL)
    first = (n + 1023) // 1024
    assert first > 1024
    r = Raw("two_level")
    assert r.ws_bytes == 8 * (first + (first + 1023) // 1024)
    r.close()
    r = Raw("ref")
    assert r.ws_bytes == 8 * ((ac.count(pc.NET_REF) + 1023) // 1024)
    r.close()


# ------------------------------------------------------------------ clip, decay, lr = 0
@pytest.mark.parametrize("which", ("ref", "odd"))
def test_clip_active_and_inactive(which):
    d = Dev(which, max_grad_norm=0.5)
    want = ac.reference_run(which, 2, grad_scale=1e3, max_grad_norm=0.5)
    assert all(0.0 < float(w[3]["clip_scale"]) < 1e-2 for w in want)
    for k in range(2):
        d.step(ac.grads(which, k, 1e3))
        assert_matches(d.read(), want[k], "%s clipped step %d" % (which, k + 1))
    assert d.image_is_the_parameters()
    d.close()
    d = Dev(which, max_grad_norm=1e9)
    d.step(ac.grads(which, 0))
    got = d.read()
    assert_matches(got, ac.reference_run(which, 1, max_grad_norm=1e9)[0], "%s loose clip" % which)
    assert got[3].clip_scale == 1.0
    assert all(same_bits(a, b) for a, b in zip(got[0], ac.reference_five(which)[0][0]))  # c == 1 changes no bit
    d.close()


@pytest.mark.parametrize("which", ("ref", "odd"))
@pytest.mark.parametrize("decoupled", (False, True), ids=("l2", "adamw"))
def test_weight_decay(which, decoupled):
    hyper = dict(lr=1e-2, weight_decay=0.05, decoupled=decoupled)
    d = Dev(which, **hyper)
    want = ac.reference_run(which, 3, **hyper)
    for k in range(3):
        d.step(ac.grads(which, k))
    assert_matches(d.read(), want[2], "%s decay, decoupled=%s" % (which, decoupled))
    assert not all(same_bits(a, b) for a, b in zip(want[2][0], ac.reference_run(which, 3, lr=1e-2)[2][0]))
    assert d.image_is_the_parameters()
    d.close()


def test_lr_zero_moves_the_moments_only():
    d = Dev("odd", lr=0.0)
    d.step(ac.grads("odd", 0))
    got = d.read()
    assert_matches(got, ac.reference_run("odd", 1, lr=0.0)[0], "lr = 0")
    assert all(same_bits(a, b) for a, b in zip(got[0], ac.params("odd")))
    assert all(bool((a != 0).any()) for a in got[1] + got[2])
    # lr is settable between calls
    d.opt.lr = 1e-3
    d.step(ac.grads("odd", 1))
    assert_matches(d.read(), ac.reference_run("odd", 1, start=ac.reference_run("odd", 1, lr=0.0)[0], lr=1e-3)[0],
                   "lr set between calls")
    d.close()


# ------------------------------------------------------------------ a non-finite gradient
def test_non_finite_gradient_changes_nothing_but_the_count():
    d = Dev("ref", max_grad_norm=0.5)
    ref = ac.reference_run("ref", 2, max_grad_norm=0.5)
    for k in range(2):
        d.step(ac.grads("ref", k))
    kept, acted = d.read(), d.act()
    assert_matches(kept, ref[1], "before the bad gradients")
    cur = ref[1]
    for n_skipped, (name, index, value) in enumerate((("value_head.bias", (0,), np.nan),
                                                      ("affine1.weight", (-1, -1), np.inf)), 1):
        g = [x.copy() for x in ac.grads("ref", 2)]
        g[ac.NAMES.index(name)][index] = value
        d.step(g)
        cur = policy.reference_adam_step(cur[0], g, cur[1], cur[2], cur[3], max_grad_norm=0.5)
        got = d.read()
        assert_matches(got, cur, "skip %d" % n_skipped, non_finite=True)
        assert all(same_bits(a, b) for x, y in zip(got[:3], kept[:3]) for a, b in zip(x, y))
        assert int(got[3].skipped) == n_skipped and int(got[3].step) == 2
        after = d.act()
        assert same_bits(after[0], acted[0]) and same_bits(after[1], acted[1])
    assert d.opt.stats()["skipped"] == 2 and d.opt.stats()["grad_norm"] == float("inf")
    # a clean step afterwards continues from the unchanged state
    g = ac.grads("ref", 2)
    d.step(g)
    cur = policy.reference_adam_step(cur[0], g, cur[1], cur[2], cur[3], max_grad_norm=0.5)
    assert cur[3]["step"] == 3 and cur[3]["skipped"] == 2
    assert_matches(d.read(), cur, "the clean step after")
    assert d.image_is_the_parameters()
    d.close()


# ------------------------------------------------------------------ reproducible, checkpoints
def test_two_runs_give_equal_bits():
    runs = []
    for _ in range(2):
        r = Raw("ref")
        r.load()
        for k in range(3):
            assert r.call(ac.grads("ref", k), max_grad_norm=0.5) == 0
        runs.append(r.read())
        r.close()
    assert all(same_bits(a, b) for x, y in zip(runs[0][:3], runs[1][:3]) for a, b in zip(x, y))
    assert bytes(runs[0][3]) == bytes(runs[1][3])


def test_state_dict_round_trips_and_moves_to_torch():
    hyper = dict(lr=2e-3, betas=(0.8, 0.99), weight_decay=0.01, max_grad_norm=0.5)
    a = Dev("odd", **hyper)
    for k in range(3):
        a.step(ac.grads("odd", k))
    sd = a.opt.state_dict()
    assert sorted(sd["state"]) == list(range(10)) and float(sd["state"][0]["step"]) == 3.0
    b = Dev("odd")
    b.model.load_state_dict(a.model.state_dict())
    b.pol.load(b.model)
    b.opt.load_state_dict(sd)
    assert (b.opt.lr, b.opt.betas, b.opt.weight_decay, b.opt.max_grad_norm) == (2e-3, (0.8, 0.99), 0.01, 0.5)
    for x in (a, b):
        x.step(ac.grads("odd", 3))
    got_a, got_b = a.read(), b.read()
    assert all(same_bits(p, q) for x, y in zip(got_a[:3], got_b[:3]) for p, q in zip(x, y))
    assert (got_b[3].step, got_b[3].beta1_pow, got_b[3].beta2_pow) == (4, got_a[3].beta1_pow, got_a[3].beta2_pow)
    # torch's Adam takes the same checkpoint (its own rounding order from there on)
    topt = torch.optim.Adam(b.model.parameters())
    topt.load_state_dict(a.opt.state_dict())
    assert topt.param_groups[0]["lr"] == 2e-3 and float(topt.state[b.by_name["affine1.weight"]]["step"]) == 4.0
    # what step() asks of the gradients
    b.by_name["affine2.bias"].grad = None
    with pytest.raises(RuntimeError, match="affine2.bias"):
        b.opt.step()
    with pytest.raises(ValueError):
        policy.DeviceAdam(b.pol, ac.make_model("odd"))  # parameters on the CPU
    with pytest.raises(ValueError):
        policy.DeviceAdam(b.pol, b.model, betas=(0.9, 1.0))
    a.close()
    b.close()


# ------------------------------------------------------------------ a captured update, the example
def example():
    spec = importlib.util.spec_from_file_location("train_actor_critic", os.path.join(REPO, "examples",
                                                                                   "train_actor_critic.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_captured_update_replays_to_the_eager_bits():
    n = 258
    args = [torch.as_tensor(np.ascontiguousarray(x)).to(DEV) for x in (pgc.features("ref", n),) + pgc.rows("ref", n)]
    env = env_for(5)

    def fresh():
        torch.manual_seed(11)
        model = example().Policy(449, 5).to(DEV)
        pol = policy.DevicePolicy(model, env)
        return model, pol, policy.DeviceAdam(pol, model, lr=1e-2, max_grad_norm=0.5)

    def update(pol, model, opt):
        out = pol.loss_and_grad(*args, into=model, reduction="mean", entropy_coef=0.01)
        opt.step()
        return out

    model, pol, opt = fresh()
    losses = [update(pol, model, opt)["loss"].clone() for _ in range(3)]
    want = [p.detach().clone() for p in model.parameters()] + [x.clone() for x in opt.exp_avg + opt.exp_avg_sq]
    want_state = bytes(opt._read_state())
    assert not torch.equal(losses[0], losses[2])  # (each update sees the parameters of the one before)
    pol.close()

    model, pol, opt = fresh()
    pol.loss_and_grad(*args, into=model, reduction="mean", entropy_coef=0.01)  # (workspace and .grad exist)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        cap = update(pol, model, opt)
    assert opt.stats()["step"] == 0  # (a capture runs nothing)
    for k in range(3):
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(cap["loss"], losses[k]), k
    got = [p.detach() for p in model.parameters()] + opt.exp_avg + opt.exp_avg_sq
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    assert bytes(opt._read_state()) == want_state
    pol.close()


def test_train_loop_runs():
    mod = example()
    env = BatchedWolvesAndBushesEnv(dict(pc.OPTS_REF), num_envs=128, seed=pc.SEED, device=DEV)
    wrapper = PragmaticObsWrapper(env)
    wrapper.reset()
    torch.manual_seed(3)
    model = mod.Policy(449, 5).to(DEV)
    pol = policy.DevicePolicy(model, env)
    opt = policy.DeviceAdam(pol, model, lr=3e-4, max_grad_norm=0.5)
    before = [p.detach().clone() for p in model.parameters()]
    losses = [float(mod.update_device(wrapper, pol, model, opt, 8, entropy_coef=0.01)["loss"]) for _ in range(3)]
    pol.check()
    assert all(np.isfinite(x) for x in losses), losses
    stats = opt.stats()
    assert stats["step"] == 3 and stats["skipped"] == 0 and stats["grad_norm"] > 0 and 0 < stats["clip_scale"] <= 1
    assert all(not torch.equal(p.detach(), q) for p, q in zip(model.parameters(), before))
    pol.close()
