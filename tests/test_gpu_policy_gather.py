"""Rows gathered by an index on the GPU (DevicePolicy.loss_and_grad, ppo_loss_and_grad and evaluate
with rows=; wab_policy_grad_gather, wab_policy_grad_ppo_gather, wab_policy_evaluate_gather).

The specification is an identity: a call with rows= is, bit for bit, the contiguous call on
index_select copies of the features and of every per-row array: the ten gradients, the four loss
scalars, the four PPO sums and every row output.  The contiguous call is held to the contract by
tests/test_gpu_policy_grad.py and tests/test_gpu_ppo.py, so nothing here has a tolerance:
torch.equal everywhere.  An index outside the source is never followed: the result is the
contiguous call on copies gathered through the clamped index with action -1 at those rows."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import policy_grad_cases as pgc
import ppo_cases as ppc
import test_gpu_ppo as tp
from wab_gym_amd import _lib, policy

pytestmark = pytest.mark.gpu
DEV = tp.DEV
NETS = ("ref", "odd", "wide", (1, 1, 1, 1, 5))
M = 300
ROWS = (0, 1, 128, 129, 257)
KEYS = ("x", "a", "adv", "t", "old_logp", "old_value")
SCALARS = ("loss", "loss_policy", "loss_value", "entropy")
PPO_CONFIGS = [dict(value_clip=vc, entropy_coef=ec, reduction=red)
               for vc in (ppc.VALUE_CLIP, None) for ec in (0.0, 0.01) for red in ("sum", "mean")]


@functools.lru_cache(maxsize=None)
def source(net, m=M):
    """The source's M rows on the device, made once: ppo_cases' case of the net."""
    c = ppc.case(net, m)
    return {k: tp.dev(c[k], torch.int8 if k == "a" else torch.float32) for k in KEYS}


def index_kinds(n, m=M):
    """{name: int32 [n] source rows}."""
    rng = np.random.RandomState(1000 + n)
    perm = rng.permutation(m)
    kinds = {}
    if n <= m:
        kinds["identity"] = np.arange(n)
        kinds["reversed"] = np.arange(n)[::-1]
    kinds["permutation"] = perm[:n] if n <= m else np.concatenate([perm, rng.permutation(m)])[:n]
    kinds["duplicates"] = rng.randint(m, size=n)
    kinds["one_row"] = np.full(n, 123)
    ends = kinds["permutation"].copy()  # rows 0 and M - 1 at the first and last place of each block
    for place, row in ((0, 0), (127, m - 1), (128, m - 1), (255, 0), (256, 0), (n - 1, m - 1)):
        if 0 <= place < n:
            ends[place] = row
    kinds["ends"] = ends
    return {k: np.ascontiguousarray(v, dtype=np.int32) for k, v in kinds.items()}


def gathered(src, r):
    """index_select copies of the source through the int64 index r."""
    return {k: v.index_select(0, r).contiguous() for k, v in src.items()}


def a2c(pol, s, **kw):
    return pol.loss_and_grad(s["x"], s["a"], s["adv"], s["t"], return_rows=True, value_coef=0.5, **kw)


def ppo(pol, s, value_clip=ppc.VALUE_CLIP, **kw):
    return pol.ppo_loss_and_grad(s["x"], s["a"], s["adv"], s["t"], s["old_logp"], clip=ppc.CLIP,
                                 old_value=s["old_value"], value_clip=value_clip, return_rows=True, value_coef=0.5, **kw)


def assert_equal(got, want, what):
    assert sorted(got) == sorted(want), what
    for k, w in want.items():
        if k == "grads":
            assert sorted(got[k]) == sorted(pgc.GRAD_NAMES)
            for name in pgc.GRAD_NAMES:
                assert torch.equal(got[k][name], w[name]), (what, name)
        else:
            assert got[k].shape == w.shape and torch.equal(got[k], w), (what, k)


# ------------------------------------------------------------------ the identity, M = 300
@pytest.mark.parametrize("net", NETS, ids=str)
@pytest.mark.parametrize("n", ROWS)
def test_gathered_call_is_the_contiguous_call_on_copies(net, n):
    src = source(net)
    pol = tp.policy_for(net)
    for kind, rows in index_kinds(n).items():
        r32 = tp.dev(rows, torch.int32)
        cp = gathered(src, r32.long())
        for chunk_rows in (0, 128):
            what = "%s N=%d %s chunk_rows=%d" % (net, n, kind, chunk_rows)
            for ec, red in ((0.0, "sum"), (0.01, "mean")):
                kw = dict(entropy_coef=ec, reduction=red, chunk_rows=chunk_rows)
                assert_equal(a2c(pol, src, rows=r32, **kw), a2c(pol, cp, **kw), what + " loss_and_grad")
            for cfg in PPO_CONFIGS:
                got, want = ppo(pol, src, rows=r32, chunk_rows=chunk_rows, **cfg), ppo(pol, cp, chunk_rows=chunk_rows, **cfg)
                assert_equal(got, want, what + " ppo %s" % (cfg,))
                assert got["logp"].shape == (n,) and got["ratio"].shape == (n,)
        got, want = pol.evaluate(src["x"], src["a"], rows=r32), pol.evaluate(cp["x"], cp["a"])
        assert_equal(got, want, "%s N=%d %s evaluate" % (net, n, kind))
        assert_equal(pol.evaluate(src["x"], rows=r32), pol.evaluate(cp["x"]), "%s N=%d %s evaluate, no actions" % (net, n, kind))
        pol.check()
    # the rows took part: the gradients are not all zero, and a permutation is not the identity's result
    if n >= 128 and net != (1, 1, 1, 1, 5):
        k = index_kinds(n)
        g1 = ppo(pol, src, rows=tp.dev(k["permutation"], torch.int32))["grads"]["affine1.weight"]
        g2 = ppo(pol, src, rows=tp.dev(k["identity"], torch.int32))["grads"]["affine1.weight"]
        assert bool((g1 != 0).any()) and not torch.equal(g1, g2)
    pol.close()


def test_int64_index_a_slice_and_a_segment_shaped_source():
    net, n = "odd", 129
    src = source(net)
    pol = tp.policy_for(net)
    perm = tp.dev(np.random.RandomState(5).permutation(M), torch.int32)
    want = ppo(pol, gathered(src, perm[100:100 + n].long()))
    assert_equal(ppo(pol, src, rows=perm[100:100 + n]), want, "a slice of a permutation")
    assert_equal(ppo(pol, src, rows=perm.long()[100:100 + n]), want, "an int64 index")
    T = 3
    seg = {k: v.view(T, M // T, *v.shape[1:]) for k, v in src.items()}
    got = ppo(pol, seg, rows=perm[100:100 + n])
    assert_equal(got, want, "a [T, B, F] source")
    for bad in (perm.float(), perm.view(2, -1), perm[::2], perm.cpu()):
        with pytest.raises(ValueError):
            ppo(pol, src, rows=bad)
    # N may exceed M
    twice = torch.cat([perm, perm.flip(0)])
    assert_equal(ppo(pol, src, rows=twice), ppo(pol, gathered(src, twice.long())), "N = 2 M")
    pol.check()
    pol.close()


def test_accumulate_over_two_gathered_halves():
    src = source("ref")
    _, model = tp.model_of()
    pol = policy.DevicePolicy(model, tp.env_for(5, 128))
    _, model2 = tp.model_of()
    perm = tp.dev(np.random.RandomState(6).permutation(M), torch.int32)
    halves = (perm[:M // 2], perm[M // 2:])
    outs, outs2 = [], []
    for i, h in enumerate(halves):
        outs.append(ppo(pol, src, rows=h, into=model, accumulate=i > 0, entropy_coef=0.01))
        outs2.append(ppo(pol, gathered(src, h.long()), into=model2, accumulate=i > 0, entropy_coef=0.01))
    for (k, p), (k2, p2) in zip(model.named_parameters(), model2.named_parameters()):
        assert k == k2 and torch.equal(p.grad, p2.grad) and bool((p.grad != 0).any()), k
    for o, o2 in zip(outs, outs2):
        assert_equal(o, o2, "accumulate")
    pol.check()
    pol.close()


# ------------------------------------------------------------------ more than one block per slab
@functools.lru_cache(maxsize=None)
def big_source(net, m=20000):
    """pgc's rows of the net; old_logp and old_value are the device's own logp and value shifted by
    fixed patterns, so that rows of every kind take part."""
    a, w, t = pgc.rows(net, m)
    s = {"x": tp.dev(pgc.features(net, m), torch.float32), "a": tp.dev(a, torch.int8), "adv": tp.dev(w, torch.float32),
         "t": tp.dev(t, torch.float32)}
    pol = tp.policy_for(net)
    ev = pol.evaluate(s["x"], s["a"])
    pol.check()
    i = torch.arange(m, device=DEV)
    s["old_logp"] = (ev["logp"] + ((i % 5) - 2).float() * 0.125).contiguous()
    s["old_value"] = (ev["value"] + ((i % 4).float() - 1.5) * 0.2).contiguous()
    pol.close()
    return s


@pytest.mark.parametrize("net", ("ref", "odd"))
def test_gathered_call_with_several_blocks_in_every_slab(net):
    m, n = 20000, 16513
    src = big_source(net)
    pol = tp.policy_for(net)
    assert (n + 127) // 128 >= 2 * pgc.SLABS[net]
    r32 = tp.dev(np.random.RandomState(11).permutation(m)[:n], torch.int32)
    cp = gathered(src, r32.long())
    for chunk_rows in (0, 384):
        what = "%s N=%d chunk_rows=%d" % (net, n, chunk_rows)
        kw = dict(entropy_coef=0.01, reduction="mean", chunk_rows=chunk_rows)
        assert_equal(a2c(pol, src, rows=r32, **kw), a2c(pol, cp, **kw), what + " loss_and_grad")
        assert_equal(ppo(pol, src, rows=r32, **kw), ppo(pol, cp, **kw), what + " ppo")
    assert_equal(pol.evaluate(src["x"], src["a"], rows=r32), pol.evaluate(cp["x"], cp["a"]), "%s evaluate" % net)
    pol.check()
    # the state left behind: a small gathered call afterwards is a fresh policy's
    small = tp.dev(np.random.RandomState(12).permutation(m)[:130], torch.int32)
    used = ppo(pol, src, rows=small, entropy_coef=0.01)
    fresh = tp.policy_for(net)
    assert_equal(used, ppo(fresh, src, rows=small, entropy_coef=0.01), "%s: 130 rows after the big call" % net)
    assert_equal(used, ppo(fresh, gathered(src, small.long()), entropy_coef=0.01), "%s: 130 rows, copies" % net)
    fresh.close()
    pol.check()
    pol.close()


# ------------------------------------------------------------------ indices outside the source
def counts(pol):
    L = _lib.load()
    out = []
    for call in (L.wab_policy_grad_bad_actions, L.wab_policy_grad_bad_rows):
        v = ctypes.c_uint64(0)
        call(pol._p, pol._grad_ws.data_ptr(), pol.env._stream(), ctypes.byref(v))
        out.append(int(v.value))
    return tuple(out)


@pytest.mark.parametrize("net", ("ref", "wide"))
def test_bad_indices_are_clamped_left_out_and_counted(net):
    n = 300
    src = source(net)
    pol = tp.policy_for(net)
    rows = np.random.RandomState(13).permutation(M).astype(np.int64)
    places = (5, 127, 128, 299)  # blocks 0, 0 (its last row), 1 and 2
    values = (-1, M, 2 ** 31 - 1, -2 ** 31)
    assert len({p // 128 for p in places}) == 3
    bad = rows.copy()
    bad[list(places)] = values
    r32 = tp.dev(bad.astype(np.int32), torch.int32)
    clamped = tp.dev(np.clip(bad, 0, M - 1), torch.int64)
    cp = gathered(src, clamped)
    cp["a"][list(places)] = -1
    for chunk_rows in (0, 128):
        kw = dict(entropy_coef=0.01, chunk_rows=chunk_rows)
        got = ppo(pol, src, rows=r32, **kw)
        assert counts(pol) == (0, 4)
        with pytest.raises(IndexError, match=r"4 rows had an index outside"):
            pol.check()
        want = ppo(pol, cp, **kw)
        assert counts(pol) == (4, 0)  # (the copies' four rows are bad-action rows)
        assert_equal(got, want, "%s bad indices, ppo, chunk_rows=%d" % (net, chunk_rows))
        for p in places:
            assert float(got["logp"][p]) == 0.0 and float(got["ratio"][p]) == 0.0
        got = a2c(pol, src, rows=r32, **kw)
        assert counts(pol) == (0, 4)
        assert_equal(got, a2c(pol, cp, **kw), "%s bad indices, loss_and_grad, chunk_rows=%d" % (net, chunk_rows))
    got = pol.evaluate(src["x"], src["a"], rows=r32)
    assert counts(pol) == (0, 4)
    assert_equal(got, pol.evaluate(cp["x"], cp["a"]), "%s bad indices, evaluate" % net)
    # value and entropy are the clamped source row's
    clean = pol.evaluate(src["x"], src["a"], rows=tp.dev(np.clip(bad, 0, M - 1).astype(np.int32), torch.int32))
    assert counts(pol) == (0, 0)
    pol.check()
    assert torch.equal(got["value"], clean["value"]) and torch.equal(got["entropy"], clean["entropy"])
    # a bad action at a good index is still a bad action, and the next clean call reports nothing
    a_bad = src["a"].clone()
    a_bad[int(rows[7])] = 9
    s2 = dict(src, a=a_bad)
    ppo(pol, s2, rows=r32)
    assert counts(pol) == (1, 4)
    ppo(pol, src, rows=tp.dev(rows.astype(np.int32), torch.int32))
    assert counts(pol) == (0, 0)
    pol.check()
    pol.close()


# ------------------------------------------------------------------ a captured graph, the example
def test_a_captured_graph_reads_the_index_at_replay():
    net, n = "ref", 129
    src = source(net)
    pol = tp.policy_for(net)
    rng = np.random.RandomState(14)
    perms = [tp.dev(rng.permutation(M), torch.int32) for _ in range(3)]
    buf = perms[0].clone()
    kw = dict(entropy_coef=0.01, reduction="mean")
    ppo(pol, src, rows=buf[20:20 + n], **kw)  # (the workspace exists before the capture)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        cap = ppo(pol, src, rows=buf[20:20 + n], **kw)
    for p in perms[1:]:
        buf.copy_(p)
        g.replay()
        torch.cuda.synchronize()
        got = {k: (v.clone() if k != "grads" else {q: x.clone() for q, x in v.items()}) for k, v in cap.items()}
        assert_equal(got, ppo(pol, gathered(src, p[20:20 + n].long()), **kw), "replay after a new permutation")
    pol.check()
    pol.close()


def test_a_short_shuffled_ppo_run():
    from wab_gym_amd.env import BatchedWolvesAndBushesEnv
    from wab_gym_amd.wrappers import PragmaticObsWrapper
    import policy_cases as pc

    B, T = 256, 16
    mod, model = tp.model_of(seed=3)
    env = BatchedWolvesAndBushesEnv(dict(pc.OPTS_REF), num_envs=B, seed=pc.SEED, device=DEV)
    wrapper = PragmaticObsWrapper(env)
    wrapper.reset()
    pol = policy.DevicePolicy(model, env)
    opt = policy.DeviceAdam(pol, model, lr=3e-4, max_grad_norm=0.5)
    before = [p.detach().clone() for p in model.parameters()]
    perm = torch.zeros(T * B, dtype=torch.int32, device=DEV)
    results = mod.update(wrapper, pol, model, opt, T, epochs=2, minibatches=2, clip=0.2, value_clip=0.2,
                         entropy_coef=0.01, shuffle=True, perm=perm)
    pol.check()
    assert torch.equal(perm.sort().values, torch.arange(T * B, dtype=torch.int32, device=DEV))  # the last epoch's
    flat = [o for outs in results for o in outs]
    assert len(flat) == 4
    assert float(flat[0]["approx_kl"]) == 0.0 and float(flat[0]["ratio_mean"]) == 1.0
    assert any(float(o["approx_kl"]) > 0.0 for o in flat[1:])
    assert all(np.isfinite(float(o["loss"])) for o in flat)
    assert all(not torch.equal(p.detach(), q) for p, q in zip(model.parameters(), before))
    assert opt.stats()["step"] == 4 and opt.stats()["skipped"] == 0
    pol.close()
