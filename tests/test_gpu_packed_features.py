"""Packed feature rows on the GPU (include/wab.h, WAB_HAS_PACKED_FEATURES): wab_features_pack and
wab_features_unpack against the NumPy statement of the format, and the packed evaluate, gradient
and PPO calls against the float calls on the same binary rows and the same loaded weights.  Both
sides of every comparison run on the GPU and the criterion is bitwise equality: 0 and 1 are exact
in bf16 and no sum changes its order."""
import ctypes

import numpy as np
import pytest
import torch

import packed_cases as pkc
import policy_grad_cases as pgc
import test_gpu_ppo as tp
from wab_gym_amd import _lib, features, policy

pytestmark = pytest.mark.gpu
DEV = tp.DEV
KEYS = ("x", "a", "adv", "t", "old_logp", "old_value")
GUARD = 0x5A5A5A5A


def on_device(c):
    return {k: tp.dev(c[k], torch.int8 if k == "a" else torch.float32) for k in KEYS}


def flat(r):
    """A result dict as {name: tensor}, the gradients by their names."""
    out = {k: v for k, v in r.items() if k != "grads"}
    out.update({"grads." + k: v for k, v in r.get("grads", {}).items()})
    return out


def assert_same(got, want, what):
    got, want = flat(got), flat(want)
    assert sorted(got) == sorted(want), what
    for k, w in want.items():
        assert tp.same(got[k], w), (what, k)


def counts(pol):
    """(bad actions, bad rows) of the latest call on the policy's workspace."""
    L, out = _lib.load(), []
    for fn in (L.wab_policy_grad_bad_actions, L.wab_policy_grad_bad_rows):
        v = ctypes.c_uint64(99)
        fn(pol._p, pol._grad_ws.data_ptr(), pol.env._stream(), ctypes.byref(v))
        out.append(int(v.value))
    return tuple(out)


def three_calls(pol, feats, s, rows=None, **kw):
    """evaluate, loss_and_grad and ppo_loss_and_grad on `feats` (float rows or bits): every output
    and the two bad counts after each call."""
    out = {"evaluate": pol.evaluate(feats, s["a"], rows=rows)}
    out["evaluate"]["counts"] = torch.tensor(counts(pol))
    out["grad"] = pol.loss_and_grad(feats, s["a"], s["adv"], s["t"], value_coef=0.5, entropy_coef=0.01, return_rows=True,
                                    rows=rows, **kw)
    out["grad"]["counts"] = torch.tensor(counts(pol))
    out["ppo"] = pol.ppo_loss_and_grad(feats, s["a"], s["adv"], s["t"], s["old_logp"], clip=pkc.CLIP,
                                       old_value=s["old_value"], value_clip=pkc.VALUE_CLIP, value_coef=0.5,
                                       entropy_coef=0.01, reduction="mean", return_rows=True, rows=rows, **kw)
    out["ppo"]["counts"] = torch.tensor(counts(pol))
    return out


def assert_three_same(got, want, what):
    for call in ("evaluate", "grad", "ppo"):
        assert_same(got[call], want[call], "%s %s" % (what, call))


# ------------------------------------------------------------------ 3. pack and unpack
@pytest.mark.parametrize("F", pkc.PACK_F)
def test_pack_and_unpack_are_the_numpy_format(F):
    P = pkc.pitch(F)
    L = _lib.load()
    for n in pkc.PACK_ROWS:
        x = pkc.binary_rows(F, n).copy()
        planted = 0
        if n >= 63:  # 0.5, -0.0 and NaN in the first, a middle and the last element of the array
            for (r, k), v in zip(((0, 0), (n // 2, F // 2), (n - 1, F - 1), (n // 3, F - 1)), (0.5, -0.0, np.nan, 0.5)):
                x[r, k] = v
            planted = features.nonbinary_reference(x)
            assert planted >= 3
        want = features.pack_reference(x)
        # guard dwords before and after the output; the input at a 16-byte aligned and at an odd address
        for shift in (0, 1):
            buf = torch.full((4 + n * P + 4,), GUARD, dtype=torch.int32, device=DEV)
            src = torch.zeros(4 + n * F + shift, dtype=torch.float32, device=DEV)
            xs = src[4 + shift:4 + shift + n * F].view(n, F)
            xs.copy_(torch.from_numpy(x))
            assert n == 0 or xs.data_ptr() % 16 == 4 * shift
            count = torch.full((1,), 1000, dtype=torch.int64, device=DEV)
            rc = L.wab_features_pack(xs.data_ptr() if n else None, n, F, buf[4:].data_ptr() if n else None,
                                     count.data_ptr(), None)
            assert rc == 0, L.wab_last_error()
            torch.cuda.synchronize()
            got = buf.cpu().numpy()
            assert (got[:4] == GUARD).all() and (got[4 + n * P:] == GUARD).all(), (n, shift)
            assert np.array_equal(got[4:4 + n * P].reshape(n, P), want), (n, shift)
            assert int(count.item()) == 1000 + planted, (n, shift)
            # a NULL counter is allowed
            buf2 = torch.full((n * P + 4,), GUARD, dtype=torch.int32, device=DEV)
            assert L.wab_features_pack(xs.data_ptr() if n else None, n, F, buf2.data_ptr() if n else None, None, None) == 0
            assert np.array_equal(buf2.cpu().numpy()[:n * P].reshape(n, P), want)
            # unpack: exactly 0.0f / 1.0f, nothing past the output, pad bits ignored
            bits = torch.from_numpy(want.copy()).to(DEV)
            dirty = torch.from_numpy((want.view(np.uint32) | ~features.pack_reference(np.ones_like(x)).view(np.uint32))
                                     .view(np.int32)).to(DEV)
            for b in (bits, dirty):
                dst = torch.full((4 + n * F + shift + 4,), GUARD, dtype=torch.int32, device=DEV)
                o = dst[4 + shift:4 + shift + n * F]
                rc = L.wab_features_unpack(b.data_ptr() if n else None, n, F, o.data_ptr() if n else None, None)
                assert rc == 0, L.wab_last_error()
                got = dst.cpu().numpy()
                assert (got[:4 + shift] == GUARD).all() and (got[4 + shift + n * F:] == GUARD).all(), (n, shift)
                u = got[4 + shift:4 + shift + n * F].view(np.uint32).reshape(n, F)
                assert ((u == 0) | (u == 0x3F800000)).all()
                assert np.array_equal(u != 0, x.view(np.uint32) != 0), (n, shift)


def test_python_pack_checks_and_round_trips():
    x = tp.dev(pkc.binary_rows(449, 257))
    bits = features.pack_features(x.view(1, 257, 449))
    assert bits.shape == (1, 257, 16) and bits.dtype == torch.int32
    assert np.array_equal(bits.cpu().numpy()[0], features.pack_reference(pkc.binary_rows(449, 257)))
    assert torch.equal(features.unpack_features(bits, 449), x.view(1, 257, 449))
    out = torch.empty_like(bits)
    assert features.pack_features(x.view(1, 257, 449), out=out) is out and torch.equal(out, bits)
    y = x.clone()
    y[3, 7] = 0.25
    y[200, 448] = -0.0
    with pytest.raises(ValueError, match="2 elements"):
        features.pack_features(y)
    features.pack_features(y, check=False)
    L = _lib.load()
    for args, word in (((None, 4, 449, bits.data_ptr(), None, None), "NULL"),
                       ((x.data_ptr(), 4, 449, None, None, None), "NULL"),
                       ((x.data_ptr(), 4, 449, bits.data_ptr() + 4, None, None), "16-byte"),
                       ((x.data_ptr() + 2, 4, 449, bits.data_ptr(), None, None), "4-byte"),
                       ((x.data_ptr(), 4, 0, bits.data_ptr(), None, None), "F outside"),
                       ((x.data_ptr(), 4, (1 << 20) + 1, bits.data_ptr(), None, None), "F outside"),
                       ((x.data_ptr(), -1, 449, bits.data_ptr(), None, None), "n_rows")):
        assert L.wab_features_pack(*args) == -1 and word in L.wab_last_error().decode(), args
    assert L.wab_features_unpack(None, 4, 449, x.data_ptr(), None) == -1
    assert L.wab_features_unpack(bits.data_ptr() + 8, 4, 449, x.data_ptr(), None) == -1
    assert "wab_features_unpack" in L.wab_last_error().decode()


# ------------------------------------------------------------------ 4. evaluate, gradients, PPO
@pytest.mark.parametrize("net", pkc.NETS, ids=str)
def test_packed_calls_have_the_float_calls_bits(net):
    pol = tp.policy_for(net)
    for n in pkc.ROWS:
        s = on_device(pkc.case(net, n))
        bits = features.pack_features(s["x"])
        assert bits.shape == (n, pkc.pitch(net[0]))
        want = three_calls(pol, s["x"], s)
        got = three_calls(pol, bits, s)
        assert_three_same(got, want, "%s N=%d" % (net, n))
        pol.check()
        if n >= 128 and net != (1, 1, 1, 1, 5):
            assert bool((got["ppo"]["grads"]["affine1.weight"] != 0).any())
        if n == 257:  # rows over several chunks and slabs, and a [T, B, P] view
            assert_three_same(three_calls(pol, bits, s, chunk_rows=128), three_calls(pol, s["x"], s, chunk_rows=128),
                              "%s N=257 chunk_rows=128" % (net,))
        if n == 128:
            seg = {k: v.view(2, 64, *v.shape[1:]) for k, v in s.items()}
            r = three_calls(pol, bits.view(2, 64, -1), seg)
            assert r["ppo"]["logp"].shape == (2, 64)
            assert tp.same(r["ppo"]["logp"].view(128), want["ppo"]["logp"])
            assert not tp.same_grads(r["ppo"]["grads"], want["ppo"]["grads"])
    pol.close()


def test_packed_into_and_accumulate():
    net, n = pkc.NET_REF, 129
    pol = tp.policy_for(net)
    s = on_device(pkc.case(net, n))
    bits = features.pack_features(s["x"])
    _, m1 = tp.model_of()
    _, m2 = tp.model_of()
    for feats, model in ((s["x"], m1), (bits, m2)):
        for acc in (False, True):
            pol.ppo_loss_and_grad(feats, s["a"], s["adv"], s["t"], s["old_logp"], clip=pkc.CLIP, into=model,
                                  accumulate=acc)
    for (k, p1), (_, p2) in zip(m1.named_parameters(), m2.named_parameters()):
        assert tp.same(p1.grad, p2.grad) and bool((p1.grad != 0).any()), k
    pol.check()
    pol.close()


# ------------------------------------------------------------------ 5. gather
@pytest.mark.parametrize("net", (pkc.NET_REF, (560, 130, 8, 8, 5)), ids=str)
def test_packed_gather_has_the_float_gathers_bits(net):
    M, N = 300, 129
    pol = tp.policy_for(net)
    c = {k: v.copy() for k, v in pkc.case(net, M).items()}
    rows = pkc.gather_index(N, M)
    c["a"][rows[3]] = net[4]  # one bad action, at a row the index reaches
    s = on_device(c)
    bits = features.pack_features(s["x"])
    r32 = tp.dev(rows, torch.int32)
    want = three_calls(pol, s["x"], s, rows=r32)
    got = three_calls(pol, bits, s, rows=r32)
    assert_three_same(got, want, "%s gather" % (net,))
    bad_actions, bad_rows = (int(v) for v in got["ppo"]["counts"])
    assert bad_rows == 1 and bad_actions == int((rows == rows[3]).sum())
    with pytest.raises(IndexError):
        pol.check()
    assert got["ppo"]["logp"].shape == (N,)
    pol.close()


def test_a_captured_packed_graph_reads_the_index_at_replay():
    net, M, N = pkc.NET_REF, 300, 129
    pol = tp.policy_for(net)
    s = on_device(pkc.case(net, M))
    bits = features.pack_features(s["x"])
    rng = np.random.RandomState(14)
    perms = [tp.dev(rng.permutation(M), torch.int32) for _ in range(3)]
    buf = perms[0].clone()

    def ppo(feats, rows):
        return pol.ppo_loss_and_grad(feats, s["a"], s["adv"], s["t"], s["old_logp"], clip=pkc.CLIP,
                                     old_value=s["old_value"], value_clip=pkc.VALUE_CLIP, entropy_coef=0.01,
                                     reduction="mean", return_rows=True, rows=rows)

    ppo(bits, buf[20:20 + N])  # (the workspace exists before the capture)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        cap = ppo(bits, buf[20:20 + N])
    for p in perms[1:]:
        buf.copy_(p)
        g.replay()
        torch.cuda.synchronize()
        got = {k: (v.clone() if k != "grads" else {q: x.clone() for q, x in v.items()}) for k, v in cap.items()}
        assert_same(got, ppo(s["x"], p[20:20 + N].clone()), "replay after a new permutation")
    pol.check()
    pol.close()


# ------------------------------------------------------------------ 8. pad bits
def test_pad_bits_of_the_input_are_ignored():
    net, n = pkc.NET_REF, 129
    pol = tp.policy_for(net)
    s = on_device(pkc.case(net, n))
    bits = features.pack_features(s["x"])
    pad = torch.from_numpy((~features.pack_reference(np.ones((1, net[0]), np.float32)).view(np.uint32)).view(np.int32))
    assert int(np.unpackbits(pad.numpy().view(np.uint8)).sum()) == 512 - 449
    dirty = bits | pad.to(DEV)
    assert not torch.equal(dirty, bits)
    want = three_calls(pol, s["x"], s)
    assert_three_same(three_calls(pol, dirty, s), want, "pad bits set")
    r32 = tp.dev(np.arange(n)[::-1].copy(), torch.int32)
    assert_three_same(three_calls(pol, dirty, s, rows=r32), three_calls(pol, s["x"], s, rows=r32), "pad bits set, gathered")
    pol.check()
    pol.close()
