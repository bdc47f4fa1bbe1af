"""wab_rollout_policy_packed (PragmaticObsWrapper.rollout_policy(store_features="packed")) against
wab_rollout_policy on a twin env: the same seed, the same policy, the default options with
max_turns = 5 so that envs reset inside the segment.  One env stores float rows, the other packed
rows; everything the two calls write is compared bit for bit, over two consecutive calls.  Then
examples/train_ppo.py's update with packed=True against packed=False."""
import ctypes

import numpy as np
import pytest
import torch

import packed_cases as pkc
import policy_cases as pc
import test_gpu_ppo as tp
import test_gpu_rollout_policy as trp
from wab_gym_amd import _lib, features, policy
from wab_gym_amd.env import BatchedWolvesAndBushesEnv
from wab_gym_amd.wrappers import PragmaticObsWrapper

pytestmark = pytest.mark.gpu
DEV = tp.DEV
F, P = 449, 16
KEYS = ("actions", "value", "probs", "reward", "done", "returns")


def assert_twin_segments(a, wa, ea, b, wb, eb, B, T, what):
    """a: the float env's result, b: the packed env's."""
    assert b["features"] is None and a["features"].shape == (T, B, F), what
    bits = b["feature_bits"]
    assert bits.shape == (T, B, P) and bits.dtype == torch.int32 and bits.is_contiguous(), what
    assert tp.same(features.unpack_features(bits, F), a["features"]), what
    ref = torch.from_numpy(features.pack_reference(a["features"].cpu().numpy()))
    assert torch.equal(bits.cpu(), ref), what  # (the pad bits are zero: pack_reference's are)
    u = bits.cpu().numpy().view(np.uint32)
    assert not (u[..., 14] >> np.uint32(1)).any() and not u[..., 15].any(), what
    for k in KEYS:
        assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), (what, k)
    assert tp.same(wa.features, wb.features), what
    assert ea.counters() == eb.counters(), what
    sa, sb = ea.state(), eb.state()
    for k, v in sa.items():
        assert np.array_equal(v, sb[k]), (what, k)


@pytest.mark.parametrize("B,T", [(64, 1), (68, 3), (132, 7)])  # B = 68: a last group of 4 active envs
def test_fused_packed_rollout_is_the_float_rollout(B, T):
    ea, wa, pa = trp.closed_loop(B, pc.OPTS_REF)
    eb, wb, pb = trp.closed_loop(B, pc.OPTS_REF)
    assert trp.fused_flag(ea, pa) == 1 and trp.fused_flag(eb, pb) == 1
    for call in (1, 2):  # the second call continues from what the first left
        a = wa.rollout_policy(pa, T, return_probs=True, fused=True)
        b = wb.rollout_policy(pb, T, return_probs=True, fused=True, store_features="packed")
        assert_twin_segments(a, wa, ea, b, wb, eb, B, T, "call %d" % call)
    assert eb.counters()["rollout_launches"] == 2 and eb.counters()["rollout_step_calls"] == 0
    if T == 7:
        assert int(b["done"].sum()) > 0  # resets happened inside the segment
    with pytest.raises(ValueError):
        wb.rollout_policy(pb, T, store_features="bits")


def c_rollout_packed(env, pol, f0, T, bits, last):
    B, A = env.num_envs, pol.n_actions
    out = {"actions": torch.full((T, B), -1, dtype=torch.int8, device=DEV), "value": torch.empty((T, B), device=DEV),
           "probs": torch.empty((T, B, A), device=DEV), "reward": torch.empty((T, B), device=DEV),
           "done": torch.empty((T, B), dtype=torch.uint8, device=DEV), "returns": torch.empty((T, B), device=DEV),
           "scal": torch.empty((3, T, B), dtype=torch.uint8, device=DEV)}
    s = out["scal"]
    st = _lib.WabObs(None, s[0].data_ptr(), s[1].data_ptr(), s[2].data_ptr())
    rc = _lib.load().wab_rollout_policy_packed(
        env._h, pol._p, f0.data_ptr(), T, ctypes.addressof(st), out["actions"].data_ptr(), out["value"].data_ptr(),
        out["probs"].data_ptr(), out["reward"].data_ptr(), out["done"].data_ptr(),
        None if bits is None else bits.data_ptr(), last.data_ptr(), 0.99, None, out["returns"].data_ptr(), env._stream())
    return rc, out


def test_unfused_packed_rollout_is_the_float_rollout():
    B, T = 68, 3
    kw = {"wolf_slots": 16}
    ea, wa, pa = trp.closed_loop(B, pc.OPTS_REF, **kw)
    eb, wb, pb = trp.closed_loop(B, pc.OPTS_REF, **kw)
    assert trp.fused_flag(ea, pa) == 0 and trp.fused_flag(eb, pb) == 0
    for call in (1, 2):
        a = wa.rollout_policy(pa, T, return_probs=True)
        b = wb.rollout_policy(pb, T, return_probs=True, store_features="packed")
        assert_twin_segments(a, wa, ea, b, wb, eb, B, T, "loop, call %d" % call)
    # the C entry point itself runs the 2 T launches there, a pack launch after each step
    ec, wc, pcl = trp.closed_loop(B, pc.OPTS_REF, **kw)
    ed, wd, pd = trp.closed_loop(B, pc.OPTS_REF, **kw)
    feats = torch.empty((T, B, F), device=DEV)
    last_c, last_d = torch.zeros((B, F), device=DEV), torch.zeros((B, F), device=DEV)
    rc, c = trp.c_rollout(ec, pcl, wc.observation().clone(), T, feats, last_c)
    assert rc == 0, _lib.load().wab_last_error()
    bits = torch.full((T, B, P), -1, dtype=torch.int32, device=DEV)
    rc, d = c_rollout_packed(ed, pd, wd.observation().clone(), T, bits, last_d)
    assert rc == 0, _lib.load().wab_last_error()
    torch.cuda.synchronize()
    for k in KEYS:
        assert torch.equal(c[k], d[k]), k
    assert tp.same(last_c, last_d)
    assert torch.equal(bits.cpu(), torch.from_numpy(features.pack_reference(feats.cpu().numpy())))
    assert ec.counters() == ed.counters() and ed.counters()["rollout_step_calls"] == 1


# ------------------------------------------------------------------ 10. the example
@pytest.mark.parametrize("shuffle", [False, True])
def test_packed_update_leaves_the_float_updates_parameters(shuffle):
    B, T = 64, 4
    mod, _ = tp.model_of()
    params = []
    for packed in (False, True):
        _, model = tp.model_of(seed=3)
        env = BatchedWolvesAndBushesEnv(dict(pc.OPTS_REF), num_envs=B, seed=pc.SEED, device=DEV)
        wrapper = PragmaticObsWrapper(env)
        wrapper.reset()
        pol = policy.DevicePolicy(model, env)
        opt = policy.DeviceAdam(pol, model, lr=1e-3, max_grad_norm=0.5)
        torch.manual_seed(11)  # (the same permutations in both runs)
        perm = torch.empty(T * B, dtype=torch.int32, device=DEV) if shuffle else None
        res = mod.update(wrapper, pol, model, opt, T, epochs=2, minibatches=2, shuffle=shuffle, perm=perm, packed=packed)
        pol.check()
        assert len(res) == 2 and len(res[0]) == 2
        assert opt.stats()["step"] == 4
        params.append([p.detach().clone() for p in model.parameters()])
        pol.close()
    for p0, p1 in zip(*params):
        assert tp.same(p0, p1)
    _, fresh = tp.model_of(seed=3)
    assert any(not torch.equal(p, q) for p, q in zip(params[1], fresh.parameters()))  # the update moved them
