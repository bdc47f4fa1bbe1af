"""wab_policy_grad_packed, wab_policy_grad_ppo_packed, wab_policy_evaluate_packed and
wab_rollout_policy_packed through ctypes alone (no DevicePolicy in the calls under test): every
argument the header says is refused returns WAB_E_INVALID with wab_last_error set, and one
wab_policy_grad_ppo_packed call at N = 129 has the bits of DevicePolicy.ppo_loss_and_grad."""
import ctypes

import numpy as np
import pytest
import torch

import packed_cases as pkc
import policy_cases as pc
import policy_grad_cases as pgc
import test_gpu_ppo as tp
import test_gpu_rollout_policy as trp
from wab_gym_amd import _lib, features

pytestmark = pytest.mark.gpu
DEV = tp.DEV
NET, M, N = pkc.NET_REF, 300, 129
OK, E_INVALID = 0, -1  # WAB_OK, WAB_E_INVALID (include/wab.h)


class Caller:
    """A wab_policy of the net with its weights loaded, a workspace, and the case's source rows as
    floats and as bits, all made with ctypes calls and torch allocations."""

    def __init__(self):
        self.L = L = _lib.load()
        sd = pgc.state_dict(NET)
        shp = _lib.WabPolicyShape(*NET)
        self.p = ctypes.c_void_p()
        assert L.wab_policy_create(ctypes.addressof(shp), 0, ctypes.byref(self.p)) == OK
        self.weights = [sd[k].detach().to(DEV, torch.float32).contiguous() for k in pgc.GRAD_NAMES]
        w = _lib.WabPolicyWeights(*[x.data_ptr() for x in self.weights])
        assert L.wab_policy_load(self.p, ctypes.addressof(w), None) == OK
        need = L.wab_policy_grad_workspace(self.p, N, 0)
        assert need > 0
        self.ws = torch.empty(need, dtype=torch.uint8, device=DEV)
        c = pkc.case(NET, M)
        self.src = {k: tp.dev(c[k], torch.int8 if k == "a" else torch.float32)
                    for k in ("x", "a", "adv", "t", "old_logp", "old_value")}
        P = L.wab_feature_bits_pitch(NET[0])
        assert P == 16
        self.bits = torch.empty((M, P), dtype=torch.int32, device=DEV)
        assert L.wab_features_pack(self.src["x"].data_ptr(), M, NET[0], self.bits.data_ptr(), None, None) == OK
        self.rows = tp.dev(np.random.RandomState(21).permutation(M)[:N], torch.int32)
        self.grads = [torch.zeros_like(x) for x in self.weights]
        self.gw = _lib.WabPolicyWeights(*[g.data_ptr() for g in self.grads])
        self.sums = torch.zeros(8, dtype=torch.float32, device=DEV)
        self.out = [torch.zeros(N, dtype=torch.float32, device=DEV) for _ in range(4)]
        self.loss = _lib.WabPolicyLoss(0.5, 0.01, 0, 1.0, 0, 0)
        self.ppo = _lib.WabPpoConfig(pkc.CLIP, pkc.VALUE_CLIP)

    def args(self, call, **kw):
        s = self.src
        a = dict(bits=self.bits.data_ptr(), actions=s["a"].data_ptr(), weight=s["adv"].data_ptr(),
                 target=s["t"].data_ptr(), old_logp=s["old_logp"].data_ptr(), old_value=s["old_value"].data_ptr(), N=N,
                 loss=ctypes.addressof(self.loss), ppo=ctypes.addressof(self.ppo), grads=ctypes.addressof(self.gw),
                 loss_out=self.sums.data_ptr(), ppo_out=self.sums[4:].data_ptr(), logp=self.out[0].data_ptr(),
                 value=self.out[1].data_ptr(), entropy=self.out[2].data_ptr(), ratio=self.out[3].data_ptr(),
                 ws=self.ws.data_ptr(), ws_bytes=self.ws.numel(), stream=None, rows=self.rows.data_ptr(), M=M)
        a.update(kw)
        order = {"grad": ("bits", "actions", "weight", "target", "N", "loss", "grads", "loss_out", "logp", "value",
                          "entropy", "ws", "ws_bytes", "stream", "rows", "M"),
                 "ppo": ("bits", "actions", "weight", "target", "old_logp", "old_value", "N", "loss", "ppo", "grads",
                         "loss_out", "ppo_out", "logp", "value", "entropy", "ratio", "ws", "ws_bytes", "stream", "rows",
                         "M"),
                 "evaluate": ("bits", "actions", "N", "logp", "value", "entropy", "ws", "ws_bytes", "stream", "rows",
                              "M")}[call]
        return [self.p] + [a[k] for k in order]

    def run(self, call, **kw):
        fn = {"grad": self.L.wab_policy_grad_packed, "ppo": self.L.wab_policy_grad_ppo_packed,
              "evaluate": self.L.wab_policy_evaluate_packed}[call]
        return fn(*self.args(call, **kw))

    def close(self):
        torch.cuda.synchronize()
        self.L.wab_policy_destroy(self.p)


def test_refused_arguments_return_invalid_with_a_message():
    c = Caller()
    L = c.L
    refused = [
        (dict(bits=None), "feature_bits"),                 # NULL bits with N > 0
        (dict(bits=c.bits.data_ptr() + 4), "16-byte aligned"),
        (dict(bits=c.bits.data_ptr() + 8), "16-byte aligned"),
        (dict(M=0), "M outside"),                          # with rows given
        (dict(M=-1), "M outside"),
        (dict(M=1 << 31), "M outside"),
        (dict(rows=c.rows.data_ptr() + 2), "4-byte aligned"),
        # what the float calls refuse already
        (dict(N=-1), "N outside"),
        (dict(N=1 << 31), "N outside"),
        (dict(ws=None), "NULL"),
        (dict(ws_bytes=128), "workspace"),
        (dict(ws=c.ws.data_ptr() + 64), "256-byte aligned"),
        (dict(logp=c.out[0].data_ptr() + 2), "4-byte aligned"),
    ]
    for call in ("grad", "ppo", "evaluate"):
        for kw, word in refused:
            rc = c.run(call, **kw)
            msg = L.wab_last_error().decode()
            assert rc == E_INVALID and word in msg and msg.startswith("wab_policy_"), (call, kw, rc, msg)
            assert "_packed:" in msg, (call, msg)
    for kw, word in ((dict(actions=None), "NULL"), (dict(grads=None), "NULL"), (dict(loss=None), "NULL")):
        for call in ("grad", "ppo"):
            assert c.run(call, **kw) == E_INVALID and word in L.wab_last_error().decode(), (call, kw)
    assert c.run("ppo", old_logp=None) == E_INVALID and "old_logp" in L.wab_last_error().decode()
    assert c.run("ppo", ppo=None) == E_INVALID
    # rows == NULL: the contiguous rows, and M is ignored
    assert c.run("evaluate", rows=None, M=-7) == OK and L.wab_last_error().decode() == ""
    # N = 0 stays valid, bits NULL included: zero gradients and losses
    for g in c.grads:
        g.fill_(1.0)
    c.sums.fill_(1.0)
    assert c.run("ppo", N=0, rows=None, bits=None) == OK and L.wab_last_error().decode() == ""
    assert c.run("evaluate", N=0, bits=None) == OK
    torch.cuda.synchronize()
    assert all(float(g.abs().max()) == 0.0 for g in c.grads) and float(c.sums.abs().max()) == 0.0
    c.close()


def test_rollout_packed_refuses_missing_or_misaligned_bits():
    import test_gpu_packed_rollout as tpr

    B, T = 64, 2
    env, w, pol = trp.closed_loop(B, pc.OPTS_REF)
    L = _lib.load()
    f0 = w.observation().clone()
    last = torch.zeros((B, 449), device=DEV)
    before = env.state()
    bits = torch.zeros((T, B, 16), dtype=torch.int32, device=DEV)
    rc, _ = tpr.c_rollout_packed(env, pol, f0, T, None, last)
    assert rc == E_INVALID and "feature_bits" in L.wab_last_error().decode()
    assert L.wab_last_error().decode().startswith("wab_rollout_policy_packed:")
    rc, _ = tpr.c_rollout_packed(env, pol, f0, T, bits.view(-1)[1:], last)
    assert rc == E_INVALID and "16-byte aligned" in L.wab_last_error().decode()
    torch.cuda.synchronize()
    for k, v in env.state().items():  # nothing ran
        assert np.array_equal(v, before[k]), k


def test_one_c_call_has_the_python_paths_bits():
    c = Caller()
    L = c.L
    pol = tp.policy_for(NET)
    s = c.src
    kw = dict(clip=pkc.CLIP, old_value=s["old_value"], value_clip=pkc.VALUE_CLIP, value_coef=0.5, entropy_coef=0.01,
              return_rows=True)
    for rows in (c.rows, None):
        n = N
        if rows is None:  # the contiguous call: rows 0 .. N - 1 of the same arrays
            assert c.run("ppo", rows=None, M=0) == OK, L.wab_last_error().decode()
            want = pol.ppo_loss_and_grad(*[s[k][:n] for k in ("x", "a", "adv", "t", "old_logp")],
                                         **dict(kw, old_value=s["old_value"][:n]))
        else:
            assert c.run("ppo") == OK, L.wab_last_error().decode()
            want = pol.ppo_loss_and_grad(s["x"], s["a"], s["adv"], s["t"], s["old_logp"], rows=rows, **kw)
        v = ctypes.c_uint64(7)
        assert L.wab_policy_grad_bad_rows(c.p, c.ws.data_ptr(), None, ctypes.byref(v)) == OK and v.value == 0
        assert L.wab_policy_grad_bad_actions(c.p, c.ws.data_ptr(), None, ctypes.byref(v)) == OK and v.value == 0
        pol.check()
        for k, g in zip(pgc.GRAD_NAMES, c.grads):
            assert tp.same(g, want["grads"][k]) and bool((g != 0).any()), k
        for j, k in enumerate(("loss_policy", "loss_value", "entropy", "loss")):
            assert tp.same(c.sums[j], want[k]), k
        assert tp.same(c.sums[4:], want["ppo_sums"])
        for o, k in zip(c.out, ("logp", "value", "entropy_rows", "ratio")):
            assert tp.same(o, want[k]), k
    # the Python path on the same bits, and evaluate through the same index
    got = pol.ppo_loss_and_grad(c.bits, s["a"], s["adv"], s["t"], s["old_logp"], **kw)
    want = pol.ppo_loss_and_grad(s["x"], s["a"], s["adv"], s["t"], s["old_logp"], **kw)
    assert not tp.same_grads(got["grads"], want["grads"]) and tp.same(got["ratio"], want["ratio"])
    assert torch.equal(c.bits, features.pack_features(s["x"]))
    outs = [torch.zeros(N, dtype=torch.float32, device=DEV) for _ in range(3)]
    assert c.run("evaluate", logp=outs[0].data_ptr(), value=outs[1].data_ptr(), entropy=outs[2].data_ptr()) == OK
    ev = pol.evaluate(s["x"], s["a"], rows=c.rows)
    torch.cuda.synchronize()
    for o, k in zip(outs, ("logp", "value", "entropy")):
        assert tp.same(o, ev[k]), k
    pol.close()
    c.close()
