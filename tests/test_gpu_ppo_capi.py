"""wab_policy_evaluate and wab_policy_grad_ppo with no Python in the process:
examples/c_api_ppo_demo (a C++ host program linked to libwab_hip.so) runs c_api_grad_demo's
17-33-33-33-5 net over 200 made-up rows, checks itself that a ratio of 1 gives wab_policy_grad's
gradients bit for bit, and dumps a second call with shifted old_logp and a clipped value loss; the
dump is compared here with the contract under tests/test_gpu_ppo.py's gate."""
import os
import subprocess

import numpy as np
import pytest
import torch

import policy_grad_cases as pgc
import ppo_cases as ppc
from test_gpu_policy_grad_capi import A, N, demo_inputs
from wab_gym_amd import policy

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEMO = os.path.join(REPO, "examples", "bin", "c_api_ppo_demo")
CLIP, VALUE_CLIP = 0.2, 0.25


@pytest.mark.gpu
def test_c_caller_gets_the_contract_ppo_gradients(tmp_path):
    if not os.path.exists(DEMO):
        pytest.fail("examples/bin/c_api_ppo_demo not built (__graft_entry__.build())")
    dump = str(tmp_path / "ppo.bin")
    r = subprocess.run([DEMO, dump], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr  # (its own bit-for-bit check against wab_policy_grad included)
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 13 and lines[-1].startswith("OK "), r.stdout
    assert lines[10].split()[0] == "loss" and lines[11].split()[0] == "ppo"
    sd, x, a, adv, t = demo_inputs()
    raw = np.fromfile(dump, dtype=np.float32)
    sizes = [int(np.prod(sd[k].shape)) for k in pgc.GRAD_NAMES]
    off = sum(sizes)
    assert raw.size == off + 8 + 3 * N
    sums = raw[off:off + 8]
    old_logp, old_value, ratio = (raw[off + 8 + i * N:off + 8 + (i + 1) * N] for i in range(3))
    # the demo's shifts of the device's own logp and value (examples/c_api_ppo_demo.cpp)
    base = policy.reference_loss_and_grad(sd, x, a, adv, t)
    i = np.arange(N)
    assert float(np.abs(old_logp - (base["logp"].numpy() + (i % 5 - 2) * 0.25)).max()) < 1e-4
    assert float(np.abs(old_value - (base["value"].numpy() + (i % 4 - 1.5) * 0.4)).max()) < 1e-4
    args = (sd, x, a, adv, t, old_logp, CLIP, old_value, VALUE_CLIP, 0.5, 0.01, "smooth_l1")
    ref = policy.reference_ppo_loss_and_grad(*args)
    E = ppc.cost_of(ref, ppc.fp32_ppo_loss_and_grad(*args))
    pos = 0
    for line, k, size in zip(lines, pgc.GRAD_NAMES, sizes):
        want = ref["grads"][k]
        got = raw[pos:pos + size].reshape(tuple(want.shape))
        pos += size
        word, name, total = line.split()
        assert (word, name) == ("sum", k)
        assert abs(float(total) - float(got.astype(np.float64).sum())) <= 1e-9 * max(1.0, abs(float(total)))
        err = float((torch.as_tensor(got).double() - want).abs().max())
        print("%s: err %.3e  E %.3e  ratio %.4f" % (k, err, E[k], err / E[k] if E[k] else 0.0))
        assert err <= 0.5 * E[k], (k, err, E[k])
    for j, k in enumerate(("loss_policy", "loss_value", "entropy", "loss")):
        err = abs(float(sums[j]) - float(ref["loss"][j]))
        print("%s: err %.3e  E %.3e" % (k, err, E[k]))
        assert err <= 0.5 * E[k], (k, err, E[k])
    err = float(np.abs(ratio.astype(np.float64) - ref["ratio"].numpy()).max())
    print("ratio: err %.3e  E %.3e" % (err, E["ratio"]))
    assert err <= 0.5 * E["ratio"]
    # the counts exactly, the two sums under the gate; rows of every kind took part
    assert float(sums[4]) == float(ref["ppo"][0]) and float(sums[6]) == float(ref["ppo"][2])
    assert 0 < float(sums[4]) < N and 0 < float(sums[6]) < N and A == 5
    for j, k in ((5, "k3_sum"), (7, "ratio_sum")):
        err = abs(float(sums[j]) - float(ref["ppo"][j - 4]))
        print("%s: err %.3e  E %.3e" % (k, err, E[k]))
        assert err <= 0.5 * E[k], (k, err, E[k])
