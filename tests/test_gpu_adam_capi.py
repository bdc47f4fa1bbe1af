"""The whole training loop with no Python in the process: examples/c_api_train_demo (a C++ host
program linked to libwab_hip.so) runs three updates of rollout -> GAE -> whitening -> loss and
gradients -> Adam step on 256 envs and dumps the parameters, both moments and the optimizer's
state; the same loop driven from Python (the example's update_device) must leave the same bits."""
import importlib.util
import math
import os
import subprocess

import numpy as np
import pytest
import torch

from wab_gym_amd import policy
from wab_gym_amd.env import BatchedWolvesAndBushesEnv
from wab_gym_amd.wrappers import PragmaticObsWrapper

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEMO = os.path.join(REPO, "examples", "bin", "c_api_train_demo")
DEV = "cuda:0"
B, T, UPDATES, SEED = 256, 16, 3, 0x5EED
M64 = (1 << 64) - 1


def mix64(z):
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def demo_weights():
    """The demo's formulas (examples/c_api_train_demo.cpp): one running state, per layer the weight
    then the bias, uniform in +-1/sqrt(fan_in)."""
    state, out = SEED, {}
    for name, n_out, n_in in zip(policy.LAYERS, (128, 150, 128, 5, 1), (449, 128, 150, 128, 128)):
        bound = 1.0 / math.sqrt(float(n_in))
        for part, shape in (("weight", (n_out, n_in)), ("bias", (n_out,))):
            vals = np.empty(int(np.prod(shape)), np.float32)
            for i in range(vals.size):
                state = mix64((state + 0x9E3779B97F4A7C15) & M64)
                vals[i] = np.float32((((state >> 11) * 2.0 ** -53) * 2.0 - 1.0) * bound)
            out["%s.%s" % (name, part)] = torch.from_numpy(vals.reshape(shape))
    return out


@pytest.mark.gpu
def test_c_caller_trains_to_the_same_bits_as_python(tmp_path):
    if not os.path.exists(DEMO):
        pytest.fail("examples/bin/c_api_train_demo not built (__graft_entry__.build())")
    dump = str(tmp_path / "train.bin")
    r = subprocess.run([DEMO, dump], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().splitlines()
    assert len(lines) == UPDATES + 1 and lines[-1].startswith("OK c_api_train_demo"), r.stdout

    spec = importlib.util.spec_from_file_location("train_actor_critic", os.path.join(REPO, "examples",
                                                                                   "train_actor_critic.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    env = BatchedWolvesAndBushesEnv(None, num_envs=B, seed=SEED, device=DEV)
    wrapper = PragmaticObsWrapper(env)
    wrapper.reset()
    model = mod.Policy(449, 5)
    model.load_state_dict(demo_weights())
    model = model.to(DEV)
    pol = policy.DevicePolicy(model, env)
    opt = policy.DeviceAdam(pol, model, lr=3e-4, max_grad_norm=0.5)
    for u in range(UPDATES):
        out = mod.update_device(wrapper, pol, model, opt, T)
        shown = dict(zip(lines[u].split()[2::2], lines[u].split()[3::2]))  # "update u: loss x  policy x ..."
        assert np.float32(shown["loss"]) == np.float32(float(out["loss"])), (u, lines[u])  # (%.9g names one float32)
    pol.check()

    raw = np.fromfile(dump, dtype=np.uint8)
    by_name = dict(model.named_parameters())
    sets = ([by_name[n].detach() for n in policy.ADAM_TENSORS], opt.exp_avg, opt.exp_avg_sq)
    off = 0
    for what, tensors in zip(("param", "exp_avg", "exp_avg_sq"), sets):
        for name, x in zip(policy.ADAM_TENSORS, tensors):
            want = x.cpu().numpy()
            got = raw[off:off + 4 * want.size].view(np.float32).reshape(want.shape)
            off += 4 * want.size
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (what, name)
            assert what != "exp_avg" or bool((got != 0).any()), name
    assert raw.size == off + 48
    assert raw[off:].tobytes() == bytes(opt._read_state())
    assert opt.stats()["step"] == UPDATES
    pol.close()
