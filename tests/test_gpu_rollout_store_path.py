"""The rollout kernel's obs store path (wab_step_small, multi-step build) at the batch shapes
where its whole-group / partial-group branch can go wrong.

A multi-step launch stores step t's obs during step t + 1 (W0 and W2, from the bit-stream of the
other parity, clearing it as they read) and the last step's at its end (all four waves).  A
workgroup whose 64-env group is whole takes a straight-line path with a compile-time unit count
(default 11x11 geometry); a partial group (only the launch's last workgroup can be one) and
the runtime-geometry instances take the general, per-unit-masked path.  The shapes below are:
only a partial group (B = 16), only whole groups (64, 128), a whole group followed by a partial
one in the same launch (80, 208); group 1's slice starts 64 bytes into a 128-byte line (64 *
363 = 181.5 lines); T = 1 is the per-step kernel, T = 2 the last-step store after one
in-loop store, T = 3, 4 both stream parities.  Every output of every step is compared with the
C oracle (oracle/wab_oracle.c) and, bit for bit, with a twin env stepped by `wab_step`.
B = 65536 is tests/test_gpu_bench_parity.py's.
"""
import ctypes

import numpy as np
import pytest

from backends import SEED

pytestmark = pytest.mark.gpu


def _env(opts, B, slots=8, stride=0):
    from wab_gym_amd.env import BatchedWolvesAndBushesEnv

    env = BatchedWolvesAndBushesEnv(opts, num_envs=B, seed=SEED, device="cuda:0", autoreset=True,
                                    validate_actions=False, plane_stride=stride, wolf_slots=slots)
    env.reset()
    return env


def _oracle(opts, B, stride=0):
    from oracle.oracle import OracleBatch

    orc = OracleBatch(opts, B, SEED, 0, True, stride)
    orc.reset()
    return orc


def _actions(seed, T, B, n_actions):
    return np.random.RandomState(seed).randint(n_actions, size=(T, B)).astype(np.int8)


def _eq(got, want, what):
    got = got.cpu().numpy()
    want = np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not np.array_equal(got, want.astype(got.dtype)):
        bad = np.argwhere(got != want.astype(got.dtype))[:4].tolist()
        raise AssertionError("%s differs at %s" % (what, bad))


def _rollouts_vs_oracle_and_steps(opts, B, T, slots, launches=2):
    """`launches` chained rollouts of T steps: every step's planes, scalars, reward and done
    against the oracle's step and against a twin env's wab_step; then the hidden state."""
    import torch

    roll, step, orc = _env(opts, B, slots), _env(opts, B, slots), _oracle(opts, B)
    assert roll.step_kernel == "small" and step.step_kernel == "small"
    for k in range(launches):
        a = _actions(1000 * T + 10 * B + k, T, B, roll.n_actions)
        before = roll.counters()
        planes, scal, rew, done = roll.rollout(torch.as_tensor(a))
        c = roll.counters()
        assert c["rollout_launches"] - before["rollout_launches"] == 1, "not the one-launch path"
        for t in range(T):
            what = "B %d T %d launch %d step %d " % (B, T, k, t)
            op, of, orl, ost, orew, odone = orc.step(a[t])
            _eq(planes[t], op, what + "planes vs oracle")
            _eq(scal[t], np.stack([of, orl, ost]), what + "scalars vs oracle")
            _eq(rew[t], orew, what + "reward vs oracle")
            _eq(done[t], odone, what + "done vs oracle")
            obs, srew, sdone, _ = step.step(torch.as_tensor(a[t]))
            assert torch.equal(planes[t], step._obs["planes"]), what + "planes vs wab_step"
            assert torch.equal(scal[t], step._obs["scalars"]), what + "scalars vs wab_step"
            assert torch.equal(rew[t], srew), what + "reward vs wab_step"
            assert torch.equal(done[t], sdone.to(torch.uint8)), what + "done vs wab_step"
    gs, ss, os_ = roll.state(), step.state(), orc.state()
    for key in ("x", "y", "turn", "n_wolves", "episode"):
        assert np.array_equal(gs[key], os_[key]) and np.array_equal(gs[key], ss[key]), key
    assert np.array_equal(gs["food"].view(np.uint64), os_["food"].view(np.uint64))
    c = roll.counters()
    assert c["wolf_overflow"] == 0 and c["eaten_overflow"] == 0 and c["handoff_timeouts"] == 0, c


@pytest.mark.parametrize("T", [1, 2, 3, 4])
@pytest.mark.parametrize("B", [16, 64, 80, 128, 208])
def test_default_geometry_rollout_every_step(B, T):
    """Default 11x11 (the G = 11 instances): planes + scalars + reward + done of every step."""
    _rollouts_vs_oracle_and_steps(None, B, T, 8)


def test_runtime_geometry_rollout_every_step():
    """9x9 with 32 wolf slots: the runtime-geometry (G = 0) instance and its wolf-carry LDS
    layout; a whole group followed by a partial one."""
    _rollouts_vs_oracle_and_steps({"width": 9, "height": 9}, 80, 3, 32)


def test_rollout_features_with_and_without_planes():
    """wab_rollout_features, three chained launches of T = 3 at B = 80: without planes the
    stream is cleared without being stored; a unit left uncleared would show as stale bits in a
    later step's features.  Features, scalars, reward, done and returns equal with and without
    planes, and the planes (where stored) and features equal the oracle's."""
    import torch

    from oracle import oracle as O

    B, T = 80, 3
    with_p, without_p, orc = _env(None, B), _env(None, B), _oracle(None, B)
    vm = np.zeros((B, 11, 11), np.uint8)
    for k in range(3):
        a = _actions(7000 + k, T, B, with_p.n_actions)
        rp = with_p.rollout_features(torch.as_tensor(a), gamma=0.99, store_planes=True)
        rn = without_p.rollout_features(torch.as_tensor(a), gamma=0.99, store_planes=False)
        assert rn["planes"] is None and rp["planes"] is not None
        for name in ("features", "scalars", "reward", "done", "returns"):
            assert torch.equal(rp[name], rn[name]), (k, name)
        for t in range(T):
            what = "launch %d step %d " % (k, t)
            op, of, orl, ost, orew, odone = orc.step(a[t])
            _eq(rp["planes"][t], op, what + "planes vs oracle")
            _eq(rn["features"][t], O.featurize(op, of, orl, ost, vm, 11, 11), what + "features vs oracle")
            _eq(rn["reward"][t], orew, what + "reward vs oracle")
            _eq(rn["done"][t], odone, what + "done vs oracle")


@pytest.mark.parametrize("B", [80, 128])
def test_no_store_leaves_its_slice(B):
    """wab_rollout through the C-ABI as bench.py calls it, T = 3, with planes, scalars, reward
    and done carved out of larger buffers pre-filled with 0xA5: every byte outside the [T][B]
    extents is still 0xA5 afterwards, and the planes inside equal the oracle's."""
    import torch

    from wab_gym_amd import _lib

    T, PAD = 3, 4096
    env, orc = _env(None, B), _oracle(None, B)
    OB = 3 * env.W * env.S
    dev = env.device
    sizes = {"planes": T * B * OB, "food": T * B, "role": T * B, "status": T * B, "reward": 4 * T * B, "done": T * B}
    bufs = {k: torch.full((PAD + n + PAD,), 0xA5, dtype=torch.uint8, device=dev) for k, n in sizes.items()}
    ptr = {k: bufs[k].data_ptr() + PAD for k in sizes}
    assert ptr["planes"] % 16 == 0 and ptr["reward"] % 4 == 0
    a = _actions(9000 + B, T, B, env.n_actions)
    ad = torch.as_tensor(a, device=dev).contiguous()
    o = _lib.WabObs(ptr["planes"], ptr["food"], ptr["role"], ptr["status"])
    before = env.counters()
    _lib.check(_lib.load().wab_rollout(env._h, ad.data_ptr(), T, ctypes.addressof(o), ptr["reward"], ptr["done"],
                                       ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "wab_rollout")
    torch.cuda.synchronize()
    assert env.counters()["rollout_launches"] - before["rollout_launches"] == 1, "not the one-launch path"
    for k, n in sizes.items():
        h = bufs[k].cpu().numpy()
        assert (h[:PAD] == 0xA5).all(), "%s: bytes before the slice written" % k
        assert (h[PAD + n:] == 0xA5).all(), "%s: bytes after the slice written" % k
    planes = bufs["planes"].cpu().numpy()[PAD:PAD + sizes["planes"]].reshape(T, B, 3, env.W, env.S)
    rew = bufs["reward"].cpu().numpy()[PAD:PAD + sizes["reward"]].view(np.float32).reshape(T, B)
    done = bufs["done"].cpu().numpy()[PAD:PAD + sizes["done"]].reshape(T, B)
    for t in range(T):
        op, of, orl, ost, orew, odone = orc.step(a[t])
        assert np.array_equal(planes[t], op), "planes differ at step %d" % t
        assert np.array_equal(rew[t], orew), "reward differs at step %d" % t
        assert np.array_equal(done[t], odone.astype(np.uint8)), "done differs at step %d" % t
