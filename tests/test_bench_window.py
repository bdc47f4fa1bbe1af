"""bench.py's line times exactly --steps steps (plan_window: replays of one captured graph and
the steps left over).  The windows timed beside it (--full: time_launches), which take no
--steps, have a floor: at least MIN_TIMED_LAUNCHES launches of the kernel in
the captured graph, replayed until at least MIN_TIMED_SECONDS are timed.  CPU-only: the sizing
functions, and the argument checks of the closed-loop C5 mode."""
import os
import subprocess
import sys

import bench

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_window_steps_floor():
    # the driver's `--steps 20` on 64-step launches: 32 launches, not one
    assert bench.window_steps(20, 64) == 32 * 64
    assert bench.window_steps(2000, 64) == 32 * 64        # 31 whole launches -> the floor
    assert bench.window_steps(5000, 64) == 78 * 64        # above the floor: whole launches
    assert bench.window_steps(20, 1) == 32                # per-step launches
    assert bench.window_steps(3000, 1) == 3000
    assert bench.window_steps(1, 64, min_launches=1) == 64  # at least one launch
    # the bench line's env-steps at B = 65536 are then >= 32 x 64 x 65536
    assert bench.window_steps(20, 64) * bench.window_replays(10.0) * 65536 >= 32 * 64 * 65536


def test_plan_window_times_exactly_the_steps_asked():
    for per in (1, 64, 128):
        for n in (1, 20, 63, 64, 65, 2000, 2048, 2049, 5000, 100000, 1234567):
            g, q, r, cap = bench.plan_window(n, per)
            assert g * q + r == n and 0 <= r < g <= cap and q >= 1
            assert cap % per == 0 and cap >= bench.MIN_TIMED_LAUNCHES * per  # whole launches of actions
            assert cap <= max(bench.GRAPH_STEPS, bench.MIN_TIMED_LAUNCHES * per)
    assert bench.plan_window(20, 64) == (20, 1, 0, 2048)       # one 20-step launch
    assert bench.plan_window(5000, 64) == (2048, 2, 904, 2048)  # 2 replays of 32 launches + 14.125 launches
    assert bench.plan_window(1000, 64, 256) == (256, 3, 232, 256)  # the closed-loop C5 graph: 4 segments


def test_dump_outputs_whole_and_sampled(tmp_path, monkeypatch):
    """--dump-outputs: float32 .npy per output, the env shards joined on the env axis; above the
    size limit the same seeded sample of envs in every array, the same from call to call."""
    import numpy as np
    import torch

    T, B = 3, 64
    planes = torch.arange(T * B * 5, dtype=torch.int64).reshape(T, B, 5).to(torch.uint8)
    rew = torch.arange(T * B, dtype=torch.float32).reshape(T, B)
    scal = torch.arange(3 * T * B, dtype=torch.int64).reshape(3, T, B).to(torch.uint8)
    halves = lambda x, ax: list(x.split(B // 2, dim=ax))  # noqa: E731
    outs = {"planes": (halves(planes, 1), 1), "reward": (halves(rew, 1), 1), "scalars": (halves(scal, 2), 2)}
    bench.dump_outputs(str(tmp_path / "a"), outs, B)
    got = {k: np.load(tmp_path / "a" / (k + ".npy")) for k in outs}
    assert all(v.dtype == np.float32 for v in got.values())
    assert np.array_equal(got["planes"], planes.numpy()) and np.array_equal(got["reward"], rew.numpy())
    assert np.array_equal(got["scalars"], scal.numpy())
    per_env = T * 5 + T + 3 * T
    monkeypatch.setattr(bench, "DUMP_BYTES", 4 * per_env * 20)  # room for 20 envs: 10 of each of 2 ranks
    for d in ("b", "c"):
        bench.dump_outputs(str(tmp_path / d), outs, B, rank=1, world=2)
    b = {k: np.load(tmp_path / "b" / (k + "_rank1.npy")) for k in outs}
    assert 2 * sum(v.nbytes for v in b.values()) <= bench.DUMP_BYTES
    assert b["planes"].shape == (T, 10, 5) and b["reward"].shape == (T, 10) and b["scalars"].shape == (3, T, 10)
    ids = b["reward"][0].astype(int)  # reward[0, e] == e: the sampled env ids
    assert list(ids) == sorted(set(ids)) and ids.min() < B // 2 <= ids.max()  # both shards
    assert np.array_equal(b["planes"], planes.numpy()[:, ids]) and np.array_equal(b["scalars"], scal.numpy()[:, :, ids])
    for k in outs:
        assert np.array_equal(b[k], np.load(tmp_path / "c" / (k + "_rank1.npy")))


def test_window_replays_reach_min_seconds():
    assert bench.MIN_TIMED_SECONDS >= 0.2 and bench.MIN_TIMED_LAUNCHES >= 32
    for g in (0.0004, 0.013, 0.2, 0.9):
        r = bench.window_replays(g)
        assert r >= 1 and r * g >= min(bench.MIN_TIMED_SECONDS, g * r)
        assert r * g >= bench.MIN_TIMED_SECONDS or r == 1 and g >= bench.MIN_TIMED_SECONDS
        assert (r - 1) * g < bench.MIN_TIMED_SECONDS  # no more replays than needed
    assert bench.window_replays(0.0) >= 1 and bench.window_replays(1e-9) <= 10000


def _run(*args):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    return subprocess.run([sys.executable, os.path.join(REPO, "bench.py")] + list(args),
                          capture_output=True, text=True, timeout=600, env=env)


def test_policy_mode_argument_checks():
    r = _run("--policy", "mlp", "--no-cpu")  # the default config has no features
    assert r.returncode != 0 and "--config c5" in r.stderr
    r = _run("--config", "c5", "--policy", "mlp", "--rollout", "64", "--no-cpu")
    assert r.returncode != 0 and "one launch per step" in r.stderr


def test_bench_line_is_strict_json():
    # a surface the run did not measure (NaN) is null in the printed line, never a bare NaN
    import json

    line = {"a": float("nan"), "b": [1.0, float("inf")], "c": {"d": float("-inf"), "e": 2}, "f": (3.0,)}
    out = json.loads(json.dumps(bench.finite(line), allow_nan=False))
    assert out == {"a": None, "b": [1.0, None], "c": {"d": None, "e": 2}, "f": [3.0]}
