"""`bench.py --gpus 1 --steps K --warmup W` as a plain run: it times exactly K steps (whole
64-step launches and one shorter one), reports ms_per_step for them, measures nothing beside
the line (that is `--full`), and `--dump-outputs DIR` writes the last launch's outputs as float32
.npy files that a second run with the same arguments reproduces entry for entry."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, K = 1024, 70  # one whole 64-step launch of each shard and a 6-step one


def _bench(out):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", str(K),
                        "--warmup", "3", "--batch", str(B), "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


def test_plain_run_times_the_steps_asked_and_dumps_reproducible_outputs(tmp_path):
    lines = [_bench(tmp_path / d) for d in ("a", "b")]
    for line in lines:
        assert line["steps"] == K and line["steps_requested"] == K
        w = line["timed_window"]
        assert w["env_steps"] == K * B and w["launches"] == 2
        assert line["unit"] == "env-steps/s" and line["higher_is_better"] is True and line["dtype"] == "u8"
        assert line["ms_per_step"] > 0
        # the line rounds stream_ms to 1e-3 ms and ms_per_step to 1e-5 ms
        assert abs(line["ms_per_step"] * K - w["stream_ms"]) <= 0.0005 + K * 0.000005 + 1e-9
        assert abs(line["value"] / (B * K / (w["stream_ms"] * 1e-3)) - 1) <= 0.0005 / w["stream_ms"] + 1e-6
        # nothing measured beside the line
        assert "configs" not in line and "cpu_baseline" not in line
        assert line["rollout"]["per_step_launch"]["us_per_step"] is None
    tt = K % 64
    shapes = {"planes": (tt, B, 3, 11, 11), "scalars": (3, tt, B), "reward": (tt, B), "done": (tt, B)}
    assert sorted(os.listdir(tmp_path / "a")) == sorted(n + ".npy" for n in shapes)
    for name, shape in shapes.items():
        a, b = np.load(tmp_path / "a" / (name + ".npy")), np.load(tmp_path / "b" / (name + ".npy"))
        assert a.dtype == np.float32 and a.shape == shape
        assert np.array_equal(a, b), name
    planes = np.load(tmp_path / "a" / "planes.npy")
    assert set(np.unique(planes)) == {0.0, 1.0}  # rendered observations, not an untouched buffer
