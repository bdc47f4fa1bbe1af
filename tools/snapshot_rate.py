"""Time wab_snapshot_save and wab_snapshot_restore against a device-to-device copy of the same bytes.

    python tools/snapshot_rate.py [--envs 65536] [--reps 50] [--batches 7] [--config default|wide31]

One handle of B envs (reset, 30 steps, so the state is a played one), then, alternating,
batches of `reps` back-to-back calls of
    save     wab_snapshot_save of all B envs into one [B, R] buffer,
    restore  wab_snapshot_restore of all of them from it,
    copy     hipMemcpyAsync device-to-device of B * R bytes (the floor: the least traffic a
             snapshot can be, and not the code under test),
each batch between two hipEvents on the stream, after a warm-up batch of each.  Prints the
per-call time of every batch (batch time / reps), the median over batches, and the ratios to
the copy, and one JSON line.  Back-to-back calls on 30 MB leave the data in the 256 MB Infinity
Cache, for the copy as for the kernels; the comparison is like for like, the absolute
bandwidths are not HBM bandwidths.
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def loaded_hip_runtime():
    """The HIP runtime this process already has (torch's), for hipMemcpyAsync."""
    with open("/proc/self/maps") as f:
        for line in f:
            path = line.split()[-1]
            if "libamdhip64.so" in os.path.basename(path):
                return ctypes.CDLL(path)
    raise RuntimeError("no libamdhip64.so in this process")


def main():
    import numpy as np
    import torch

    from wab_gym_amd import _lib
    from wab_gym_amd.env import BatchedWolvesAndBushesEnv

    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--batches", type=int, default=7)
    ap.add_argument("--config", default="default", choices=["default", "wide31"])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("snapshot_rate needs a GPU: a time measured anywhere else says nothing")

    B = args.envs
    if args.config == "wide31":
        env = BatchedWolvesAndBushesEnv({"width": 31, "height": 31}, num_envs=B, device="cuda:0", plane_stride=32)
    else:
        env = BatchedWolvesAndBushesEnv(num_envs=B, device="cuda:0")
    env.reset()
    rng = np.random.RandomState(0)
    for _ in range(30):
        env.step(torch.as_tensor(rng.randint(env.n_actions, size=B)))
    L = _lib.load()
    R = int(L.wab_snapshot_bytes(ctypes.addressof(env.cfg)))
    records = torch.empty((B, R), dtype=torch.uint8, device="cuda:0")
    other = torch.empty_like(records)
    info = _lib.WabSnapshotInfo()
    stream = env._stream()
    hip = loaded_hip_runtime()
    hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    D2D = 3  # hipMemcpyDeviceToDevice

    def save():
        _lib.check(L.wab_snapshot_save(env._h, 0, B, records.data_ptr(), ctypes.addressof(info), stream))

    def restore():
        _lib.check(L.wab_snapshot_restore(env._h, ctypes.addressof(info), records.data_ptr(), None, stream))

    def copy():
        if hip.hipMemcpyAsync(other.data_ptr(), records.data_ptr(), B * R, D2D, stream) != 0:
            raise RuntimeError("hipMemcpyAsync failed")

    calls = {"save": save, "restore": restore, "copy": copy}

    def batch(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.reps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / args.reps  # us per call

    state_before = {k: v.copy() for k, v in env.state().items()}
    for fn in calls.values():  # warm-up: code objects loaded, buffers touched
        batch(fn)
    times = {k: [] for k in calls}
    for _ in range(args.batches):
        for k, fn in calls.items():
            times[k].append(batch(fn))
    # the timed restores put back the state the saves took: nothing may have changed
    after = env.state()
    assert all(np.array_equal(after[k].view(np.uint8), v.view(np.uint8)) for k, v in state_before.items())
    assert torch.equal(other, records)

    med = {k: statistics.median(v) for k, v in times.items()}
    nbytes = B * R
    for k, v in times.items():
        print("%-8s us per call, by batch: %s   median %.1f us  (%.0f GB/s read + written)"
              % (k, " ".join("%.1f" % x for x in v), med[k], 2 * nbytes / med[k] / 1e3))
    print(json.dumps({"config": args.config, "envs": B, "record_bytes": R, "bytes": nbytes, "reps": args.reps,
                      "batches": args.batches, "kernel": env.step_kernel,
                      "save_us": round(med["save"], 2), "restore_us": round(med["restore"], 2),
                      "copy_us": round(med["copy"], 2),
                      "save_over_copy": round(med["save"] / med["copy"], 2),
                      "restore_over_copy": round(med["restore"] / med["copy"], 2)}))


if __name__ == "__main__":
    main()
