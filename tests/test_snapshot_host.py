"""The host side of snapshots, no GPU: wab_snapshot_bytes and wab_snapshot_hash (host-only entry
points of include/wab.h), the ctypes mirror of wab_snapshot_info, and EnvSnapshot files."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from wab_gym_amd import _lib
from wab_gym_amd.options import make_config

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "wab.h")


def lib():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail("libwab_hip.so not built (run __graft_entry__.build())")
    return _lib.load()


def record_bytes(width, height, wolf_slots, eaten_capacity):
    """The record format: hdr 16, food 8, wolf tiles, log entries (u32 tile + u8 berries left),
    up to a dword; the bitmap dwords; up to 16 bytes."""
    n = 16 + 8 + 4 * wolf_slots + 5 * eaten_capacity
    n = (n + 3) // 4 * 4 + 4 * ((width * height + 31) // 32)
    return (n + 15) // 16 * 16


def snapshot_bytes(options=None, **kw):
    cfg, keep = make_config(options, **kw)
    return lib().wab_snapshot_bytes(ctypes.addressof(cfg))


def snapshot_hash(options=None, table=True, **kw):
    cfg, keep = make_config(options, **kw)
    if not table:
        cfg.bush_thresholds = None
    return lib().wab_snapshot_hash(ctypes.addressof(cfg))


def test_snapshot_bytes():
    assert record_bytes(11, 11, 8, 80) == 480
    assert snapshot_bytes() == 480
    assert snapshot_bytes(wolf_slots=32, eaten_capacity=12) == record_bytes(11, 11, 32, 12) == 240
    assert snapshot_bytes({"width": 31, "height": 31}) == record_bytes(31, 31, 8, 80) == 592
    # eaten_capacity defaults to max_turns; a capacity that is no multiple of 4 pads its bytes
    assert snapshot_bytes({"max_turns": 61}) == record_bytes(11, 11, 8, 61)
    cfg, keep = make_config()
    cfg.width = 12
    assert lib().wab_snapshot_bytes(ctypes.addressof(cfg)) < 0
    assert b"odd" in lib().wab_last_error()
    assert lib().wab_snapshot_bytes(None) < 0


def test_snapshot_hash():
    base = snapshot_hash()
    assert base != 0 and base == snapshot_hash()
    assert snapshot_hash(plane_stride=16) == base
    assert snapshot_hash(table=False) == base  # NULL: the table wab_bush_thresholds computes
    assert snapshot_hash(wolf_slots=8) == base and snapshot_hash(eaten_capacity=80) == base  # the resolved values
    changed = {
        "chance_wolf_on_square": snapshot_hash({"chance_wolf_on_square": 0.002}),
        "max_turns": snapshot_hash({"max_turns": 81}, eaten_capacity=80),
        "width": snapshot_hash({"width": 13}),
        "wolf_slots": snapshot_hash(wolf_slots=16),
        "eaten_capacity": snapshot_hash(eaten_capacity=81),
        "reward_for_eating": snapshot_hash({"reward_for_eating": 0.2}),
        "autoreset": snapshot_hash(autoreset=False),
    }
    for what, h in changed.items():
        assert h != base and h != 0, what
    assert len(set(changed.values())) == len(changed)


def test_snapshot_info_layout_matches_c(tmp_path):
    fields = [f for f, _ in _lib.WabSnapshotInfo._fields_]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "%s"' % HEADER, "int main(void){",
             'printf("%zu\\n", sizeof(wab_snapshot_info));']
    lines += ['printf("%%zu\\n", offsetof(wab_snapshot_info, %s));' % f for f in fields]
    lines += ['printf("%u %u\\n", WAB_SNAPSHOT_MAGIC, WAB_SNAPSHOT_VERSION);', "return 0;}"]
    prog = tmp_path / "layout.c"
    prog.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-o", str(exe), str(prog)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    assert int(out[0]) == ctypes.sizeof(_lib.WabSnapshotInfo)
    for i, f in enumerate(fields):
        assert int(out[1 + i]) == getattr(_lib.WabSnapshotInfo, f).offset, f
    assert int(out[-2]) == _lib.SNAPSHOT_MAGIC and int(out[-1]) == _lib.SNAPSHOT_VERSION
    assert _lib.SNAPSHOT_MAGIC.to_bytes(4, "little") == b"WABS"


def cpu_snapshot(n=5, R=480, W=11, H=11, S=16, terminal=True):
    import torch

    from wab_gym_amd import EnvSnapshot

    g = torch.Generator().manual_seed(3)

    def u8(*shape):
        return torch.randint(0, 256, shape, dtype=torch.uint8, generator=g)

    return EnvSnapshot(_lib.SNAPSHOT_MAGIC, _lib.SNAPSHOT_VERSION, 2**64 - 5, 2**63 + 7, 2**40 + 3, n, R,
                       u8(n, R), u8(n, 3, W, S), u8(3, n), torch.rand(n, generator=g), u8(n), W, H, S,
                       planes_valid=False, term_planes=u8(n, 3, W, S) if terminal else None,
                       term_scalars=u8(3, n) if terminal else None)


SCALARS = ("magic", "version", "config_hash", "seed", "env_id_first", "count", "record_bytes", "W", "H", "S",
           "planes_valid")
TENSORS = ("records", "planes", "scalars", "reward", "done", "term_planes", "term_scalars")


@pytest.mark.parametrize("terminal", [True, False])
def test_env_snapshot_file_round_trip(tmp_path, terminal):
    import torch

    from wab_gym_amd import EnvSnapshot

    snap = cpu_snapshot(terminal=terminal)
    path = tmp_path / "snap.bin"  # (no .npz suffix is added)
    snap.save(path)
    assert os.path.exists(path)
    with np.load(path, allow_pickle=False) as z:  # plain arrays only
        assert all(z[k].dtype != object for k in z.files)
    back = EnvSnapshot.load(path)
    for f in SCALARS:
        assert getattr(back, f) == getattr(snap, f), f
    for f in TENSORS:
        a, b = getattr(snap, f), getattr(back, f)
        if a is None:
            assert b is None, f
        else:
            assert a.dtype == b.dtype and torch.equal(a, b), f
    info = back.info()
    assert (info.magic, info.config_hash, info.seed, info.env_id_first, info.count, info.record_bytes) == \
        (_lib.SNAPSHOT_MAGIC, 2**64 - 5, 2**63 + 7, 2**40 + 3, 5, 480)


def test_env_snapshot_load_refuses_what_is_not_one(tmp_path):
    from wab_gym_amd import EnvSnapshot

    snap = cpu_snapshot()
    good = tmp_path / "good.npz"
    snap.save(good)
    raw = good.read_bytes()
    cut = tmp_path / "cut.npz"
    cut.write_bytes(raw[:len(raw) // 2])
    with pytest.raises(ValueError):
        EnvSnapshot.load(cut)
    with np.load(good, allow_pickle=False) as z:
        arrays = {k: z[k] for k in z.files}
    for key, value in (("magic", np.array(_lib.SNAPSHOT_MAGIC + 1, np.int64)), ("version", np.array(2, np.int64)),
                       ("records", arrays["records"][:, :-16]), ("scalars", arrays["scalars"][:2]),
                       ("reward", arrays["reward"].astype(np.float64))):
        bad = tmp_path / ("bad_%s.npz" % key)
        with open(bad, "wb") as f:
            np.savez(f, **dict(arrays, **{key: value}))
        with pytest.raises(ValueError):
            EnvSnapshot.load(bad)
    missing = tmp_path / "missing.npz"
    with open(missing, "wb") as f:
        np.savez(f, **{k: v for k, v in arrays.items() if k != "planes"})
    with pytest.raises(ValueError):
        EnvSnapshot.load(missing)
    assert EnvSnapshot.load(good).count == snap.count
