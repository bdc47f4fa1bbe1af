"""EnvSnapshot — what `BatchedWolvesAndBushesEnv.snapshot()` returns and `.restore()` takes.

A snapshot of envs with global ids [env_id_first, env_id_first + count) holds

  * the fields of `wab_snapshot_info` (include/wab.h): magic, version, config_hash, seed,
    env_id_first, count, record_bytes;
  * `records` u8 [count, record_bytes]: the device state of each env (wab_snapshot_save);
  * the same envs' rows of the gym surface at that moment: obs planes [count, 3, W, S] and
    scalars [3, count], reward [count], done [count], the terminal obs (or None) and whether
    the planes were valid.  The current observation is taken before the step's eat and spawn,
    so it cannot be derived from the records; it is copied.

The tensors live where the env lives; `.cpu()` / `.to(device)` move a snapshot, `.save(path)`
writes it as plain numpy arrays (`np.savez`, nothing pickled) and `EnvSnapshot.load(path)` reads
one back onto the host.
"""
from __future__ import annotations

import zipfile

import numpy as np

from . import _lib

_INFO_FIELDS = ("magic", "version", "config_hash", "seed", "env_id_first", "count", "record_bytes")
_TENSORS = ("records", "planes", "scalars", "reward", "done", "term_planes", "term_scalars")
_FILE_FORMAT = 1


class EnvSnapshot:
    def __init__(self, magic, version, config_hash, seed, env_id_first, count, record_bytes, records,
                 planes, scalars, reward, done, W, H, S, planes_valid=True, term_planes=None,
                 term_scalars=None):
        self.magic, self.version = int(magic), int(version)
        self.config_hash, self.seed = int(config_hash), int(seed)
        self.env_id_first, self.count = int(env_id_first), int(count)
        self.record_bytes = int(record_bytes)
        self.W, self.H, self.S = int(W), int(H), int(S)
        self.planes_valid = bool(planes_valid)
        self.records, self.planes, self.scalars = records, planes, scalars
        self.reward, self.done = reward, done
        self.term_planes, self.term_scalars = term_planes, term_scalars
        self._validate()

    def _validate(self):
        if self.magic != _lib.SNAPSHOT_MAGIC:
            raise ValueError("not an env snapshot: magic 0x%08x, expected 0x%08x ('WABS')"
                             % (self.magic, _lib.SNAPSHOT_MAGIC))
        if self.version != _lib.SNAPSHOT_VERSION:
            raise ValueError("env snapshot version %d, this package reads version %d"
                             % (self.version, _lib.SNAPSHOT_VERSION))
        n, W, S = self.count, self.W, self.S
        if n < 0 or self.record_bytes <= 0 or self.record_bytes % 16 or not 0 < self.H <= S or W <= 0:
            raise ValueError("env snapshot with impossible sizes")
        want = {"records": (n, self.record_bytes), "planes": (n, 3, W, S), "scalars": (3, n),
                "reward": (n,), "done": (n,), "term_planes": (n, 3, W, S), "term_scalars": (3, n)}
        if (self.term_planes is None) != (self.term_scalars is None):
            raise ValueError("env snapshot with half a terminal observation")
        for name in _TENSORS:
            x = getattr(self, name)
            if x is None and name.startswith("term_"):
                continue
            if x is None or tuple(x.shape) != want[name]:
                raise ValueError("env snapshot: %s has shape %s, expected %s"
                                 % (name, None if x is None else tuple(x.shape), want[name]))

    def info(self):
        """The `wab_snapshot_info` of these records."""
        return _lib.WabSnapshotInfo(*(getattr(self, f) for f in _INFO_FIELDS))

    @property
    def device(self):
        return self.records.device

    def to(self, device):
        """The same snapshot with its tensors on `device`."""
        kw = {f: getattr(self, f) for f in _INFO_FIELDS}
        for name in _TENSORS:
            x = getattr(self, name)
            kw[name] = None if x is None else x.to(device)
        return EnvSnapshot(W=self.W, H=self.H, S=self.S, planes_valid=self.planes_valid, **kw)

    def cpu(self):
        return self.to("cpu")

    def save(self, path):
        """Write the snapshot to `path` as numpy arrays (np.savez: a zip of .npy members)."""
        arrays = {f: np.array(getattr(self, f), dtype=np.uint64 if f in ("config_hash", "seed") else np.int64)
                  for f in _INFO_FIELDS}
        arrays["file_format"] = np.array(_FILE_FORMAT, np.int64)
        arrays["geometry"] = np.array([self.W, self.H, self.S, int(self.planes_valid)], np.int64)
        for name in _TENSORS:
            x = getattr(self, name)
            if x is not None:
                arrays[name] = x.detach().cpu().numpy()
        with open(path, "wb") as f:
            np.savez(f, **arrays)

    @classmethod
    def load(cls, path):
        """Read a snapshot written by save() onto the host.  ValueError for a file that is not
        one: truncated, another magic or version, arrays of the wrong shape or type."""
        import torch

        dtypes = {"records": np.uint8, "planes": np.uint8, "scalars": np.uint8, "reward": np.float32,
                  "done": np.uint8, "term_planes": np.uint8, "term_scalars": np.uint8}
        try:
            with np.load(path, allow_pickle=False) as z:
                names = set(z.files)
                if int(z["file_format"]) != _FILE_FORMAT:
                    raise ValueError("env snapshot file format %d, expected %d" % (int(z["file_format"]), _FILE_FORMAT))
                kw = {f: int(z[f]) for f in _INFO_FIELDS}
                W, H, S, valid = (int(v) for v in z["geometry"])
                for name in _TENSORS:
                    if name not in names:
                        kw[name] = None
                        continue
                    a = z[name]
                    if a.dtype != dtypes[name]:
                        raise ValueError("env snapshot: %s has dtype %s" % (name, a.dtype))
                    kw[name] = torch.from_numpy(np.ascontiguousarray(a))
        except (zipfile.BadZipFile, KeyError, EOFError, OSError, TypeError) as e:
            if isinstance(e, FileNotFoundError):
                raise
            raise ValueError("%s is not an env snapshot file: %s" % (path, e)) from e
        return cls(W=W, H=H, S=S, planes_valid=bool(valid), **kw)


__all__ = ["EnvSnapshot"]
