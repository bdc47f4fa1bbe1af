"""Inputs shared by the packed-feature tests (tests/test_packed_host.py on the CPU,
tests/test_gpu_packed_*.py): the nets whose shapes sit on the edges of the packed staging, binary
feature rows, and per-row inputs.  Every GPU comparison is a packed call against the float call on
the same binary rows and the same loaded weights, bit for bit, so the per-row inputs need no
property beyond being finite and of both signs.  Everything here runs on the CPU."""
from __future__ import annotations

import functools

import numpy as np

import policy_cases as pc
import policy_grad_cases as pgc

NET_REF = (449, 128, 150, 128, 5)
NETS = (
    (1, 1, 1, 1, 5),           # F = 1
    (17, 33, 33, 33, 5),       # F < 32, P = 4, 111 pad bits
    (256, 32, 32, 32, 5),      # no pad bits, F a multiple of 128: the ones column's tile is past the row
    NET_REF,                   # the reference net, <false> instance, KC = 160
    (449, 129, 150, 128, 6),   # the <true> instance
    (560, 130, 8, 8, 5),       # KC = 144: a chunk start in the middle of a dword, 4 chunks
)
ROWS = (0,) + tuple(pgc.ROWS)
PACK_F = (1, 31, 32, 33, 128, 449)
PACK_ROWS = (0, 1, 63, 64, 65, 257)
PITCH_F = (1, 31, 32, 33, 128, 129, 449, 512, 1000)
CLIP, VALUE_CLIP = 0.25, 0.25


def pitch(F):
    """P = 4 ceil(F / 128), the format's statement (include/wab.h)."""
    return 4 * -(-F // 128)


@functools.lru_cache(maxsize=None)
def binary_rows(F, n):
    """[n, F] float32 rows of 0.0 / 1.0: the oracle's real feature rows at F = 449, RandomState
    rows elsewhere."""
    if n == 0:
        return np.zeros((0, F), np.float32)
    if F == 449:
        x = np.ascontiguousarray(pc.ref_features(n), dtype=np.float32)
    else:
        x = np.random.RandomState(77 + n + 3 * F).randint(2, size=(n, F)).astype(np.float32)
    assert ((x == 0) | (x == 1)).all()
    return x


@functools.lru_cache(maxsize=None)
def case(net, n):
    """x (binary rows), a, adv, t, old_logp, old_value of n rows: advantages of both signs with
    zeros, old_logp around log(1 / A) so that some ratios clip, old values around the targets."""
    F, A = net[0], net[4]
    rng = np.random.RandomState(300 + n + 5 * F + net[1])
    adv = (rng.randint(-12, 13, size=n) / 4.0).astype(np.float32)
    adv[rng.rand(n) < 0.2] = 0.0
    return {"x": binary_rows(F, n), "a": rng.randint(A, size=n).astype(np.int8), "adv": adv,
            "t": (rng.randint(-8, 9, size=n) / 4.0).astype(np.float32),
            "old_logp": (np.log(1.0 / A) + rng.choice((0.0, 0.0625, -0.0625, 0.5, -0.5), size=n)).astype(np.float32),
            "old_value": (rng.randint(-8, 9, size=n) / 8.0).astype(np.float32)}


def gather_index(n, m):
    """An int32 [n] index into m rows with repeats, a reversed run and one entry outside [0, m)."""
    rng = np.random.RandomState(50 + n + m)
    r = rng.randint(m, size=n)
    r[10:40] = np.arange(m - 1, m - 31, -1)
    r[40:44] = 7
    r[n // 2] = m + 5
    return np.ascontiguousarray(r, dtype=np.int32)
