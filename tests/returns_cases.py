"""Inputs shared by the returns tests (tests/test_featurizer_oracle.py on the CPU,
tests/test_gpu_returns.py on the device): the option sets that select each reward-table size NE
of wab_returns_kernel<VEC, NE> and the [T, B] reward / done segments
built to make a wrong row access, byte select or chunk edge change the answer.  Everything here
runs on the CPU (numpy)."""
from __future__ import annotations

import numpy as np

REWARD_KEYS = ("reward_for_eating", "reward_per_turn", "reward_for_finishing", "reward_for_starving",
               "reward_for_being_killed")

# (name, eating / per turn / finishing / starving / being killed or None for the defaults, the
# NE the kernel is launched with).  NE counts the table entries whose float32 is not their
# double; 5 to 7 are padded to 8.  tests/test_featurizer_oracle.py restates the table rule and
# confirms every count.
OPTION_SETS = (
    ("exact", (0.5, 0, 1, -1, -1), 0),
    ("eat", (0.1, 0, 0, 0, 0), 1),
    ("eat_finish", (0.1, 0, 1, 0, 0), 2),
    ("defaults", None, 3),
    ("killed2", (0.1, 0, 1, -1, -2), 4),
    # 0.01, 0.11, 1.3, 1.4, -0.9, -1.9 are inexact, -1 and -2 exact: 6, padded to 8
    ("six", (0.1, 0.01, 1.3, -1, -2), 8),
    ("eight", (0.1, 0.01, 1.3, -0.7, -1.2), 8),
)
INEXACT = {"exact": 0, "eat": 1, "eat_finish": 2, "defaults": 3, "killed2": 4, "six": 6, "eight": 8}


def options_of(name):
    """The game options (a dict to pass to the env; {} for the defaults) of an OPTION_SETS name."""
    vals = {n: v for n, v, _ in OPTION_SETS}[name]
    return {} if vals is None else dict(zip(REWARD_KEYS, vals))


def launched_ne(n_inexact):
    return n_inexact if n_inexact <= 4 else 8


DONE_BYTES = np.array([1, 0x80, 0xFF], np.uint8)


def make_case(T, B, values, seed=0, bootstrap=True):
    """(reward [T, B] f32, done [T, B] u8, bootstrap [B] f32 or None).

    Rewards: `values`, the option set's eight step rewards (step_reward_values of
    tests/test_featurizer_oracle.py), as float32 (most), arbitrary standard_normal
    floats (which must pass through as float32) and -0.0.  done: zero for nine in ten entries,
    else one of 1, 0x80, 0xFF, the byte chosen by (env + step) % 3, so two neighbouring envs
    never hold the same nonzero byte at a step and most neighbours differ: a wrong byte select,
    a swapped lane or a test of one bit changes which env restarts.  Column 0 is never done
    and column 1 always; columns 2..5 are done at t = 0, T - 1, 31 and 32; the same six mirrored
    at the last six columns.  B = 1 takes the four forced steps in its one column."""
    rng = np.random.RandomState(1000 + 31 * seed + T)
    vals = np.concatenate([np.asarray(values, np.float64).astype(np.float32),
                           np.array([-0.0], np.float32)])
    pick = rng.randint(0, 12, size=(T, B)).astype(np.int8)
    reward = vals[np.minimum(pick, 8)]
    loose = pick > 8
    reward[loose] = rng.standard_normal(int(loose.sum())).astype(np.float32)
    phase = ((np.arange(T, dtype=np.uint8) % 3)[:, None] + (np.arange(B) % 3).astype(np.uint8)[None, :]) % 3
    done = np.where(rng.randint(0, 10, size=(T, B), dtype=np.uint8) == 0, DONE_BYTES[phase], 0).astype(np.uint8)
    forced = [t for t in (0, T - 1, 31, 32) if t < T]
    if B == 1:
        done[forced, 0] = 0x80
    else:
        assert B >= 12
        for cols in (range(6), range(B - 1, B - 7, -1)):
            done[:, cols[0]] = 0
            done[:, cols[1]] = DONE_BYTES[phase[:, cols[1]]]
            for c, t in zip(cols[2:], (0, T - 1, 31, 32)):
                if t < T:
                    done[t, c] = DONE_BYTES[phase[t, c]]
    boot = rng.standard_normal(B).astype(np.float32) if bootstrap else None
    return reward, done, boot
