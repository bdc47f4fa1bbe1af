"""The advantage functions on the host: the header declares them at ABI 11, the CPU paths of
wrappers.gae and wrappers.whitened equal the numpy references of tests/gae_cases.py bit for bit,
and three identities of the contract itself pin the references and the test data."""
import os
import re

import numpy as np
import pytest
import torch

import gae_cases as gc
import returns_cases as rc
from wab_gym_amd import _lib
from wab_gym_amd.wrappers import gae, whitened

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "wab.h")
NEW = ("wab_gae", "wab_whiten_workspace", "wab_whiten", "wab_debug_gae_plan")


class OptionsOnly:
    """What gae(env=...) reads of an env on the CPU path: its options."""

    def __init__(self, opts):
        from wab_gym_amd.options import default_game_options

        self.game_options = dict(default_game_options)
        self.game_options.update(opts)
        self.device = torch.device("cpu")


def test_header_is_abi_11_and_declares_the_new_functions():
    src = open(HEADER).read()
    version = int(re.search(r"#define\s+WAB_ABI_VERSION\s+(\d+)", src).group(1))
    assert version == _lib.ABI_VERSION and version >= 11
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in _lib.EXPORTED
    # the contract is written down in the header, the kernel source and DESIGN.md
    for path in (HEADER, os.path.join(REPO, "wab_gym_amd", "csrc", "wab_advantage.hip"),
                 os.path.join(REPO, "DESIGN.md")):
        text = open(path).read()
        assert "delta = (r + (d ? 0.0 : gamma * vnext)) - v" in text, path
        assert "A     = delta + (d ? 0.0 : gl * A)" in text, path


def test_gae_plan_thresholds_and_host_side_refusals():
    """wab_debug_gae_plan without a handle (host only: the pointers are never read): VEC is 2 when
    B is even, B / 2 >= 65536, reward, value and the outputs are 8-byte aligned and done 2-byte
    aligned, else 1; NE is 0 without a reward table.  The refusals wab_gae and wab_whiten make
    before they touch the device need none either."""
    import ctypes

    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libwab_hip.so not built")
    L = _lib.load()
    base = dict(reward=1 << 20, done=2 << 20, value=3 << 20, advantage=4 << 20, target=5 << 20)

    def vec(B, **at):
        p = dict(base, **at)
        out = (ctypes.c_int32 * 2)(-1, -1)
        assert L.wab_debug_gae_plan(None, p["reward"], p["done"], p["value"], p["advantage"], p["target"], B, out) == 0
        assert out[1] == 0
        return out[0]

    assert [vec(B) for B in (1, 65536, 131070, 131071, 131072, 131073, 131074, 262144, 1 << 33)] == \
        [1, 1, 1, 1, 2, 1, 2, 2, 2]
    B = 131072
    for name in ("reward", "value", "advantage", "target"):
        assert [vec(B, **{name: base[name] + o}) for o in (4, 8, 12, 16)] == [1, 2, 1, 2], name
    assert [vec(B, done=base["done"] + o) for o in (1, 2, 3, 4)] == [1, 2, 1, 2]
    assert vec(B, advantage=None) == 2 and vec(B, target=None) == 2 and vec(B, target=None, advantage=base["advantage"] + 4) == 1
    out = (ctypes.c_int32 * 2)()
    assert L.wab_debug_gae_plan(None, 4096, 8192, 12288, None, None, B, out) == -1
    assert L.wab_debug_gae_plan(None, None, 8192, 12288, 16384, None, B, out) == -1
    assert L.wab_debug_gae_plan(None, 4096, 8192, 12288, 16384, None, -1, out) == -1
    assert L.wab_debug_gae_plan(None, 4096, 8192, 12288, 16384, None, B, None) == -1

    def call(adv, tgt, T=4, B=16, value=base["value"]):
        return L.wab_gae(None, base["reward"], base["done"], value, None, T, B, 0.99, 0.95, adv, tgt, None)

    assert call(None, None) == -1
    assert call(base["advantage"], None, T=-1) == -1 and call(base["advantage"], None, B=-1) == -1
    assert call(base["advantage"], None, value=None) == -1
    assert call(base["value"] + 4 * 16, None) == -1 and b"overlaps an input" in L.wab_last_error()   # one row into value
    assert call(base["reward"] - 4, None) == -1                                                       # one float into reward
    assert call(base["advantage"], base["advantage"] + 4 * 4 * 16 - 4) == -1 and b"overlap" in L.wab_last_error()
    assert call(base["advantage"], None, T=0) == 0 and call(base["advantage"], None, B=0) == 0       # nothing launched
    size = L.wab_whiten_workspace(1 << 20)
    assert size > 0 and size % 8 == 0 and L.wab_whiten_workspace(0) == size == L.wab_whiten_workspace(1 << 40)
    assert L.wab_whiten_workspace(-1) == -1 and L.wab_whiten_workspace((1 << 40) + 1) == -1
    assert L.wab_whiten(4096, -1, 1e-7, 4096, 8192, None) == -1
    assert L.wab_whiten(4096, 8, 1e-7, 4096, None, None) == -1 and L.wab_whiten(4096, 8, 1e-7, 4096, 8196, None) == -1
    assert L.wab_whiten(4096, 8, 1e-7, 4096 + 16, 8192, None) == -1 and b"overlap" in L.wab_last_error()
    assert L.wab_whiten(None, 0, 1e-7, None, None, None) == 0


@pytest.mark.parametrize("name", ["defaults", "exact", "eight"])
@pytest.mark.parametrize("T,B", [(1, 1), (33, 65), (65, 200)])
def test_cpu_gae_is_the_contract(T, B, name):
    if B == 1:
        B = 12 if T > 1 else 1
    reward, done, value, last, opts = gc.make_gae_case(T, B, name)
    to = torch.from_numpy
    for table in (True, False):
        for lv in (last, None):
            want = gc.gae_reference(gc.exact_rewards(reward, opts, table), done, value, lv, 0.99, 0.95)
            got = gae(to(reward), to(done), to(value), None if lv is None else to(lv), 0.99, 0.95,
                      env=OptionsOnly(opts) if table else None)
            assert gc.same_bits(got[0].numpy(), want[0]) and gc.same_bits(got[1].numpy(), want[1])
    adv = torch.empty(T, B)
    tgt = torch.empty(T, B)
    got = gae(to(reward), to(done != 0), to(value), to(last), 0.99, 0.95, advantage=adv, target=tgt)
    assert got[0] is adv and got[1] is tgt
    want = gc.gae_reference(gc.exact_rewards(reward, opts, False), done, value, last, 0.99, 0.95)
    assert gc.same_bits(adv.numpy(), want[0]) and gc.same_bits(tgt.numpy(), want[1])


def test_cpu_gae_refuses_bad_shapes():
    r = torch.zeros(4, 3)
    with pytest.raises(ValueError):
        gae(r, torch.zeros(4, 2, dtype=torch.uint8), r)
    with pytest.raises(ValueError):
        gae(r, torch.zeros(4, 3, dtype=torch.uint8), r, last_value=torch.zeros(4))
    with pytest.raises(ValueError):
        gae(r, torch.zeros(4, 3, dtype=torch.uint8), r, advantage=torch.zeros(4, 3, dtype=torch.float64))


def test_exact_rewards_change_the_advantages():
    """The table matters: with the default options about one advantage in ten differs in its
    float32 between the exact and the float32 rewards."""
    reward, done, value, last, opts = gc.make_gae_case(65, 200)
    a = gc.gae_reference(gc.exact_rewards(reward, opts, True), done, value, last, 0.99, 0.95)[0]
    b = gc.gae_reference(gc.exact_rewards(reward, opts, False), done, value, last, 0.99, 0.95)[0]
    assert (gc.bits(a) != gc.bits(b)).mean() > 0.01


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 4097, 64 * 1000 + 1])
def test_cpu_whitened_is_the_reference(n):
    x = gc.make_whiten_input(n)
    want = gc.whiten_reference(x)
    got = whitened(torch.from_numpy(x))
    if n == 1:
        assert np.isnan(want).all() and torch.isnan(got).all()
        return
    assert gc.same_bits(got.numpy(), want)
    y = torch.from_numpy(x.copy())
    assert whitened(y, out=y) is y and gc.same_bits(y.numpy(), want)
    assert gc.same_bits(whitened(torch.from_numpy(x), eps=0.5).numpy(), gc.whiten_reference(x, 0.5))
    shaped = torch.from_numpy(x[: n - n % 2].reshape(2, -1).copy()) if n > 2 else None
    if shaped is not None:
        assert whitened(shaped).shape == shaped.shape


def test_cpu_whitened_refuses_other_dtypes_and_layouts():
    with pytest.raises(ValueError):
        whitened(torch.zeros(8, dtype=torch.float64))
    with pytest.raises(ValueError):
        whitened(torch.zeros(8, 8).t())
    with pytest.raises(ValueError):
        whitened(torch.zeros(8), out=torch.zeros(9))


# ------------------------------------------------------------------ identities of the contract
IDENTITY_CASES = [(129, 1000, 4.0, 0.99), (129, 1000, 1.0e4, 0.99), (65, 1000, 4.0, 1.0)]


@pytest.mark.parametrize("T,B,scale,gamma", IDENTITY_CASES)
def test_lambda_zero_is_the_one_step_residual(T, B, scale, gamma):
    reward, done, value, last, opts = gc.make_gae_case(T, B, scale=scale)
    r64 = gc.exact_rewards(reward, opts)
    adv, _ = gc.gae_reference(r64, done, value, last, gamma, 0.0)
    v64 = value.astype(np.float64)
    vnext = np.concatenate([v64[1:], last.astype(np.float64)[None]])
    with np.errstate(all="ignore"):
        delta = (r64 + np.where(done != 0, 0.0, gamma * vnext)) - v64
    # (the contract's A = delta + (0.0 or 0 * A): a -0.0 residual leaves as +0.0, and in the column
    # of infinities 0 * A is NaN until the next done)
    want = (delta + 0.0).astype(np.float32)
    cols = gc.finite_columns(value, last)
    assert gc.same_bits(adv[:, cols], want[:, cols])
    assert np.isnan(adv[:, ~cols]).any()


@pytest.mark.parametrize("T,B,scale,gamma", IDENTITY_CASES)
def test_gamma_zero_is_reward_minus_value(T, B, scale, gamma):
    reward, done, value, last, opts = gc.make_gae_case(T, B, scale=scale)
    r64 = gc.exact_rewards(reward, opts)
    adv, _ = gc.gae_reference(r64, done, value, last, 0.0, 0.95)
    cols = gc.finite_columns(value, last)  # (0 * inf is NaN in the contract, not r - v)
    with np.errstate(all="ignore"):
        want = (r64 - value.astype(np.float64)).astype(np.float32)
    assert gc.same_bits(adv[:, cols], want[:, cols])
    assert np.isnan(adv[:, ~cols]).any()


@pytest.mark.parametrize("T,B,scale,gamma", IDENTITY_CASES)
def test_lambda_one_targets_are_the_bootstrapped_returns(T, B, scale, gamma):
    reward, done, value, last, opts = gc.make_gae_case(T, B, scale=scale)
    r64 = gc.exact_rewards(reward, opts)
    _, tgt = gc.gae_reference(r64, done, value, last, gamma, 1.0)
    R = gc.returns_reference(r64, done, last, gamma)
    cols = gc.finite_columns(value, last)
    differ, worst = gc.check_lambda_one(tgt, R.astype(np.float32), np.abs(R).max(0), value, last, cols)
    print("lambda = 1, T = %d, scale %g, gamma %g: %.4f %% differ, worst %.3g of the bound"
          % (T, scale, gamma, 100 * differ, worst))


def test_every_option_set_has_a_case():
    for name, _, _ in rc.OPTION_SETS:
        reward, done, value, last, opts = gc.make_gae_case(33, 64, name)
        assert opts == rc.options_of(name)
        assert (np.signbit(value) & (value == 0)).any() and np.isinf(value[:, 6]).all()
        assert set(np.unique(done).tolist()) == {0, 1, 0x80, 0xFF}
